// Per-channel batch-norm finalisation math shared by the standalone finalize kernel
// (bn_kernels.hip) and any kernel that finalises statistics in its own epilogue,
// so both produce bit-identical (s, t) for the same fp64 sums.
//
// mode 0: FusedConvBN (unbiased var, s = 1/(sqrt(var)+eps), no affine)   resnet.py:75-100
// mode 1: BatchNorm2d train (biased var + eps, affine, running stats with momentum and the
//         unbiased var)
// mode 2: BatchNorm2d eval  (running stats, affine)
// mode 3: FusedConvBN train, tracked: mode 0's outputs, plus running stats like mode 1 (the
//         unbiased var mode 0 computes)
// save_mean[c], save_aux[c]: modes 0/3 -> sd ; modes 1/2 -> invstd
// momentum < 0 (modes 1 / 3): cumulative average, factor 1 / (num_batches_tracked + 1) -- PyTorch's
// momentum=None; the launcher then increments nbt after the finalize kernel (every channel reads
// the same count), otherwise the channel-0 thread increments it in place.
#pragma once
#include "common.h"

namespace fdt {

struct FinArgs {
  int mode;
  float eps;
  float momentum;
  double count;
  const float* gamma;
  const float* beta;
  float* run_mean;
  float* run_var;
  long long* nbt;
  float* out_s;
  float* out_t;
  float* save_mean;
  float* save_aux;
};

// running statistics of channel c (modes 1 / 3) <- this batch's mean and unbiased variance
__device__ __forceinline__ void bn_track(const FinArgs& f, int c, double mean, double var_u) {
  if (f.run_mean) {
    const double m = f.momentum < 0.f ? 1.0 / (double)(f.nbt[0] + 1) : (double)f.momentum;
    f.run_mean[c] = (float)((1.0 - m) * f.run_mean[c] + m * mean);
    f.run_var[c] = (float)((1.0 - m) * f.run_var[c] + m * var_u);
  }
  if (f.nbt && c == 0 && f.momentum >= 0.f) f.nbt[0] += 1;
}

// (s, t) of channel c from its fp64 sums; ``write``: also the unit's outputs (out_s / out_t,
// saved mean / aux, running statistics, num_batches_tracked) -- exactly one thread per channel
// may write them
__device__ __forceinline__ void bn_finalize_st(const FinArgs& f, int c, double S, double Q, float& s_out,
                                               float& t_out, bool write) {
  double sc, tt, mean, aux;
  if (f.mode == 0 || f.mode == 3) {
    mean = S / f.count;
    double var = (Q - S * mean) / (f.count - 1.0);
    if (var < 0.0) var = 0.0;
    aux = sqrt(var);
    sc = 1.0 / (aux + (double)f.eps);
    tt = -mean * sc;
    if (f.mode == 3 && write) bn_track(f, c, mean, var);
  } else if (f.mode == 1) {
    mean = S / f.count;
    double m2 = Q - S * mean;
    if (m2 < 0.0) m2 = 0.0;
    const double var_b = m2 / f.count;
    const double var_u = f.count > 1.0 ? m2 / (f.count - 1.0) : var_b;
    aux = 1.0 / sqrt(var_b + (double)f.eps);
    const double g = f.gamma ? (double)f.gamma[c] : 1.0, b = f.beta ? (double)f.beta[c] : 0.0;
    sc = g * aux;
    tt = b - mean * g * aux;
    if (write) bn_track(f, c, mean, var_u);
  } else {
    mean = f.run_mean[c];
    aux = 1.0 / sqrt((double)f.run_var[c] + (double)f.eps);
    const double g = f.gamma ? (double)f.gamma[c] : 1.0, b = f.beta ? (double)f.beta[c] : 0.0;
    sc = g * aux;
    tt = b - mean * g * aux;
  }
  s_out = (float)sc;
  t_out = (float)tt;
  if (write) {
    f.out_s[c] = s_out;
    f.out_t[c] = t_out;
    f.save_mean[c] = (float)mean;
    f.save_aux[c] = (float)aux;
  }
}

__device__ __forceinline__ void bn_finalize_channel(const FinArgs& f, int c, double S, double Q) {
  float s, t;
  bn_finalize_st(f, c, S, Q, s, t, true);
}

// BN-backward coefficients from the per-channel reductions (g_s, g_t) of dL/dy; see the mode
// table above stats_bwd_coef_kernel (bn_kernels.hip).
struct CoefArgs {
  int mode;
  float eps;
  double count;
  const float* save_mean;
  const float* save_aux;
  const float* gamma;
  float* alpha;
  float* beta;
  float* ggamma;
  float* gbeta;
};

__device__ __forceinline__ void bwd_coef_one(const CoefArgs& a, int c, double g_s, double g_t) {
  const double mean = a.save_mean[c], aux = a.save_aux[c];
  const double count = a.count;
  if (a.mode == 0) {
    const double sd = aux;
    const double s = 1.0 / (sd + (double)a.eps);
    const double b = sd > 0.0 ? -(g_s - mean * g_t) * s * s / ((count - 1.0) * sd) : 0.0;
    a.beta[c] = (float)b;
    a.alpha[c] = (float)(-b * mean - g_t * s / count);
  } else {
    const double inv = aux;
    const double g = a.gamma ? (double)a.gamma[c] : 1.0;
    const double s = g * inv;
    if (a.mode == 1) {
      const double b = -(g_s - mean * g_t) * g * inv * inv * inv / count;
      a.beta[c] = (float)b;
      a.alpha[c] = (float)(-b * mean - g_t * s / count);
    } else {
      a.beta[c] = 0.f;
      a.alpha[c] = 0.f;
    }
    // accumulate (+=) into the parameter gradients (flat gradient views)
    if (a.ggamma) a.ggamma[c] += (float)((g_s - mean * g_t) * inv);
    if (a.gbeta) a.gbeta[c] += (float)g_t;
  }
}

}  // namespace fdt
