// Layer-wise adaptive rates over the FLAT buffers: LARS (SGD + momentum, You et al. 2017) and
// LAMB (AdamW, You et al. 2019).
//
// The step kernels of optim.hip are slot-agnostic element streams; a trust ratio needs the norm
// of every parameter tensor ("slot" of utils/flat.py).  Instead of two norm launches and a host
// scalar per tensor, the host cuts every slot into tiles of at most kLayerTile elements ONCE per
// layout and the step is three launches over that table:
//   LARS: slot_sumsq (p, g)  -> slot_finalize -> lars_apply
//   LAMB: lamb_moments (m, v in place; partials of p, u) -> slot_finalize -> lamb_apply
// Table rows are int32 x 4 (one 16-byte load):
//   tiles[t] = {slot, first element, element count, first tile of the slot}
//   slots[s] = {first tile, tile count, adapted (trust ratio applies), decayed (weight decay applies)}
// Tiles cover exactly the numel elements of a slot: the alignment padding between slots belongs
// to no tile, is never summed and never written.  Slot offsets are multiples of 64 elements and
// a slot's storage is padded to a multiple of 64, so every tile start is 16-byte aligned and the
// float4 holding a slot's last elements lies inside the buffer; its lanes past the element count
// are masked (reductions) or handled element-wise (updates).
//
// Determinism: no atomics.  A tile partial is the per-lane float4 stream, then wave_sum, then an
// LDS combine in wave order; slot_finalize adds a slot's partials in a fixed order in fp64.  DDP
// replicas, which each run the whole step on the same all-reduced gradients, stay bitwise equal.
//
// Skipped steps (device found_inf flag): the reductions return at once (trust may hold anything);
// the apply kernel leaves p / state / shadow alone, clears the slots' gradients when it owns
// zero_grad, and -- LAMB -- bumps kskip once.  Only the apply kernels zero the gradient: pass A of
// LAMB reads it, so the whole skip / zero logic of a step sits in its last launch.
#include "common.h"
#include "optim_ops.h"

namespace fdt {
namespace {

constexpr int kLB = 256;           // threads per workgroup
constexpr int kLW = kLB / 64;      // waves per workgroup
constexpr int kLayerTile = 4096;   // elements per tile: 4 float4 per lane
constexpr int kMaxGrid = 16384;    // workgroups; more tiles than that are walked grid-stride

inline int tile_grid(int ntiles) { return ntiles < 1 ? 1 : (ntiles > kMaxGrid ? kMaxGrid : ntiles); }

__device__ __forceinline__ void store_shadow4(bf16* sh, long i, float4 v) {
  uint2 u;
  u.x = pack_bf16x2(v.x, v.y);
  u.y = pack_bf16x2(v.z, v.w);
  *reinterpret_cast<uint2*>(sh + i) = u;
}

// lanes of the float4 at tile element e that lie past the tile's n elements read padding: zeroed
__device__ __forceinline__ float4 mask_tail(float4 v, int e, int n) {
  if (e + 1 >= n) v.y = 0.f;
  if (e + 2 >= n) v.z = 0.f;
  if (e + 3 >= n) v.w = 0.f;
  return v;
}

// workgroup sums of two per-lane accumulators in a fixed order -> out[0..1] (thread 0 writes)
__device__ __forceinline__ void tile_partials(float a, float b, float* __restrict__ out) {
  __shared__ float sm[2][kLW];
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sm[0][threadIdx.x >> 6] = a;
    sm[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = 0.f, tb = 0.f;
    for (int w = 0; w < kLW; ++w) {
      ta += sm[0][w];
      tb += sm[1][w];
    }
    out[0] = ta;
    out[1] = tb;
  }
  __syncthreads();  // (sm is reused by the next tile of a grid-stride walk)
}

// a skipped step still clears the gradient of every slot element (never the padding)
__device__ __forceinline__ void zero_tile(float* __restrict__ g, int n) {
  for (int e = threadIdx.x * 4; e < n; e += kLB * 4) {
    if (e + 4 <= n) {
      *reinterpret_cast<float4*>(g + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int k = 0; k < n - e; ++k) g[e + k] = 0.f;
    }
  }
}

// ------------------------------------------------------------------ per-tile sums of squares
// part[t] = {sum a^2, sum b^2} over the elements of tile t
__global__ __launch_bounds__(kLB) void slot_sumsq_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const int4* __restrict__ tiles, int ntiles,
                                                         float* __restrict__ part, const int* __restrict__ found_inf) {
  if (opt::skip_step(found_inf)) return;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int4 row = tiles[t];
    const float* at = a + row.y;
    const float* bt = b + row.y;
    const int n = row.z;
    float sa = 0.f, sb = 0.f;
    for (int e = threadIdx.x * 4; e < n; e += kLB * 4) {
      const float4 av = mask_tail(*reinterpret_cast<const float4*>(at + e), e, n);
      const float4 bv = mask_tail(*reinterpret_cast<const float4*>(bt + e), e, n);
      sa += av.x * av.x + av.y * av.y + av.z * av.z + av.w * av.w;
      sb += bv.x * bv.x + bv.y * bv.y + bv.z * bv.z + bv.w * bv.w;
    }
    tile_partials(sa, sb, part + 2 * (long)t);
  }
}

// ------------------------------------------------------------------ trust ratio per slot
// One wave per slot: the slot's tile partials (first column: p, second: g or u) are added in a
// fixed order in fp64 (lane l takes tiles l, l+64, ..., then the wave butterfly).
//   LARS: wn = |p|, gn = c |g|;  q = eta wn / (gn + wd_s wn + eps)
//   LAMB: wn = |p|, un = |u|;    q = wn / un       (the clip coefficient is already inside u)
// q = 1 where the slot is not adapted or a norm is zero.  The clip coefficient c (device scalar,
// may be null) enters here, not in the reduction: |c g| = c |g|.
__global__ __launch_bounds__(kLB) void slot_finalize_kernel(const float* __restrict__ part, const int4* __restrict__ slots,
                                                            int nslots, int lamb, double eta, double wd, double eps,
                                                            const float* __restrict__ gsc,
                                                            const int* __restrict__ found_inf, float* __restrict__ trust,
                                                            float* __restrict__ norms) {
  if (opt::skip_step(found_inf)) return;
  const int s = blockIdx.x * kLW + (threadIdx.x >> 6);
  if (s >= nslots) return;
  const int lane = threadIdx.x & 63;
  const int4 sl = slots[s];
  double a = 0.0, b = 0.0;
  for (int i = lane; i < sl.y; i += 64) {
    a += (double)part[2 * (long)(sl.x + i)];
    b += (double)part[2 * (long)(sl.x + i) + 1];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    const double wn = sqrt(a);
    const double on = lamb ? sqrt(b) : (double)opt::gscale(gsc) * sqrt(b);
    double q = 1.0;
    if (sl.z && wn > 0.0 && on > 0.0) q = lamb ? wn / on : eta * wn / (on + (sl.w ? wd : 0.0) * wn + eps);
    trust[s] = (float)q;
    norms[2 * s] = (float)wn;
    norms[2 * s + 1] = (float)on;
  }
}

// ------------------------------------------------------------------ LARS apply
// The rule is opt::SgdOp's (optim_ops.h) with the slot's coefficient folded into its two
// scalars: d = g (q c) + (q wd_s) p, then SGD's momentum / nesterov / lr step unchanged.  With
// q = 1 this IS the sgd_kernel rule, bit for bit.
__global__ __launch_bounds__(kLB) void lars_apply_kernel(const opt::SgdArgs args, const int4* __restrict__ tiles,
                                                         int ntiles, const int4* __restrict__ slots,
                                                         const float* __restrict__ trust) {
  if (opt::SgdOp::skipped(args)) {
    if (args.zero_grad)
      for (int t = blockIdx.x; t < ntiles; t += gridDim.x) zero_tile(args.g + tiles[t].y, tiles[t].z);
    return;
  }
  const opt::SgdOp base(args);
  const bool mom = base.momentum != 0.f;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int4 row = tiles[t];
    const int n = row.z;
    const float q = trust[row.x];
    opt::SgdOp op = base;
    op.c = base.c * q;
    op.a.wd = slots[row.x].w ? q * args.wd : 0.f;
    for (int e = threadIdx.x * 4; e < n; e += kLB * 4) {
      const long i = (long)row.y + e;
      if (e + 4 <= n) {
        float4 pv = *reinterpret_cast<const float4*>(args.p + i);
        const float4 gv = *reinterpret_cast<const float4*>(args.g + i);
        float4 bv = (mom && !args.first) ? *reinterpret_cast<const float4*>(args.buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        pv.x = op.rule(pv.x, gv.x, bv.x);
        pv.y = op.rule(pv.y, gv.y, bv.y);
        pv.z = op.rule(pv.z, gv.z, bv.z);
        pv.w = op.rule(pv.w, gv.w, bv.w);
        if (mom) *reinterpret_cast<float4*>(args.buf + i) = bv;
        *reinterpret_cast<float4*>(args.p + i) = pv;
        if (args.shadow) store_shadow4(args.shadow, i, pv);
        if (args.zero_grad) *reinterpret_cast<float4*>(args.g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        for (int k = 0; k < n - e; ++k) op(i + k);  // the slot's last 1-3 elements: padding follows
      }
    }
  }
}

// ------------------------------------------------------------------ LAMB
struct LambArgs {
  float *p, *g, *m, *v;
  bf16* shadow;
  float lr, b1, b2, eps, wd;
  long step;  // 1-based count of step() calls; the applied count is step - *kskip
  int* kskip;
  const float* gsc;
  const int* found_inf;
  int zero_grad;
};

struct LambOp {
  float c, b1, b2, eps, bc1, bc2;
  __device__ explicit LambOp(const LambArgs& a) : c(opt::gscale(a.gsc)), b1(a.b1), b2(a.b2), eps(a.eps) {
    const float st = (float)opt::applied_k(a.step, a.kskip);
    bc1 = 1.f - powf(b1, st);
    bc2 = 1.f - powf(b2, st);
  }
  // (no FMA contraction: pass A and the apply pass must round u identically)
  __device__ __forceinline__ void moments(float gv, float& mv, float& vv) const {
#pragma clang fp contract(off)
    gv *= c;
    mv = b1 * mv + (1.f - b1) * gv;
    vv = b2 * vv + (1.f - b2) * gv * gv;
  }
  __device__ __forceinline__ float update(float pv, float mv, float vv, float wd) const {
#pragma clang fp contract(off)
    return (mv / bc1) / (sqrtf(vv / bc2) + eps) + wd * pv;
  }
};

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4], int nv) {
  if (nv == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < nv; ++k) p[k] = v[k];
  }
}

// pass A: m, v updated in place; part[t] = {sum p^2, sum u^2} of tile t
__global__ __launch_bounds__(kLB) void lamb_moments_kernel(const LambArgs args, const int4* __restrict__ tiles, int ntiles,
                                                           const int4* __restrict__ slots, float* __restrict__ part) {
  if (opt::skip_step(args.found_inf)) return;
  const LambOp op(args);
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int4 row = tiles[t];
    const int n = row.z;
    const float wd = slots[row.x].w ? args.wd : 0.f;
    float sa = 0.f, sb = 0.f;
    for (int e = threadIdx.x * 4; e < n; e += kLB * 4) {
      const long i = (long)row.y + e;
      const int nv = n - e < 4 ? n - e : 4;
      float pv[4], gv[4], mv[4], vv[4];
      ld4(args.p + i, pv);
      ld4(args.g + i, gv);
      ld4(args.m + i, mv);
      ld4(args.v + i, vv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          op.moments(gv[k], mv[k], vv[k]);
          const float u = op.update(pv[k], mv[k], vv[k], wd);
          sa += pv[k] * pv[k];
          sb += u * u;
        }
      }
      st4(args.m + i, mv, nv);
      st4(args.v + i, vv, nv);
    }
    tile_partials(sa, sb, part + 2 * (long)t);
  }
}

// pass B: u recomputed from the stored m, v and the (still old) p; p -= lr q u
__global__ __launch_bounds__(kLB) void lamb_apply_kernel(const LambArgs args, const int4* __restrict__ tiles, int ntiles,
                                                         const int4* __restrict__ slots, const float* __restrict__ trust) {
  if (opt::skip_step(args.found_inf)) {
    // (an applied step reads kskip, a skipped one writes it: never both in one launch)
    opt::count_skip(args.kskip);
    if (args.zero_grad)
      for (int t = blockIdx.x; t < ntiles; t += gridDim.x) zero_tile(args.g + tiles[t].y, tiles[t].z);
    return;
  }
  const LambOp op(args);
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int4 row = tiles[t];
    const int n = row.z;
    const float wd = slots[row.x].w ? args.wd : 0.f;
    const float lrq = args.lr * trust[row.x];
    for (int e = threadIdx.x * 4; e < n; e += kLB * 4) {
      const long i = (long)row.y + e;
      const int nv = n - e < 4 ? n - e : 4;
      float pv[4], mv[4], vv[4];
      ld4(args.p + i, pv);
      ld4(args.m + i, mv);
      ld4(args.v + i, vv);
#pragma unroll
      for (int k = 0; k < 4; ++k) pv[k] = pv[k] - lrq * op.update(pv[k], mv[k], vv[k], wd);
      st4(args.p + i, pv, nv);
      if (args.shadow) {
        if (nv == 4) {
          store_shadow4(args.shadow, i, make_float4(pv[0], pv[1], pv[2], pv[3]));
        } else {
          for (int k = 0; k < nv; ++k) args.shadow[i + k] = __float2bfloat16(pv[k]);
        }
      }
      if (args.zero_grad) {
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        st4(args.g + i, z, nv);
      }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------ launchers
int layer_tile() { return kLayerTile; }

void slot_sumsq(uint64_t a, uint64_t b, uint64_t tiles, int ntiles, uint64_t part, uint64_t found_inf, uint64_t stream) {
  if (ntiles <= 0) return;
  slot_sumsq_kernel<<<tile_grid(ntiles), kLB, 0, as_stream(stream)>>>(P<const float>(a), P<const float>(b),
                                                                      P<const int4>(tiles), ntiles, P<float>(part),
                                                                      P<const int>(found_inf));
  FDT_LAUNCH_CHECK();
}

void slot_finalize(uint64_t part, uint64_t slots, int nslots, int lamb, double eta, double wd, double eps, uint64_t gsc,
                   uint64_t found_inf, uint64_t trust, uint64_t norms, uint64_t stream) {
  if (nslots <= 0) return;
  slot_finalize_kernel<<<(nslots + kLW - 1) / kLW, kLB, 0, as_stream(stream)>>>(
      P<const float>(part), P<const int4>(slots), nslots, lamb, eta, wd, eps, P<const float>(gsc),
      P<const int>(found_inf), P<float>(trust), P<float>(norms));
  FDT_LAUNCH_CHECK();
}

void lars_apply(uint64_t p, uint64_t g, uint64_t buf, uint64_t shadow, uint64_t tiles, int ntiles, uint64_t slots,
                uint64_t trust, float lr, float momentum, float dampening, float wd, int nesterov, int first,
                uint64_t gsc, uint64_t found_inf, int zero_grad, uint64_t stream) {
  FDT_CHECK(momentum == 0.f || buf != 0, "momentum buffer required");
  if (ntiles <= 0) return;
  const opt::SgdArgs a{P<float>(p), P<float>(g), P<float>(buf), P<bf16>(shadow), lr, momentum, dampening, wd,
                       nesterov, first, P<const float>(gsc), P<const int>(found_inf), zero_grad,
                       nullptr};  // (no device-side [lr, momentum]: the step is not captured into a graph)
  lars_apply_kernel<<<tile_grid(ntiles), kLB, 0, as_stream(stream)>>>(a, P<const int4>(tiles), ntiles,
                                                                      P<const int4>(slots), P<const float>(trust));
  FDT_LAUNCH_CHECK();
}

void lamb_moments(uint64_t p, uint64_t g, uint64_t m, uint64_t v, uint64_t tiles, int ntiles, uint64_t slots,
                  uint64_t part, float b1, float b2, float eps, float wd, long step, uint64_t kskip, uint64_t gsc,
                  uint64_t found_inf, uint64_t stream) {
  if (ntiles <= 0) return;
  const LambArgs a{P<float>(p), P<float>(g), P<float>(m), P<float>(v), nullptr, 0.f, b1, b2, eps, wd, step,
                   P<int>(kskip), P<const float>(gsc), P<const int>(found_inf), 0};
  lamb_moments_kernel<<<tile_grid(ntiles), kLB, 0, as_stream(stream)>>>(a, P<const int4>(tiles), ntiles,
                                                                        P<const int4>(slots), P<float>(part));
  FDT_LAUNCH_CHECK();
}

void lamb_apply(uint64_t p, uint64_t g, uint64_t m, uint64_t v, uint64_t shadow, uint64_t tiles, int ntiles,
                uint64_t slots, uint64_t trust, float lr, float b1, float b2, float eps, float wd, long step,
                uint64_t kskip, uint64_t found_inf, int zero_grad, uint64_t stream) {
  if (ntiles <= 0) return;
  const LambArgs a{P<float>(p), P<float>(g), P<float>(m), P<float>(v), P<bf16>(shadow), lr, b1, b2, eps, wd, step,
                   P<int>(kskip), nullptr, P<const int>(found_inf), zero_grad};
  lamb_apply_kernel<<<tile_grid(ntiles), kLB, 0, as_stream(stream)>>>(a, P<const int4>(tiles), ntiles,
                                                                      P<const int4>(slots), P<const float>(trust));
  FDT_LAUNCH_CHECK();
}

}  // namespace fdt
