// Mixup kernels (reference resnet50_test.py:355-457, transformer.py:71-80).
//  * mixup_fwd:  out[i] = lam[i]*x[i] + (1-lam[i])*x[perm[i]]   (permuted gather + lerp)
//  * mixup_bwd:  gx[i] = lam[i]*g[i] + (1-lam[inv[i]])*g[inv[i]]  (inverse-permutation
//                gather: no atomics, deterministic); optional per-sample
//                dlam[i] = sum_j g[i,j]*(x[i,j]-x[perm[i],j]) for the learnable meta-mixup.
//  * mixup_ce_fwd: fused log-softmax cross entropy against two targets with per-sample
//                lambda: loss, dlogits and dloss/dlam in one single-block kernel (the
//                logits are tiny: B x 10 / B x 4), no host sync.  mixup_ce_smooth_fwd is the
//                label-smoothed instantiation (target (1-eps)*mix + eps/C).
//  * cutmix_prep / cutmix_fwd / cutmix_bwd: CutMix (Yun et al. 2019).  One workgroup draws the
//                permutation (mixup_prep's, for the same seed) and the clipped boxes; the
//                forward is a pure select out[i] = box_i ? x[perm[i]] : x[i] that reads only the
//                source it needs; the backward gathers through the inverse permutation.
#include "common.h"

#include <type_traits>

namespace fdt {

template <typename T>
__global__ __launch_bounds__(256) void mixup_fwd_kernel(const T* __restrict__ x, const int* __restrict__ perm,
                                                        const float* __restrict__ lam, T* __restrict__ out, long inner) {
  const int i = blockIdx.y;
  const int j = perm[i];
  const float l = lam[i];
  const T* xi = x + (long)i * inner;
  const T* xj = x + (long)j * inner;
  T* o = out + (long)i * inner;
  if (inner % 8 == 0) {
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < inner / 8; v += (long)gridDim.x * blockDim.x) {
      float a[8], b[8];
      Vec8<T>::load(xi + v * 8, a);
      Vec8<T>::load(xj + v * 8, b);
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = l * a[k] + (1.f - l) * b[k];
      Vec8<T>::store(o + v * 8, a);
    }
  } else {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < inner; e += (long)gridDim.x * blockDim.x)
      o[e] = from_f<T>(l * to_f(xi[e]) + (1.f - l) * to_f(xj[e]));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mixup_bwd_kernel(const T* __restrict__ g, const T* __restrict__ x,
                                                        const int* __restrict__ perm, const int* __restrict__ inv,
                                                        const float* __restrict__ lam, T* __restrict__ gx,
                                                        float* __restrict__ dlam, long inner) {
  __shared__ float sm[4];
  const int i = blockIdx.x;
  const int ii = inv[i], pj = perm[i];
  const float li = lam[i], lk = 1.f - lam[ii];
  const T* gi = g + (long)i * inner;
  const T* gk = g + (long)ii * inner;
  const T* xi = x + (long)i * inner;
  const T* xp = x + (long)pj * inner;
  T* o = gx + (long)i * inner;
  float acc = 0.f;
  for (long e = threadIdx.x; e < inner; e += blockDim.x) {
    float gv = to_f(gi[e]);
    o[e] = from_f<T>(li * gv + lk * to_f(gk[e]));
    if (dlam) acc += gv * (to_f(xi[e]) - to_f(xp[e]));
  }
  if (dlam) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dlam[i] = sm[0] + sm[1] + sm[2] + sm[3];
  }
}

// One row per THREAD when C <= 64 (CIFAR: 10 classes -- a wave per row would idle 54 of
// its 64 lanes and serialise B/16 rows per wave), one row per WAVE otherwise.
// SMOOTH: label smoothing eps in (0,1): target (1-eps)*(lam*onehot(a) + (1-lam)*onehot(b)) + eps/C,
// i.e. loss = (1-eps)*(lam*ce_a + (1-lam)*ce_b) + eps*(lse - mean_c(row)).  Every smoothing term
// sits under `if constexpr (SMOOTH)`: the SMOOTH = false instantiation is the unsmoothed kernel.
template <typename T, typename L, bool ROW_PER_THREAD, bool SMOOTH>
__global__ __launch_bounds__(1024) void mixup_ce_kernel(const T* __restrict__ logits, const L* __restrict__ ya,
                                                        const L* __restrict__ yb, const float* __restrict__ lam,
                                                        float lam_s, float* __restrict__ loss, T* __restrict__ glog,
                                                        float* __restrict__ dlam, float* __restrict__ meter, int B,
                                                        int C, float eps) {
  // meter (optional): training accumulators [loss sum, lambda-weighted correct, samples]
  // updated in place (one block: plain read-modify-write) -- the reference's per-batch
  // accuracy bookkeeping (resnet50_test.py:550-558) without a dozen separate launches.
  __shared__ float sm[16], smc[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float tot = 0.f, corr = 0.f;
  const float invB = 1.f / (float)B;
  [[maybe_unused]] const float keep = 1.f - eps, unif = eps / (float)C;
  if constexpr (ROW_PER_THREAD) {
    for (int r = threadIdx.x; r < B; r += blockDim.x) {
      const T* row = logits + (long)r * C;
      // (the row is re-read from L1 per pass: a runtime-indexed register array would spill)
      float mx = -INFINITY;
      int am = 0;
      for (int c = 0; c < C; ++c) {
        const float x = to_f(row[c]);
        if (x > mx) { mx = x; am = c; }  // strict >: first occurrence (torch.argmax)
      }
      float se = 0.f;
      [[maybe_unused]] float sx = 0.f;
      for (int c = 0; c < C; ++c) {
        se += __expf(to_f(row[c]) - mx);
        if constexpr (SMOOTH) sx += to_f(row[c]);
      }
      const float lse = mx + __logf(se);
      const int a = (int)ya[r], b = (int)yb[r];
      const float l = lam ? lam[r] : lam_s;
      const float cea = lse - to_f(row[a]), ceb = lse - to_f(row[b]);
      for (int c = 0; c < C; ++c) {
        const float p = __expf(to_f(row[c]) - lse);
        float t = (c == a ? l : 0.f) + (c == b ? 1.f - l : 0.f);
        if constexpr (SMOOTH) t = keep * t + unif;
        glog[(long)r * C + c] = from_f<T>((p - t) * invB);
      }
      if constexpr (SMOOTH) {
        tot += keep * (l * cea + (1.f - l) * ceb) + eps * (lse - sx / (float)C);
        if (dlam) dlam[r] = keep * (cea - ceb) * invB;
      } else {
        tot += l * cea + (1.f - l) * ceb;
        if (dlam) dlam[r] = (cea - ceb) * invB;
      }
      corr += (am == a ? l : 0.f) + (am == b ? 1.f - l : 0.f);
    }
    tot = wave_sum(tot);
    corr = wave_sum(corr);
  } else {
    for (int r = w; r < B; r += nw) {
      const T* row = logits + (long)r * C;
      float mx = -INFINITY;
      for (int c = lane; c < C; c += 64) mx = fmaxf(mx, to_f(row[c]));
      mx = wave_max(mx);
      float se = 0.f;
      [[maybe_unused]] float sx = 0.f;
      for (int c = lane; c < C; c += 64) {
        se += __expf(to_f(row[c]) - mx);
        if constexpr (SMOOTH) sx += to_f(row[c]);
      }
      se = wave_sum(se);
      if constexpr (SMOOTH) sx = wave_sum(sx);
      const float lse = mx + __logf(se);
      const int a = (int)ya[r], b = (int)yb[r];
      int am = C;  // argmax, first occurrence (torch.argmax)
      if (meter) {
        for (int c = lane; c < C; c += 64)
          if (to_f(row[c]) == mx) { am = c; break; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
      }
      const float l = lam ? lam[r] : lam_s;
      const float cea = lse - to_f(row[a]), ceb = lse - to_f(row[b]);
      for (int c = lane; c < C; c += 64) {
        float p = __expf(to_f(row[c]) - lse);
        float t = (c == a ? l : 0.f) + (c == b ? 1.f - l : 0.f);
        if constexpr (SMOOTH) t = keep * t + unif;
        glog[(long)r * C + c] = from_f<T>((p - t) * invB);
      }
      if (lane == 0) {
        if constexpr (SMOOTH) {
          tot += keep * (l * cea + (1.f - l) * ceb) + eps * (lse - sx / (float)C);
          if (dlam) dlam[r] = keep * (cea - ceb) * invB;
        } else {
          tot += l * cea + (1.f - l) * ceb;
          if (dlam) dlam[r] = (cea - ceb) * invB;
        }
        corr += (am == a ? l : 0.f) + (am == b ? 1.f - l : 0.f);
      }
    }
  }
  if (lane == 0) { sm[w] = tot; smc[w] = corr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f, cc = 0.f;
    for (int k = 0; k < nw; ++k) { t += sm[k]; cc += smc[k]; }
    *loss = t * invB;
    if (meter) {
      meter[0] += t * invB;
      meter[1] += cc;
      meter[2] += (float)B;
    }
  }
}

#define DISPATCH_T(dt, ...)                                     \
  switch (dt) {                                                 \
    case kF32: { using T = float; __VA_ARGS__; break; }         \
    case kBF16: { using T = bf16; __VA_ARGS__; break; }         \
    case kF16: { using T = f16; __VA_ARGS__; break; }           \
    default: throw std::runtime_error("bad dtype code");        \
  }

void mixup_fwd(uint64_t x, uint64_t perm, uint64_t lam, uint64_t out, int b, long inner, int dt, uint64_t stream) {
  long work = inner % 8 == 0 ? inner / 8 : inner;
  int gx = (int)((work + 255) / 256);
  if (gx > 64) gx = 64;
  dim3 grid(gx, b);
  DISPATCH_T(dt, {
    mixup_fwd_kernel<T><<<grid, 256, 0, as_stream(stream)>>>(P<const T>(x), P<const int>(perm), P<const float>(lam),
                                                            P<T>(out), inner);
  });
  FDT_LAUNCH_CHECK();
}

void mixup_bwd(uint64_t g, uint64_t x, uint64_t perm, uint64_t inv, uint64_t lam, uint64_t gx, uint64_t dlam, int b,
               long inner, int dt, uint64_t stream) {
  DISPATCH_T(dt, {
    mixup_bwd_kernel<T><<<b, 256, 0, as_stream(stream)>>>(P<const T>(g), P<const T>(x), P<const int>(perm),
                                                         P<const int>(inv), P<const float>(lam), P<T>(gx),
                                                         P<float>(dlam), inner);
  });
  FDT_LAUNCH_CHECK();
}

template <bool SMOOTH>
static void mixup_ce_launch(uint64_t logits, uint64_t ya, uint64_t yb, uint64_t lam, float lam_s, uint64_t loss,
                            uint64_t glog, uint64_t dlam, uint64_t meter, int B, int C, int dt, int labels64, float eps,
                            uint64_t stream) {
  auto go = [&](auto tag_t, auto tag_l) {
    using T = decltype(tag_t);
    using L = decltype(tag_l);
    if (C <= 64)
      mixup_ce_kernel<T, L, true, SMOOTH><<<1, 1024, 0, as_stream(stream)>>>(
          P<const T>(logits), P<const L>(ya), P<const L>(yb), P<const float>(lam), lam_s, P<float>(loss), P<T>(glog),
          P<float>(dlam), P<float>(meter), B, C, eps);
    else
      mixup_ce_kernel<T, L, false, SMOOTH><<<1, 1024, 0, as_stream(stream)>>>(
          P<const T>(logits), P<const L>(ya), P<const L>(yb), P<const float>(lam), lam_s, P<float>(loss), P<T>(glog),
          P<float>(dlam), P<float>(meter), B, C, eps);
  };
  DISPATCH_T(dt, {
    if (labels64) go(T{}, int64_t{});
    else go(T{}, int{});
  });
  FDT_LAUNCH_CHECK();
}

void mixup_ce_fwd(uint64_t logits, uint64_t ya, uint64_t yb, uint64_t lam, float lam_s, uint64_t loss, uint64_t glog,
                  uint64_t dlam, uint64_t meter, int B, int C, int dt, int labels64, uint64_t stream) {
  mixup_ce_launch<false>(logits, ya, yb, lam, lam_s, loss, glog, dlam, meter, B, C, dt, labels64, 0.f, stream);
}

void mixup_ce_smooth_fwd(uint64_t logits, uint64_t ya, uint64_t yb, uint64_t lam, float lam_s, uint64_t loss,
                         uint64_t glog, uint64_t dlam, uint64_t meter, int B, int C, int dt, int labels64, float eps,
                         uint64_t stream) {
  FDT_CHECK(eps >= 0.f && eps < 1.f, "mixup_ce_smooth_fwd: 0 <= eps < 1");
  FDT_CHECK(B >= 1 && C >= 1, "mixup_ce_smooth_fwd: empty logits");
  mixup_ce_launch<true>(logits, ya, yb, lam, lam_s, loss, glog, dlam, meter, B, C, dt, labels64, eps, stream);
}

// One workgroup: a uniformly random permutation of b <= 1024 samples (bitonic sort in LDS of
// 64-bit counter-hash keys -- distinct, the hash is a bijection), the permuted labels and the
// per-sample lambda vector: replaces randperm's sort passes, the int32 cast, the label gather
// and the lambda fill of an input-mixup step (reference resnet50_test.py:355-376).
// (shared by mixup_prep and cutmix_prep: the same seed gives the same permutation)  On return
// idx[0..b) is the permutation; key / idx are LDS arrays of 1024 entries.
__device__ __forceinline__ void sort_permutation(uint64_t seed, int b, uint64_t* key, int* idx) {
  int n = 1;
  while (n < b) n <<= 1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    key[i] = i < b ? mix64(seed + (uint64_t)i * 0xD1B54A32D192ED03ull) : ~0ull;
    idx[i] = i;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int p = i ^ j;
        if (p > i) {
          const bool up = (i & k) == 0;
          const uint64_t a = key[i], c = key[p];
          if ((a > c) == up) {
            key[i] = c;
            key[p] = a;
            const int t = idx[i];
            idx[i] = idx[p];
            idx[p] = t;
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(1024) void mixup_prep_kernel(const int64_t* __restrict__ y, int b, float lam,
                                                          uint64_t seed, int* __restrict__ perm,
                                                          int64_t* __restrict__ yb, float* __restrict__ lam_vec) {
  __shared__ uint64_t key[1024];
  __shared__ int idx[1024];
  sort_permutation(seed, b, key, idx);
  for (int i = threadIdx.x; i < b; i += blockDim.x) {
    const int j = idx[i];
    perm[i] = j;
    yb[i] = y[j];
    lam_vec[i] = lam;
  }
}

void mixup_prep(uint64_t y, int b, float lam, uint64_t seed, uint64_t perm, uint64_t yb, uint64_t lam_vec,
                uint64_t stream) {
  FDT_CHECK(b >= 1 && b <= 1024, "mixup_prep: 1 <= batch <= 1024");
  mixup_prep_kernel<<<1, 1024, 0, as_stream(stream)>>>(P<const int64_t>(y), b, lam, seed, P<int>(perm),
                                                       P<int64_t>(yb), P<float>(lam_vec));
  FDT_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------- CutMix
// Box centres come from a second stream of the seed (the permutation keys use the first):
// sample i (or 0 for one box per batch) -> mix64 -> cy = (high word * H) >> 32, cx = (low word * W)
// >> 32 (multiply-shift range reduction: no division in the one workgroup that every step waits for).
// Integer arithmetic only; ops/mixup.py cutmix_boxes is the bit-exact host mirror.
constexpr uint64_t kCutmixStream = 0xC2B2AE3D27D4EB4Full;

__global__ __launch_bounds__(1024) void cutmix_prep_kernel(const int64_t* __restrict__ y, int b, int H, int W, int bh,
                                                           int bw, int per_sample, uint64_t seed,
                                                           int* __restrict__ perm, int64_t* __restrict__ yb,
                                                           int* __restrict__ box, float* __restrict__ lam_vec) {
  __shared__ uint64_t key[1024];
  __shared__ int idx[1024];
  sort_permutation(seed, b, key, idx);
  for (int i = threadIdx.x; i < b; i += blockDim.x) {
    const int j = idx[i];
    perm[i] = j;
    yb[i] = y[j];
    const uint64_t h = mix64((seed ^ kCutmixStream) + (uint64_t)(per_sample ? i : 0) * 0x9E3779B97F4A7C15ull);
    const int cy = (int)__umulhi((uint32_t)(h >> 32), (uint32_t)H), cx = (int)__umulhi((uint32_t)h, (uint32_t)W);
    const int y0 = max(cy - bh / 2, 0), y1 = min(cy + bh / 2, H);
    const int x0 = max(cx - bw / 2, 0), x1 = min(cx + bw / 2, W);
    reinterpret_cast<int4*>(box)[i] = make_int4(y0, y1, x0, x1);
    lam_vec[i] = 1.f - (float)((y1 - y0) * (x1 - x0)) / (float)(H * W);
  }
}

void cutmix_prep(uint64_t y, int b, int H, int W, int bh, int bw, int per_sample, uint64_t seed, uint64_t perm,
                 uint64_t yb, uint64_t box, uint64_t lam_vec, uint64_t stream) {
  FDT_CHECK(b >= 1 && b <= 1024, "cutmix_prep: 1 <= batch <= 1024");
  FDT_CHECK(H >= 1 && W >= 1 && (long)H * W < (1l << 24), "cutmix_prep: 1 <= H*W < 2^24");
  FDT_CHECK(bh >= 0 && bh <= H && bw >= 0 && bw <= W, "cutmix_prep: 0 <= bh <= H, 0 <= bw <= W");
  FDT_CHECK(box % 16 == 0, "cutmix_prep: box rows are stored 16 bytes at a time");
  cutmix_prep_kernel<<<1, 1024, 0, as_stream(stream)>>>(P<const int64_t>(y), b, H, W, bh, bw, per_sample, seed,
                                                        P<int>(perm), P<int64_t>(yb), P<int>(box), P<float>(lam_vec));
  FDT_LAUNCH_CHECK();
}

// Eight consecutive elements as raw bits (16 B for bf16 / f16, 2 x 16 B for f32): CutMix moves
// bits, it never converts.
template <typename T>
struct Raw8 {
  using U = typename std::conditional<sizeof(T) == 2, uint16_t, uint32_t>::type;
  static constexpr int kQ = (int)sizeof(T) / 2;
  union {
    uint4 q[kQ];
    U e[8];
  };
  __device__ __forceinline__ void load(const T* p) {
#pragma unroll
    for (int k = 0; k < kQ; ++k) q[k] = reinterpret_cast<const uint4*>(p)[k];
  }
  __device__ __forceinline__ void store(T* p) const {
#pragma unroll
    for (int k = 0; k < kQ; ++k) reinterpret_cast<uint4*>(p)[k] = q[k];
  }
};

// A sample is `inner` elements; element e lies at image position t = e / xdiv, w = t % W,
// h = (t / W) % H.  xdiv = 1: contiguous NCHW (a vector of 8 spans 8 columns, W % 8 == 0);
// xdiv = cp (a multiple of 8): zero-padded NHWC, a vector lies inside one pixel.  A vector
// wholly inside or wholly outside the box loads one source; only an NCHW vector that straddles
// a box edge loads both and selects per element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void cutmix_fwd_kernel(const T* __restrict__ x, const int* __restrict__ perm,
                                                         const int* __restrict__ box, T* __restrict__ out,
                                                         uint32_t inner, uint32_t H, uint32_t W, uint32_t xdiv) {
  const int i = blockIdx.y;
  const int j = perm[i];
  const uint32_t y0 = box[4 * i], y1 = box[4 * i + 1], x0 = box[4 * i + 2], x1 = box[4 * i + 3];
  const T* xi = x + (long)i * inner;
  const T* xj = x + (long)j * inner;
  T* o = out + (long)i * inner;
  const uint32_t stride = gridDim.x * blockDim.x;
  if constexpr (VEC) {
    const uint32_t span = xdiv == 1 ? 8u : 1u;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < inner / 8; v += stride) {
      const uint32_t e = v * 8, t = e / xdiv, w = t % W, h = (t / W) % H;
      const bool row = h >= y0 && h < y1;
      const bool all = row && w >= x0 && w + span <= x1;
      const bool none = !row || w + span <= x0 || w >= x1;
      Raw8<T> a;
      if (all) {
        a.load(xj + e);
      } else {
        a.load(xi + e);
        if (!none) {
          Raw8<T> c;
          c.load(xj + e);
#pragma unroll
          for (uint32_t k = 0; k < 8; ++k)
            if (w + k >= x0 && w + k < x1) a.e[k] = c.e[k];
        }
      }
      a.store(o + e);
    }
  } else {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < inner; e += stride) {
      const uint32_t t = e / xdiv, w = t % W, h = (t / W) % H;
      const bool in = h >= y0 && h < y1 && w >= x0 && w < x1;
      o[e] = in ? xj[e] : xi[e];
    }
  }
}

// gx[i] = g[i] outside box i, plus g[inv[i]] inside box inv[i] (inverse-permutation gather: no
// atomics, deterministic).  A fixed point (inv[i] == i) adds up to g[i] everywhere.
template <typename T>
__global__ __launch_bounds__(256) void cutmix_bwd_kernel(const T* __restrict__ g, const int* __restrict__ inv,
                                                         const int* __restrict__ box, T* __restrict__ gx,
                                                         uint32_t inner, uint32_t H, uint32_t W, uint32_t xdiv) {
  const int i = blockIdx.y;
  const int ii = inv[i];
  const uint32_t y0 = box[4 * i], y1 = box[4 * i + 1], x0 = box[4 * i + 2], x1 = box[4 * i + 3];
  const uint32_t u0 = box[4 * ii], u1 = box[4 * ii + 1], v0 = box[4 * ii + 2], v1 = box[4 * ii + 3];
  const T* gi = g + (long)i * inner;
  const T* gk = g + (long)ii * inner;
  T* o = gx + (long)i * inner;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < inner; e += gridDim.x * blockDim.x) {
    const uint32_t t = e / xdiv, w = t % W, h = (t / W) % H;
    const bool own = !(h >= y0 && h < y1 && w >= x0 && w < x1);
    const bool got = h >= u0 && h < u1 && w >= v0 && w < v1;
    if (own && got) o[e] = from_f<T>(to_f(gi[e]) + to_f(gk[e]));
    else if (own) o[e] = gi[e];
    else if (got) o[e] = gk[e];
    else o[e] = from_f<T>(0.f);
  }
}

static void cutmix_check(int b, long inner, int H, int W, int xdiv) {
  FDT_CHECK(b >= 1 && H >= 1 && W >= 1 && xdiv >= 1, "cutmix: b, H, W, xdiv >= 1");
  FDT_CHECK(inner >= 1 && inner < (1l << 31), "cutmix: 1 <= elements per sample < 2^31");
  FDT_CHECK(inner % ((long)H * W * xdiv) == 0, "cutmix: elements per sample must be a multiple of H*W*xdiv");
  FDT_CHECK(xdiv == 1 || inner == (long)H * W * xdiv, "cutmix: padded NHWC holds one H x W x cp block per sample");
  FDT_CHECK(b <= 65535, "cutmix: batch <= 65535");
}

void cutmix_fwd(uint64_t x, uint64_t perm, uint64_t box, uint64_t out, int b, long inner, int H, int W, int xdiv,
                int dt, uint64_t stream) {
  cutmix_check(b, inner, H, W, xdiv);
  const bool vec = (xdiv == 1 ? W % 8 == 0 : xdiv % 8 == 0) && x % 16 == 0 && out % 16 == 0;
  const long work = vec ? inner / 8 : inner;
  int gx = (int)((work + 255) / 256);
  if (gx > 64) gx = 64;
  dim3 grid(gx, b);
  DISPATCH_T(dt, {
    if (vec)
      cutmix_fwd_kernel<T, true><<<grid, 256, 0, as_stream(stream)>>>(P<const T>(x), P<const int>(perm),
                                                                      P<const int>(box), P<T>(out), (uint32_t)inner,
                                                                      (uint32_t)H, (uint32_t)W, (uint32_t)xdiv);
    else
      cutmix_fwd_kernel<T, false><<<grid, 256, 0, as_stream(stream)>>>(P<const T>(x), P<const int>(perm),
                                                                       P<const int>(box), P<T>(out), (uint32_t)inner,
                                                                       (uint32_t)H, (uint32_t)W, (uint32_t)xdiv);
  });
  FDT_LAUNCH_CHECK();
}

void cutmix_bwd(uint64_t g, uint64_t inv, uint64_t box, uint64_t gx, int b, long inner, int H, int W, int xdiv, int dt,
                uint64_t stream) {
  cutmix_check(b, inner, H, W, xdiv);
  int nb = (int)((inner + 255) / 256);
  if (nb > 64) nb = 64;
  dim3 grid(nb, b);
  DISPATCH_T(dt, {
    cutmix_bwd_kernel<T><<<grid, 256, 0, as_stream(stream)>>>(P<const T>(g), P<const int>(inv), P<const int>(box),
                                                             P<T>(gx), (uint32_t)inner, (uint32_t)H, (uint32_t)W,
                                                             (uint32_t)xdiv);
  });
  FDT_LAUNCH_CHECK();
}

}  // namespace fdt
