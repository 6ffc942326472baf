// Exponential moving average of the weights over the FLAT parameter buffer (optim/ema.py).
//
// ema_update:  e <- fmaf(d, e - p, p)  over the whole buffer (alignment padding included; no
//   slot table).  d = decay, or min(decay, (1 + t) / (10 + t)) under warm-up, t = applied
//   updates so far = k - *kskip: the optimizers' step-count convention (optim_ops.h) -- the
//   host passes the number of update() calls, a launch that finds found_inf set changes
//   nothing in e and bumps the EMA's own device kskip, so a skipped optimizer step is a
//   skipped average as well, without a host sync.  d == 0 gives e == p bit for bit.
// ema_swap:  p <-> e in place, element by element (+ shadow = bf16(new p)): captured HIP
//   graphs and the engine hold the addresses of the flat buffers, only the contents change.
//
// Both are streaming passes (12 B / element for the update, 16-18 B for the swap): 16-B
// loads and stores, kEmaU vectors per thread and trip with every load issued before the first
// store, a grid-stride loop under the flat optimizers' grid cap.  No atomics: deterministic.
#include "common.h"
#include "optim_ops.h"

namespace fdt {

constexpr int kEmaB = 256;     // threads per workgroup
constexpr int kEmaU = 2;       // 16-B vectors per thread and trip (2 x {p, e} loads in flight)
constexpr int kEmaG = 4096;    // grid cap (optim.hip opt_grid)

inline int ema_grid(long n4) {
  long g = (n4 + (long)kEmaB * kEmaU - 1) / ((long)kEmaB * kEmaU);
  if (g > kEmaG) g = kEmaG;
  return g < 1 ? 1 : (int)g;
}

__device__ __forceinline__ float ema_rule(float d, float ev, float pv) {
#pragma clang fp contract(off)
  const float df = ev - pv;
  return fmaf(d, df, pv);
}

__global__ __launch_bounds__(kEmaB) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ e, long n4,
                                                           float decay, int warmup, long k, int* __restrict__ kskip,
                                                           const int* __restrict__ found_inf) {
  if (opt::skip_step(found_inf)) { opt::count_skip(kskip); return; }
  float d = decay;
  if (warmup) {
    const float t = (float)opt::applied_k(k, kskip);
    d = fminf(decay, (1.f + t) / (10.f + t));
  }
  const float4* p4 = reinterpret_cast<const float4*>(p);
  float4* e4 = reinterpret_cast<float4*>(e);
  const long stride = (long)gridDim.x * kEmaB;
  for (long i = (long)blockIdx.x * kEmaB + threadIdx.x; i < n4; i += stride * kEmaU) {
    float4 pv[kEmaU], ev[kEmaU];
#pragma unroll
    for (int u = 0; u < kEmaU; ++u) {
      const long j = i + u * stride;
      if (j < n4) {
        pv[u] = p4[j];
        ev[u] = e4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < kEmaU; ++u) {
      const long j = i + u * stride;
      if (j < n4) {
        float4 r;
        r.x = ema_rule(d, ev[u].x, pv[u].x);
        r.y = ema_rule(d, ev[u].y, pv[u].y);
        r.z = ema_rule(d, ev[u].z, pv[u].z);
        r.w = ema_rule(d, ev[u].w, pv[u].w);
        e4[j] = r;
      }
    }
  }
}

__global__ __launch_bounds__(kEmaB) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ e,
                                                         bf16* __restrict__ shadow, long n4) {
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* e4 = reinterpret_cast<float4*>(e);
  const long stride = (long)gridDim.x * kEmaB;
  for (long i = (long)blockIdx.x * kEmaB + threadIdx.x; i < n4; i += stride * kEmaU) {
    float4 pv[kEmaU], ev[kEmaU];
#pragma unroll
    for (int u = 0; u < kEmaU; ++u) {
      const long j = i + u * stride;
      if (j < n4) {
        pv[u] = p4[j];
        ev[u] = e4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < kEmaU; ++u) {
      const long j = i + u * stride;
      if (j < n4) {
        p4[j] = ev[u];
        e4[j] = pv[u];
        if (shadow) {
          uint2 s;
          s.x = pack_bf16x2(ev[u].x, ev[u].y);
          s.y = pack_bf16x2(ev[u].z, ev[u].w);
          *reinterpret_cast<uint2*>(shadow + j * 4) = s;
        }
      }
    }
  }
}

// {threads per workgroup, vectors per thread and trip, grid cap}: one workgroup's trip covers
// 4 * B * U elements, a full grid's 4 * B * U * G (the tests place their sizes around both)
std::vector<int> ema_launch_config() { return {kEmaB, kEmaU, kEmaG}; }

void ema_update(uint64_t p, uint64_t e, long n, float decay, int warmup, long k, uint64_t kskip, uint64_t found_inf,
                uint64_t stream) {
  FDT_CHECK(n >= 0 && n % 4 == 0, "flat buffer must be padded to a multiple of 4");
  FDT_CHECK(p != 0 && e != 0 && p % 16 == 0 && e % 16 == 0, "ema_update: p / e must be 16-B aligned");
  FDT_CHECK(decay >= 0.f && decay <= 1.f, "ema_update: decay must be in [0, 1]");
  if (n == 0) return;
  ema_update_kernel<<<ema_grid(n / 4), kEmaB, 0, as_stream(stream)>>>(P<const float>(p), P<float>(e), n / 4, decay,
                                                                      warmup, k, P<int>(kskip), P<const int>(found_inf));
  FDT_LAUNCH_CHECK();
}

void ema_swap(uint64_t p, uint64_t e, uint64_t shadow, long n, uint64_t stream) {
  FDT_CHECK(n >= 0 && n % 4 == 0, "flat buffer must be padded to a multiple of 4");
  FDT_CHECK(p != 0 && e != 0 && p != e && p % 16 == 0 && e % 16 == 0 && shadow % 8 == 0,
            "ema_swap: p / e must be distinct and 16-B aligned (shadow 8-B)");
  if (n == 0) return;
  ema_swap_kernel<<<ema_grid(n / 4), kEmaB, 0, as_stream(stream)>>>(P<float>(p), P<float>(e), P<bf16>(shadow), n / 4);
  FDT_LAUNCH_CHECK();
}

}  // namespace fdt
