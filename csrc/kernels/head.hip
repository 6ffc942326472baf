// Classifier head of the ResNet engine: global average pool + fully connected layer.
//
// The reference ends the network with avg_pool -> view -> fc (models/resnet.py forward,
// reference resnet.py ResNet.forward); run eagerly under autocast that is ~15 small PyTorch
// kernels per step (mean reduction, three bf16 weight/bias/activation casts, a library GEMM,
// and in backward two GEMMs, a bias reduction, the pooling backward broadcast and the fp32
// gradient-accumulation casts) plus the host gaps between them.  Here the head is two
// launches that live INSIDE the body's HIP graphs:
//
//   head_fwd : body [N,HW,C] bf16 -> pooled [N,C] bf16 (kept for the weight gradient) and
//              logits [N,K] bf16 = bf16(pooled) . bf16(W)^T + bf16(b), fp32 accumulation --
//              the autocast numerics of F.linear on a mean-pooled fp32 input.
//   head_bwd : blocks [0, N*cy): dpool[n,c] = bf16(sum_k dl[n,k] bf16(W[k,c])) / HW (the last
//              block's join backward reads it broadcast over HW: no [N,HW,C] gradient is
//              ever written);  blocks [N*cy, ...): W.grad[k,c] += sum_n dl[n,k] pooled[n,c],
//              one owner thread per (k,c) (deterministic, no atomics), and b.grad from
//              the first of them.
//
// K (classes) <= 32 (CIFAR-10): the kernels below, one fp32 accumulator per class in registers.
// 32 < K <= 256 (CIFAR-100, Tiny-ImageNet's 200): the wide head further down -- a pooling pass
// plus MFMA GEMMs under the same contract; it needs C % 32 == 0.  Larger heads (and other
// widths) keep the PyTorch path: nothing above 256 classes is tested, so nothing is accepted.
#include "common.h"

namespace fdt {
namespace {

constexpr int kHB = 256;

__device__ __forceinline__ float bf16r(float x) { return __bfloat162float(__float2bfloat16(x)); }

template <int KT, int S>
__global__ __launch_bounds__(kHB) void head_fwd_kernel(const bf16* __restrict__ h, const float* __restrict__ W,
                                                       const float* __restrict__ b, bf16* __restrict__ pooled,
                                                       bf16* __restrict__ logits, int HW, int C, int K) {
  __shared__ float red[kHB / 64][S * KT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long n0 = (long)blockIdx.x * S;
  const float inv = 1.f / (float)HW;
  float acc[S][KT];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[s][k] = 0.f;

  for (int cg = tid; cg < C / 8; cg += kHB) {
    const int c = cg * 8;
    float p[S][8];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const bf16* src = h + (n0 + s) * (long)HW * C + c;
      float a0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int q = 0;
      // two rows per trip, both loads issued before use
      for (; q + 1 < HW; q += 2) {
        float v0[8], v1[8];
        Vec8<bf16>::load(src + (long)q * C, v0);
        Vec8<bf16>::load(src + (long)(q + 1) * C, v1);
#pragma unroll
        for (int i = 0; i < 8; ++i) { a0[i] += v0[i]; a1[i] += v1[i]; }
      }
      if (q < HW) {
        float v0[8];
        Vec8<bf16>::load(src + (long)q * C, v0);
#pragma unroll
        for (int i = 0; i < 8; ++i) a0[i] += v0[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) p[s][i] = bf16r((a0[i] + a1[i]) * inv);
      Vec8<bf16>::store(pooled + (n0 + s) * C + c, p[s]);
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < K) {
        float w[8];
        Vec8<float>::load(W + (long)k * C + c, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = bf16r(w[i]);
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[s][k] = fmaf(p[s][i], w[i], acc[s][k]);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < K) {
        const float v = wave_sum(acc[s][k]);
        if (lane == 0) red[wv][s * KT + k] = v;
      }
    }
  __syncthreads();
  if (tid < S * K) {
    const int s = tid / K, k = tid % K;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kHB / 64; ++w) v += red[w][s * KT + k];
    v += bf16r(b[k]);
    logits[(n0 + s) * K + k] = __float2bfloat16(v);
  }
}

constexpr int kCPB = 32;          // weight-gradient block: 32 channels ...
constexpr int kNL = kHB / kCPB;   // ... x 8 sample lanes
constexpr int kNChunk = 256;      // samples staged per LDS round

template <int KT>
__global__ __launch_bounds__(kHB) void head_bwd_kernel(const bf16* __restrict__ dl, const float* __restrict__ W,
                                                       const bf16* __restrict__ pooled, bf16* __restrict__ dpool,
                                                       float* __restrict__ gW, float* __restrict__ gb, int N, int C,
                                                       int K, int HW, int cy) {
  const int tid = threadIdx.x;
  const int ndx = N * cy;
  if ((int)blockIdx.x < ndx) {
    // ---- pooled gradient of one sample, 8 channels per thread
    const int n = blockIdx.x / cy;
    const int cg = (blockIdx.x % cy) * kHB + tid;
    if (cg >= C / 8) return;
    const int c = cg * 8;
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
      const float d = __bfloat162float(dl[(long)n * K + k]);
      float w[8];
      Vec8<float>::load(W + (long)k * C + c, w);
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = fmaf(d, bf16r(w[i]), a[i]);
    }
    const float inv = 1.f / (float)HW;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = bf16r(a[i]) * inv;
    Vec8<bf16>::store(dpool + (long)n * C + c, a);
    return;
  }
  // ---- weight / bias gradient of kCPB channels
  __shared__ float sdl[kNChunk][KT];
  __shared__ float red[kNL][kCPB][KT + 1];
  const int j = blockIdx.x - ndx;
  const int cl = tid % kCPB, nl = tid / kCPB;
  const int c = j * kCPB + cl;
  const bool bias_block = (j == 0);
  float a[KT], bs = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) a[k] = 0.f;
  for (int nb = 0; nb < N; nb += kNChunk) {
    const int rows = min(kNChunk, N - nb);
    __syncthreads();
    for (int i = tid; i < rows * K; i += kHB) sdl[i / K][i % K] = __bfloat162float(dl[(long)nb * K + i]);
    __syncthreads();
    if (c < C) {
      int q = nl;
      for (; q + kNL < rows; q += 2 * kNL) {
        const float p0 = __bfloat162float(pooled[(long)(nb + q) * C + c]);
        const float p1 = __bfloat162float(pooled[(long)(nb + q + kNL) * C + c]);
#pragma unroll
        for (int k = 0; k < KT; ++k) a[k] = fmaf(sdl[q + kNL][k], p1, fmaf(sdl[q][k], p0, a[k]));
      }
      if (q < rows) {
        const float p0 = __bfloat162float(pooled[(long)(nb + q) * C + c]);
#pragma unroll
        for (int k = 0; k < KT; ++k) a[k] = fmaf(sdl[q][k], p0, a[k]);
      }
    }
    if (bias_block && tid < K)
      for (int q = 0; q < rows; ++q) bs += sdl[q][tid];
  }
#pragma unroll
  for (int k = 0; k < KT; ++k) red[nl][cl][k] = a[k];
  __syncthreads();
  if (nl == 0 && c < C) {
    for (int k = 0; k < K; ++k) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < kNL; ++q) v += red[q][cl][k];
      gW[(long)k * C + c] += v;
    }
  }
  if (bias_block && tid < K) gb[tid] += bs;
}

// ------------------------------------------------------------------ wide head, 32 < K <= 256
// One accumulator per class in registers does not scale past 32 classes, so the wide head
// pools in a pass of its own (the loop above without the class loop) and runs its three small
// GEMMs on mfma_f32_32x32x16_bf16.  Operand maps of that instruction (lane l: r = l & 31,
// h = l >> 5): A[row r][k = 8h + j] and B[k = 8h + j][col r] in element j of the fragment;
// C[row crow(i, h)][col r] in register i.  Fragments come straight from global memory: every
// product below has at least one operand whose 8 k-elements are contiguous, the strided ones
// are coalesced across the 32 lanes of a half, and the whole head is 0.4 GFLOP at N = 1024.
// Tails: every load is unconditional at a CLAMPED index (in bounds, so the compiler may issue
// the loads of several steps ahead of their MFMAs).  An output row / column past N / K computes
// on the clamped row's data and is never stored (an MFMA output element reads only its own A
// row and B column); an element of the REDUCTION index past its limit is zeroed on both operands.
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWideMaxK = 256;

__device__ __forceinline__ int crow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

__device__ __forceinline__ bf16x8_t frag_of(const float* v) {
  const uint4 u = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                             pack_bf16x2(v[6], v[7]));
  return __builtin_bit_cast(bf16x8_t, u);
}

// elements base[(first + j) * stride], j < 8, of a reduction index with `limit` entries: read at
// min(first + j, limit - 1), zero where first + j >= limit
__device__ __forceinline__ bf16x8_t frag_gather(const bf16* base, int first, int limit, long stride) {
  const unsigned short* q = reinterpret_cast<const unsigned short*>(base);
  bf16x8_t f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const short v = (short)q[min(first + j, limit - 1) * stride];
    f[j] = first + j < limit ? v : (short)0;
  }
  return f;
}

// pooled[n, c] = bf16(mean_hw body[n, :, c]): one workgroup per sample, so the grid does not
// shrink with the class tile; the summation order is that of head_fwd_kernel (even rows into one
// accumulator, odd rows into the other), with four rows' loads in flight per trip.
__global__ __launch_bounds__(kHB) void head_pool_kernel(const bf16* __restrict__ h, bf16* __restrict__ pooled, int HW,
                                                        int C) {
  const long n = blockIdx.x;
  const float inv = 1.f / (float)HW;
  for (int cg = threadIdx.x; cg < C / 8; cg += kHB) {
    const int c = cg * 8;
    const bf16* src = h + n * (long)HW * C + c;
    float a0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int q = 0;
    for (; q + 3 < HW; q += 4) {
      float v0[8], v1[8], v2[8], v3[8];
      Vec8<bf16>::load(src + (long)q * C, v0);
      Vec8<bf16>::load(src + (long)(q + 1) * C, v1);
      Vec8<bf16>::load(src + (long)(q + 2) * C, v2);
      Vec8<bf16>::load(src + (long)(q + 3) * C, v3);
#pragma unroll
      for (int i = 0; i < 8; ++i) { a0[i] = (a0[i] + v0[i]) + v2[i]; a1[i] = (a1[i] + v1[i]) + v3[i]; }
    }
    for (; q + 1 < HW; q += 2) {
      float v0[8], v1[8];
      Vec8<bf16>::load(src + (long)q * C, v0);
      Vec8<bf16>::load(src + (long)(q + 1) * C, v1);
#pragma unroll
      for (int i = 0; i < 8; ++i) { a0[i] += v0[i]; a1[i] += v1[i]; }
    }
    if (q < HW) {
      float v0[8];
      Vec8<bf16>::load(src + (long)q * C, v0);
#pragma unroll
      for (int i = 0; i < 8; ++i) a0[i] += v0[i];
    }
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (a0[i] + a1[i]) * inv;
    Vec8<bf16>::store(pooled + n * C + c, p);
  }
}

// The NW waves' partial 32 x 32 tiles, summed in wave order by the thread that owns the
// element: out(row, col, v) for 16 / NW elements per thread.
template <int NW, typename F>
__device__ __forceinline__ void combine(float (*red)[16][64], const f32x16& acc, F out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wv][i][lane] = acc[i];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16 / NW; ++q) {
    const int e = tid + 64 * NW * q, i = e >> 6, l = e & 63;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][i][l];
    out(crow(i, l >> 5), l & 31, v);
  }
}

// logits tile: 32 samples (blockIdx.x) x 32 classes (blockIdx.y).  A = pooled rows, B = W rows
// (both contiguous in the reduction index c); wave w of the 16 takes the 16-channel steps w,
// w + 16, ..., so the order in which C is summed depends on C alone and a sample's logits neither
// on the other rows of its tile (an MFMA output row reads only its own A row) nor on N.  Sixteen
// waves, each with all its loads issued before its first MFMA at C <= 2048: at batch 128 the grid
// is 16 workgroups and the kernel's time is the length of a wave's load -> MFMA chain.
constexpr int kFW = 16;  // waves of the logits workgroup
__global__ __launch_bounds__(64 * kFW) void head_wide_fwd_kernel(const bf16* __restrict__ pooled,
                                                            const float* __restrict__ W, const float* __restrict__ b,
                                                            bf16* __restrict__ logits, int N, int C, int K) {
  __shared__ float red[kFW][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const bf16* pa = pooled + (long)min(n0 + r, N - 1) * C + 8 * hh;
  const float* pb = W + (long)min(k0 + r, K - 1) * C + 8 * hh;
  f32x16 acc = zero16();
  constexpr int kW = kFW, kU = 8;  // steps a wave has in flight
  const int S = C / 16;
  int s = wv;
  for (; s + (kU - 1) * kW < S; s += kU * kW) {
    bf16x8_t af[kU];
    float w[kU][8];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      af[u] = *reinterpret_cast<const bf16x8_t*>(pa + 16 * (s + u * kW));
      Vec8<float>::load(pb + 16 * (s + u * kW), w[u]);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[u], frag_of(w[u]), acc, 0, 0, 0);
  }
  for (; s < S; s += kW) {
    const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(pa + 16 * s);
    float w[8];
    Vec8<float>::load(pb + 16 * s, w);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, frag_of(w), acc, 0, 0, 0);
  }
  combine<kFW>(red, acc, [&](int row, int col, float v) {
    const int n = n0 + row, k = k0 + col;
    if (n < N && k < K) logits[(long)n * K + k] = __float2bfloat16(v + bf16r(b[k]));
  });
}

// blocks [0, ndx): dpool tile of 32 samples x 128 channels (one 32-channel tile per wave), the
//   whole reduction over the classes in each wave: A = dl rows (classes contiguous, rows of K
//   elements are only 2-byte aligned: element loads), B = W[class][channel] (channel on the lane).
// blocks [ndx, ...): gW tile of 32 classes x 32 channels, the reduction over the samples split
//   over the four waves (16-sample steps w, w + 4, ...) and combined in wave order; the owner
//   thread of an element adds it to the gradient.  A = dl[sample][class], B = pooled[sample]
//   [channel] (class / channel on the lane).  The blocks of channel tile 0 also own gb of their
//   32 classes: 8 sample lanes per class, combined in lane order.
__global__ __launch_bounds__(kHB) void head_wide_bwd_kernel(const bf16* __restrict__ dl, const float* __restrict__ W,
                                                            const bf16* __restrict__ pooled, bf16* __restrict__ dpool,
                                                            float* __restrict__ gW, float* __restrict__ gb, int N,
                                                            int C, int K, int HW, int ndx) {
  __shared__ float red[kHB / 64][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int ct4 = (C + 127) / 128;
  if ((int)blockIdx.x < ndx) {
    const int n0 = (blockIdx.x / ct4) * 32, c0 = ((blockIdx.x % ct4) * 4 + wv) * 32;
    if (c0 >= C) return;  // (no barrier on this branch)
    const bf16* pa = dl + (long)min(n0 + r, N - 1) * K;
    const float* pb = W + c0 + r;
    f32x16 acc = zero16();
    auto wfrag = [&](int kb) {
      float w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = pb[(long)min(kb + j, K - 1) * C];
        w[j] = kb + j < K ? v : 0.f;
      }
      return frag_of(w);
    };
    int kb = 8 * hh;
    for (; kb - 8 * hh + 16 < K; kb += 32) {  // two steps in flight
      const bf16x8_t a0 = frag_gather(pa, kb, K, 1), a1 = frag_gather(pa, kb + 16, K, 1);
      const bf16x8_t b0 = wfrag(kb), b1 = wfrag(kb + 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
    }
    if (kb - 8 * hh < K)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_gather(pa, kb, K, 1), wfrag(kb), acc, 0, 0, 0);
    const float inv = 1.f / (float)HW;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int n = n0 + crow(i, hh);
      if (n < N) dpool[(long)n * C + c0 + r] = __float2bfloat16(bf16r(acc[i]) * inv);
    }
    return;
  }
  const int j = blockIdx.x - ndx, ct = C / 32;
  const int k0 = (j / ct) * 32, c0 = (j % ct) * 32;
  const bf16* pa = dl + min(k0 + r, K - 1);
  const bf16* pb = pooled + c0 + r;
  f32x16 acc = zero16();
  constexpr int kStep = 16 * (kHB / 64);  // samples between two steps of a wave
  int n1 = 16 * wv;                       // first sample of this wave's step
  for (; n1 + kStep < N; n1 += 2 * kStep) {  // two steps in flight
    const int nb = n1 + 8 * hh;
    const bf16x8_t a0 = frag_gather(pa, nb, N, K), a1 = frag_gather(pa, nb + kStep, N, K);
    const bf16x8_t b0 = frag_gather(pb, nb, N, C), b1 = frag_gather(pb, nb + kStep, N, C);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
  }
  if (n1 < N) {
    const int nb = n1 + 8 * hh;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_gather(pa, nb, N, K), frag_gather(pb, nb, N, C), acc, 0, 0, 0);
  }
  combine<kHB / 64>(red, acc, [&](int row, int col, float v) {
    if (k0 + row < K) gW[(long)(k0 + row) * C + c0 + col] += v;
  });
  if (c0 == 0) {
    __shared__ float bred[kHB / 32][32];
    const int kl = tid & 31, nl = tid >> 5, k = k0 + kl;
    float bs = 0.f;
    if (k < K)
      for (int n = nl; n < N; n += kHB / 32) bs += __bfloat162float(dl[(long)n * K + k]);
    bred[nl][kl] = bs;
    __syncthreads();
    if (nl == 0 && k < K) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < kHB / 32; ++q) v += bred[q][kl];
      gb[k] += v;
    }
  }
}

void head_wide_fwd(uint64_t h, uint64_t W, uint64_t b, uint64_t pooled, uint64_t logits, int N, int HW, int C, int K,
                   hipStream_t st) {
  head_pool_kernel<<<N, kHB, 0, st>>>(P<const bf16>(h), P<bf16>(pooled), HW, C);
  head_wide_fwd_kernel<<<dim3((N + 31) / 32, (K + 31) / 32), 64 * kFW, 0, st>>>(
      P<const bf16>(pooled), P<const float>(W), P<const float>(b), P<bf16>(logits), N, C, K);
}

void head_wide_bwd(uint64_t dl, uint64_t W, uint64_t pooled, uint64_t dpool, uint64_t gW, uint64_t gb, int N, int HW,
                   int C, int K, hipStream_t st) {
  const int ndx = ((N + 31) / 32) * ((C + 127) / 128);
  const int nw = ((K + 31) / 32) * (C / 32);
  head_wide_bwd_kernel<<<ndx + nw, kHB, 0, st>>>(P<const bf16>(dl), P<const float>(W), P<const bf16>(pooled),
                                                 P<bf16>(dpool), P<float>(gW), P<float>(gb), N, C, K, HW, ndx);
}

// The cap: 256 classes cover CIFAR-100 and Tiny-ImageNet (200); no test exercises more, so no
// more is accepted.  The wide kernels tile the channels by 32.
bool head_shape_ok(int N, int HW, int C, int K) {
  return K >= 1 && K <= kWideMaxK && N >= 1 && HW >= 1 && C % 8 == 0 && (K <= 32 || C % 32 == 0);
}
#define FDT_HEAD_SHAPE_MSG \
  ": 1 <= classes <= 256, channels a multiple of 8 (above 32 classes: a multiple of 32), samples and HW >= 1"

}  // namespace

void head_fwd(uint64_t h, uint64_t W, uint64_t b, uint64_t pooled, uint64_t logits, int N, int HW, int C, int K,
              uint64_t stream) {
  FDT_CHECK(head_shape_ok(N, HW, C, K), "head_fwd" FDT_HEAD_SHAPE_MSG);
  hipStream_t st = as_stream(stream);
  if (K > 32) {
    head_wide_fwd(h, W, b, pooled, logits, N, HW, C, K, st);
    FDT_LAUNCH_CHECK();
    return;
  }
  const bool wide = N >= 512;
  if (K <= 16) {
    if (wide && N % 4 == 0)
      head_fwd_kernel<16, 4><<<N / 4, kHB, 0, st>>>(P<const bf16>(h), P<const float>(W), P<const float>(b),
                                                    P<bf16>(pooled), P<bf16>(logits), HW, C, K);
    else
      head_fwd_kernel<16, 1><<<N, kHB, 0, st>>>(P<const bf16>(h), P<const float>(W), P<const float>(b),
                                                P<bf16>(pooled), P<bf16>(logits), HW, C, K);
  } else {
    if (wide && N % 2 == 0)
      head_fwd_kernel<32, 2><<<N / 2, kHB, 0, st>>>(P<const bf16>(h), P<const float>(W), P<const float>(b),
                                                    P<bf16>(pooled), P<bf16>(logits), HW, C, K);
    else
      head_fwd_kernel<32, 1><<<N, kHB, 0, st>>>(P<const bf16>(h), P<const float>(W), P<const float>(b),
                                                P<bf16>(pooled), P<bf16>(logits), HW, C, K);
  }
  FDT_LAUNCH_CHECK();
}

void head_bwd(uint64_t dl, uint64_t W, uint64_t pooled, uint64_t dpool, uint64_t gW, uint64_t gb, int N, int HW,
              int C, int K, uint64_t stream) {
  FDT_CHECK(head_shape_ok(N, HW, C, K), "head_bwd" FDT_HEAD_SHAPE_MSG);
  if (K > 32) {
    head_wide_bwd(dl, W, pooled, dpool, gW, gb, N, HW, C, K, as_stream(stream));
    FDT_LAUNCH_CHECK();
    return;
  }
  const int cy = (C / 8 + kHB - 1) / kHB;
  const int nw = (C + kCPB - 1) / kCPB;
  const int grid = N * cy + nw;
  hipStream_t st = as_stream(stream);
  if (K <= 16)
    head_bwd_kernel<16><<<grid, kHB, 0, st>>>(P<const bf16>(dl), P<const float>(W), P<const bf16>(pooled),
                                              P<bf16>(dpool), P<float>(gW), P<float>(gb), N, C, K, HW, cy);
  else
    head_bwd_kernel<32><<<grid, kHB, 0, st>>>(P<const bf16>(dl), P<const float>(W), P<const bf16>(pooled),
                                              P<bf16>(dpool), P<float>(gW), P<float>(gb), N, C, K, HW, cy);
  FDT_LAUNCH_CHECK();
}

}  // namespace fdt
