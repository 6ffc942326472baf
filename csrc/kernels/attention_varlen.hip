// Fused attention over a PACKED stream of variable-length sequences (gfx950 / CDNA4), head_dim
// 64, bf16: the transformer runs on the real tokens only, with no padding rows and no mask.
//
// Inputs: qkv [T][3][H][64] bf16 (the fused Q/K/V projection of the packed stream; the kernels
// take its row stride), cu_seqlens [B+1] int32 ON THE DEVICE (cu[0] = 0, non-decreasing; it is
// never read on the host), max_len = a host-side bound on any sequence length (a bucket value).
// Sequence b owns rows [cu[b], cu[b+1]);  O[r,h] = dropout(softmax(q_r K_b^T / 8)) V_b.
// Rows [cu[B], T) and the rows of a sequence past max_len are SLACK: the kernels write O = 0,
// lse = 0 and dq = dk = dv = 0 there (garbage would be summed into every weight gradient
// downstream).  Whatever cu_seqlens holds, every row index is clamped into [0, T) (seq_of).
// O and dO are [T][H][64] contiguous, the gradient goes straight into one packed [T][3][H][64]
// tensor, lse (log2 domain) and delta = rowsum(dO * O_fp32) are fp32 [H][T] (head-major: the 32
// lanes of a wave touch 32 consecutive floats).  delta uses the forward's unrounded copy of O
// for the reason given in the header of attention.hip.  No atomics: every result is bitwise
// repeatable.
//
// Work split (a design for sequences of 30-60 tokens, where the dense kernel's 128-query
// workgroup sharing one K/V tile is mostly idle): a work item is (sequence, 32-row block, head)
// and is owned by ONE WAVE.  Grid (ceil(max_len/32), ceil(H/4), B + 1), 256 threads; wave w of
// block (x, y, z) takes head 4y + w of sequence z and exits when its head is >= H or 32x >= the
// sequence length -- a zero-length sequence costs one cu read.  Plane z = B zeroes the slack
// rows [cu[B], T); the rows of a sequence past max_len are zeroed by the waves of that sequence.
// The four waves of a workgroup work on different heads and share nothing: each has its own
// [32][72] bf16 row images in LDS, the tile loop has NO __syncthreads(), only the wave's own
// LDS ordering (wave_sync).
//   forward   per 32-key tile: S^T = K Q^T (4 MFMAs, Q fragments in registers for the whole
//             sweep), online softmax with the query on the lane (one lane^32 exchange),
//             O^T += V^T P^T (4 MFMAs, P from the accumulator straight into the B operand, V
//             read transposed from the row image: attention_mma.h ldtr / crow).
//   delta     one thread per (row, head).
//   dK,dV     the wave owns 32 keys (K, V fragments in registers) and sweeps the sequence's
//             queries in 32-row tiles of Q and dO.
//   dQ        the wave owns 32 queries and sweeps 32-key tiles of K and V; P is recomputed
//             from the saved log-sum-exp.
// The last tile of a sequence is partial: absent rows are zero in LDS, absent keys score -inf.
// Dropout: attention.hip's hash (attention_mma.h drop_hash) of lin = (h T + r) max_len + j,
// r = global query row, j = key index within the sequence, uint32 arithmetic that wraps, formed
// with adds from per-lane / per-tile bases; the same keep mask in all three kernels; per-call
// seed XOR the optional device word (seed_ptr), so a graph replay can redraw the masks.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; none uses scratch):
//                        VGPRs  AGPRs  LDS [B]  waves/SIMD
//   fwd       DROP=0       112      0    36864      4
//   fwd       DROP=1       125      0    36864      4
//   delta                  109      0        0      4
//   dkdv      DROP=0       224      0    37888      2
//   dkdv      DROP=1       252      0    37888      2
//   dq        DROP=0       149      0    36864      3
//   dq        DROP=1       157      0    36864      3
// Departure from "8 waves per SIMD on the forward": the wave-private images cost 9 KB per wave,
// 36 KB per workgroup, so the 160 KB of LDS hold 4 workgroups = 4 waves per SIMD whatever the
// registers do, and 8 waves would leave 64 registers where the accumulator, the Q fragments
// and one tile of scores alone are 64.  The forward is held to 4 (amdgpu_waves_per_eu(4));
// for that it stages each tile global -> registers -> LDS inside the trip (with the next tile
// prefetched into 32 more registers it needs 147 / 160 and runs 3 waves, or spills at 4).
// dQ carries dO fragments and a second score tile and spills at 4, so it runs at 3; dK/dV
// keeps 64 accumulator and 32 K/V fragment registers, runs at 2 like the dense kernel, and
// spends its spare registers on prefetching the next Q / dO tile before the current MFMAs.
//
// LDS banks (64 banks x 4 B; the row pitch is 144 B = 36 dwords), computed from the addresses:
//   16-B row stores (stage): lane c writes row c >> 3, chunk c & 7, dword 36 row + 4 chunk.  A
//     b128 access is served 16 lanes at a time = two rows: dwords 36r..36r+31 and
//     36r+36..36r+67, so the last chunk of the second row (dwords 64..67) meets the first
//     chunk of the first row in 4 of the 64 banks: a 2-way conflict on one chunk per pass.  The
//     mapping is kept because it makes every global load a whole 128-B row.
//   ds_read_b128 fragment reads (ld8): lane (l32, h) reads dword 36 l32 + 8 ks + 4h.  The 16
//     rows of one pass start at banks 36 l mod 64 = 0 36 8 44 16 52 24 60 32 4 40 12 48 20 56 28:
//     sixteen distinct multiples of 4, 4 banks each -> all 64 banks, conflict-free.
//   transposed reads (ldtr, ds_read_b64_tr_b16): lane (q, p, g) of a half-wave reads 8 B at
//     dword 36 (R + q) + c0/2 + 8g + 2p.  Per (q, g) the 4 lanes p cover 8 banks starting at
//     (q,g): (0,0) 0, (0,1) 8, (1,0) 36, (1,1) 44, (2,0) 8, (2,1) 16, (3,0) 44, (3,1) 52 --
//     rows q and q + 2 are 72 dwords = 8 banks apart, so banks 8..15 and 44..51 are hit twice:
//     a 2-way conflict in 16 of 64 banks per 32-lane pass (the same as in attention.hip, whose
//     pitch this is; a pitch that frees the transposed reads breaks the b128 fragment reads).
#include "attention_mma.h"

namespace fdt {
namespace attn_varlen {

using namespace attn;  // fragment helpers, kD, kRowLd

constexpr int kT = 32;                 // rows of a wave's tile: queries and keys alike
constexpr int kImg = kT * kRowLd;      // one wave-private row image (bf16 elements)

struct Args {
  const bf16* qkv;   // [T][3][H][64]
  long ld;           // its row stride (elements)
  const int* cu;     // [B + 1]
  const float* o32;  // forward output before rounding [T][H][64]
  const bf16* dout;  // [T][H][64]
  bf16* out;
  float* out32;      // optional unrounded copy of out for the backward's delta; nullptr = not kept
  bf16* dqkv;        // [T][3][H][64]
  long gld;          // its row stride
  float* lse;        // [H][T] log2-domain log-sum-exp
  float* delta;      // [H][T]
  int B, T, H, max_len;
  float c2;          // log2(e) / sqrt(D)
  float scale;       // 1 / sqrt(D)
  uint32_t drop_thr; // drop iff hash < drop_thr (p * 2^32); 0 = no dropout
  float keep_scale;  // 1 / (1 - p)
  uint64_t seed;
  const uint64_t* seed_ptr;  // optional device word XORed into the seed (attention.hip Args)
};

__device__ __forceinline__ bool dropped(const Args& a, uint32_t lin) { return drop_hash(a.seed, lin) < a.drop_thr; }

// Rows of grid plane z, clamped so that nothing leaves [0, T) whatever cu holds: sequence z < B
// computes rows [s0, s0 + len) and zeroes [s0 + len, s1) (its rows past max_len); plane z = B
// has len = 0 and zeroes [cu[B], T).
struct Seq { int s0, len, s1; };
__device__ __forceinline__ Seq seq_of(const Args& a, int z) {
  const int c0 = min(max(a.cu[z], 0), a.T);
  if (z == a.B) return Seq{c0, 0, a.T};
  const int c1 = min(max(a.cu[z + 1], c0), a.T);
  return Seq{c0, min(c1 - c0, a.max_len), c1};
}

// the wave's own LDS ordering: its DS operations execute in issue order, so all that is needed
// is that the compiler keeps the stores of one lane ahead of the loads of another
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One 32 x 64 tile of a [rows][64] matrix with row stride ld: lane c + 64 it holds row c >> 3,
// 16-B chunk c & 7 (a global load instruction reads 8 whole rows); rows at or past n are zero.
struct Tile { uint4 v[4]; };
__device__ __forceinline__ Tile tile_load(const bf16* src, long ld, int r0, int n, int lane) {
  Tile t;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = r0 + 8 * it + (lane >> 3);
    t.v[it] = make_uint4(0, 0, 0, 0);
    if (row < n) t.v[it] = *reinterpret_cast<const uint4*>(src + (long)row * ld + (lane & 7) * 8);
  }
  return t;
}
__device__ __forceinline__ void tile_store(bf16* img, const Tile& t, int lane) {
#pragma unroll
  for (int it = 0; it < 4; ++it)
    *reinterpret_cast<uint4*>(img + (8 * it + (lane >> 3)) * kRowLd + (lane & 7) * 8) = t.v[it];
}

// zero rows [lo, hi) x 64 of head column `col` (element offset) of a bf16 matrix with row stride
// ld: this block takes rows lo + 32 x + l32 in steps of 32 gridDim.x, each half-wave 32 elements
__device__ __forceinline__ void zero_rows(bf16* base, long ld, long col, int lo, int hi, int lane) {
  for (int r = lo + 32 * (int)blockIdx.x + (lane & 31); r < hi; r += 32 * (int)gridDim.x) {
    uint4* p = reinterpret_cast<uint4*>(base + (long)r * ld + col + 32 * (lane >> 5));
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = make_uint4(0, 0, 0, 0);
  }
}

// store the wave's accumulator pair C^T[d][row] (d = 32 dt + crow(r, h), row on the lane) times s
__device__ __forceinline__ void store_rows(bf16* p, const f32x16* acc, float s, int h) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<uint2*>(p + 32 * dt + 8 * g + 4 * h) =
          make_uint2(pack_bf16x2(acc[dt][4 * g] * s, acc[dt][4 * g + 1] * s),
                     pack_bf16x2(acc[dt][4 * g + 2] * s, acc[dt][4 * g + 3] * s));
}

// ------------------------------------------------------------------------------ forward
template <bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void attn_varlen_fwd_kernel(Args a) {
  if (a.seed_ptr != nullptr) a.seed ^= *a.seed_ptr;
  __shared__ __attribute__((aligned(16))) bf16 Ks[4 * kImg];
  __shared__ __attribute__((aligned(16))) bf16 Vs[4 * kImg];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
  const int hd = 4 * blockIdx.y + w;
  if (hd >= a.H) return;
  const Seq sq = seq_of(a, blockIdx.z);
  const long hw = (long)a.H * kD;
  if (sq.s0 + sq.len < sq.s1) {  // slack rows: O = 0, lse = 0
    zero_rows(a.out, hw, (long)hd * kD, sq.s0 + sq.len, sq.s1, lane);
    for (int r = sq.s0 + sq.len + 32 * (int)blockIdx.x + l32; r < sq.s1; r += 32 * (int)gridDim.x) {
      if (a.out32 != nullptr) {
        float4* p = reinterpret_cast<float4*>(a.out32 + (long)r * hw + hd * kD + 32 * h);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (h == 0) a.lse[(long)hd * a.T + r] = 0.f;
    }
  }
  const int q0 = 32 * blockIdx.x, len = sq.len;
  if (q0 >= len) return;
  bf16* Kw = Ks + w * kImg;
  bf16* Vw = Vs + w * kImg;
  const bool qv = q0 + l32 < len;
  const int row = sq.s0 + min(q0 + l32, len - 1);  // absent queries: clamped for the loads, never stored
  const bf16* qp = a.qkv + (long)row * a.ld + hd * kD;
  bf16x8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = ld8(qp + 16 * s + 8 * h);
  const bf16* kp = a.qkv + (long)sq.s0 * a.ld + hw + hd * kD;
  const bf16* vp = kp + hw;
  f32x16 oacc[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const uint32_t qlin = ((uint32_t)hd * (uint32_t)a.T + (uint32_t)row) * (uint32_t)a.max_len;

  for (int k0 = 0; k0 < len; k0 += kT) {
    tile_store(Kw, tile_load(kp, a.ld, k0, len, lane), lane);
    tile_store(Vw, tile_load(vp, a.ld, k0, len, lane), lane);
    wave_sync();
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s = mfma(ld8(Kw + l32 * kRowLd + 16 * ks + 8 * h), qf[ks], s);
    float x[16];
    float mb = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = k0 + crow(r, h) < len ? s[r] * a.c2 : -INFINITY;
      mb = fmaxf(mb, x[r]);
    }
    mb = fmaxf(mb, __shfl_xor(mb, 32));
    const float mn = fmaxf(m, mb);  // finite: key k0 is present in every tile
    const float alpha = fexp2(m - mn);
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = fexp2(x[r] - mn);
      ls += x[r];
    }
    ls += __shfl_xor(ls, 32);
    l = l * alpha + ls;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
    if (DROP) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        x[r] = dropped(a, qlin + (uint32_t)(k0 + crow(r, h))) ? 0.f : x[r] * a.keep_scale;
    }
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      const bf16x8_t pb = pack8(&x[8 * hs]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) oacc[dt] = mfma(ldtr(Vw, 16 * hs, 32 * dt, lane), pb, oacc[dt]);
    }
    wave_sync();
  }

  if (qv) {
    const float inv = 1.f / l;  // l >= 1: the row maximum contributes exp2(0)
    store_rows(a.out + (long)row * hw + hd * kD, oacc, inv, h);
    if (a.out32 != nullptr) {
      float* op32 = a.out32 + (long)row * hw + hd * kD;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(op32 + 32 * dt + 8 * g + 4 * h) =
              make_float4(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv, oacc[dt][4 * g + 2] * inv,
                          oacc[dt][4 * g + 3] * inv);
    }
    if (h == 0) a.lse[(long)hd * a.T + row] = m + log2f(l);
  }
}

// ------------------------------------------------------------------------------ backward
// delta[h][r] = sum_d dO * O, O unrounded (one thread per (r, h) row of 64; slack rows of O are
// zero, and their delta is never read)
__global__ __launch_bounds__(256) void attn_varlen_delta_kernel(Args a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.T * a.H) return;
  const float* o = a.o32 + i * kD;
  const bf16* g = a.dout + i * kD;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float4 o0 = *reinterpret_cast<const float4*>(o + 8 * c);
    const float4 o1 = *reinterpret_cast<const float4*>(o + 8 * c + 4);
    const uint4 ug = *reinterpret_cast<const uint4*>(g + 8 * c);
    acc += o0.x * bf16_lo(ug.x) + o0.y * bf16_hi(ug.x) + o0.z * bf16_lo(ug.y) + o0.w * bf16_hi(ug.y);
    acc += o1.x * bf16_lo(ug.z) + o1.y * bf16_hi(ug.z) + o1.z * bf16_lo(ug.w) + o1.w * bf16_hi(ug.w);
  }
  a.delta[(i % a.H) * a.T + i / a.H] = acc;
}

template <bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn_varlen_dkdv_kernel(Args a) {
  if (a.seed_ptr != nullptr) a.seed ^= *a.seed_ptr;
  __shared__ __attribute__((aligned(16))) bf16 Qs[4 * kImg];
  __shared__ __attribute__((aligned(16))) bf16 Gs[4 * kImg];  // dO rows
  __shared__ __attribute__((aligned(16))) float lse_s[4 * kT];
  __shared__ __attribute__((aligned(16))) float del_s[4 * kT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
  const int hd = 4 * blockIdx.y + w;
  if (hd >= a.H) return;
  const Seq sq = seq_of(a, blockIdx.z);
  const long hw = (long)a.H * kD;
  if (sq.s0 + sq.len < sq.s1) {  // slack rows: dk = dv = 0
    zero_rows(a.dqkv, a.gld, hw + hd * kD, sq.s0 + sq.len, sq.s1, lane);
    zero_rows(a.dqkv, a.gld, 2 * hw + hd * kD, sq.s0 + sq.len, sq.s1, lane);
  }
  const int key0 = 32 * blockIdx.x, len = sq.len;
  if (key0 >= len) return;
  bf16* Qw = Qs + w * kImg;
  bf16* Gw = Gs + w * kImg;
  float* lw = lse_s + w * kT;
  float* dw = del_s + w * kT;
  const int key = key0 + l32;
  const bool kv = key < len;
  const int krow = sq.s0 + min(key, len - 1);
  bf16x8_t kf[4], vf[4];
  {
    const bf16* kp = a.qkv + (long)krow * a.ld + hw + hd * kD;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kf[s] = ld8(kp + 16 * s + 8 * h);
      vf[s] = ld8(kp + hw + 16 * s + 8 * h);
    }
  }
  const float sadd = kv ? 0.f : -INFINITY;  // an absent key: P = 0, so dS = 0
  // dropout index (hd T + r) max_len + key for r = s0 + q0 + 4h + (j & 3) + 8 (j >> 2): per-tile
  // base + lo[j & 3] + hi[j >> 2]
  const uint32_t Mu = (uint32_t)a.max_len;
  const uint32_t lo[4] = {0u, Mu, 2u * Mu, 3u * Mu}, hi[4] = {0u, 8u * Mu, 16u * Mu, 24u * Mu};
  const bf16* qbase = a.qkv + (long)sq.s0 * a.ld + hd * kD;
  const bf16* gbase = a.dout + (long)sq.s0 * hw + hd * kD;
  const float* lbase = a.lse + (long)hd * a.T + sq.s0;
  const float* dbase = a.delta + (long)hd * a.T + sq.s0;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }

  Tile tq = tile_load(qbase, a.ld, 0, len, lane), tg = tile_load(gbase, hw, 0, len, lane);
  for (int q0 = 0; q0 < len; q0 += kT) {
    tile_store(Qw, tq, lane);
    tile_store(Gw, tg, lane);
    if (h == 0) {  // an absent query: lse = +inf makes P = 0
      lw[l32] = q0 + l32 < len ? lbase[q0 + l32] : INFINITY;
      dw[l32] = q0 + l32 < len ? dbase[q0 + l32] : 0.f;
    }
    wave_sync();
    if (q0 + kT < len) {
      tq = tile_load(qbase, a.ld, q0 + kT, len, lane);
      tg = tile_load(gbase, hw, q0 + kT, len, lane);
    }
    f32x16 S, dP;
#pragma unroll
    for (int r = 0; r < 16; ++r) { S[r] = 0.f; dP[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      S = mfma(ld8(Qw + l32 * kRowLd + 16 * ks + 8 * h), kf[ks], S);
      dP = mfma(ld8(Gw + l32 * kRowLd + 16 * ks + 8 * h), vf[ks], dP);
    }
    float p[16], ds[16];
    const uint32_t tlin = ((uint32_t)hd * (uint32_t)a.T + (uint32_t)(sq.s0 + q0 + 4 * h)) * Mu + (uint32_t)key;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {  // rows crow(4 g4 + j, h) = 8 g4 + 4h + j: one float4
      const float4 l4 = *reinterpret_cast<const float4*>(lw + 8 * g4 + 4 * h);
      const float4 d4 = *reinterpret_cast<const float4*>(dw + 8 * g4 + 4 * h);
      const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g4 + j;
        const float pv = fexp2(fmaf(S[r], a.c2, sadd) - lv[j]);
        float z = 1.f;
        if (DROP) z = dropped(a, tlin + lo[j] + hi[g4]) ? 0.f : a.keep_scale;
        p[r] = pv * z;
        ds[r] = pv * (dP[r] * z - dl[j]);
      }
    }
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      const bf16x8_t pb = pack8(&p[8 * hs]);
      const bf16x8_t sb = pack8(&ds[8 * hs]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = mfma(ldtr(Gw, 16 * hs, 32 * dt, lane), pb, dv[dt]);
        dk[dt] = mfma(ldtr(Qw, 16 * hs, 32 * dt, lane), sb, dk[dt]);
      }
    }
    wave_sync();
  }

  if (kv) {
    bf16* gp = a.dqkv + (long)krow * a.gld + hw + hd * kD;
    store_rows(gp, dk, a.scale, h);
    store_rows(gp + hw, dv, 1.f, h);
  }
}

template <bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void attn_varlen_dq_kernel(Args a) {
  if (a.seed_ptr != nullptr) a.seed ^= *a.seed_ptr;
  __shared__ __attribute__((aligned(16))) bf16 Ks[4 * kImg];
  __shared__ __attribute__((aligned(16))) bf16 Vs[4 * kImg];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, l32 = lane & 31;
  const int hd = 4 * blockIdx.y + w;
  if (hd >= a.H) return;
  const Seq sq = seq_of(a, blockIdx.z);
  const long hw = (long)a.H * kD;
  if (sq.s0 + sq.len < sq.s1) zero_rows(a.dqkv, a.gld, (long)hd * kD, sq.s0 + sq.len, sq.s1, lane);
  const int q0 = 32 * blockIdx.x, len = sq.len;
  if (q0 >= len) return;
  bf16* Kw = Ks + w * kImg;
  bf16* Vw = Vs + w * kImg;
  const bool qv = q0 + l32 < len;
  const int row = sq.s0 + min(q0 + l32, len - 1);
  bf16x8_t qf[4], gf[4];
  {
    const bf16* qp = a.qkv + (long)row * a.ld + hd * kD;
    const bf16* gp = a.dout + (long)row * hw + hd * kD;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[s] = ld8(qp + 16 * s + 8 * h);
      gf[s] = ld8(gp + 16 * s + 8 * h);
    }
  }
  const float lse2 = a.lse[(long)hd * a.T + row];
  const float dl = a.delta[(long)hd * a.T + row];
  const uint32_t qlin = ((uint32_t)hd * (uint32_t)a.T + (uint32_t)row) * (uint32_t)a.max_len;
  const bf16* kp = a.qkv + (long)sq.s0 * a.ld + hw + hd * kD;
  const bf16* vp = kp + hw;
  f32x16 dq[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;

  for (int k0 = 0; k0 < len; k0 += kT) {
    tile_store(Kw, tile_load(kp, a.ld, k0, len, lane), lane);
    tile_store(Vw, tile_load(vp, a.ld, k0, len, lane), lane);
    wave_sync();
    f32x16 S, dP;
#pragma unroll
    for (int r = 0; r < 16; ++r) { S[r] = 0.f; dP[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      S = mfma(ld8(Kw + l32 * kRowLd + 16 * ks + 8 * h), qf[ks], S);
      dP = mfma(ld8(Vw + l32 * kRowLd + 16 * ks + 8 * h), gf[ks], dP);
    }
    float ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = k0 + crow(r, h);
      const float pv = fexp2((kr < len ? S[r] * a.c2 : -INFINITY) - lse2);
      float z = 1.f;
      if (DROP) z = dropped(a, qlin + (uint32_t)kr) ? 0.f : a.keep_scale;
      ds[r] = pv * (dP[r] * z - dl);
    }
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      const bf16x8_t sb = pack8(&ds[8 * hs]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) dq[dt] = mfma(ldtr(Kw, 16 * hs, 32 * dt, lane), sb, dq[dt]);
    }
    wave_sync();
  }
  if (qv) store_rows(a.dqkv + (long)row * a.gld + hd * kD, dq, a.scale, h);
}

static Args make_args(uint64_t qkv, long qkv_ld, uint64_t cu, int B, int T, int H, int max_len, float p_drop,
                      uint64_t seed, uint64_t seed_ptr) {
  FDT_CHECK(max_len >= 1 && max_len <= 4096, "varlen attention: max_len in [1, 4096]");
  FDT_CHECK(H >= 1 && T >= 1 && B >= 1, "varlen attention: bad shape");
  FDT_CHECK(qkv_ld >= 3L * H * kD && qkv_ld % 8 == 0, "varlen attention: bad qkv row stride");
  FDT_CHECK(p_drop >= 0.f && p_drop < 1.f, "varlen attention: dropout in [0, 1)");
  FDT_CHECK(cu != 0, "varlen attention: cu_seqlens missing");
  Args a{};
  a.qkv = P<const bf16>(qkv);
  a.ld = qkv_ld;
  a.cu = P<const int>(cu);
  a.B = B; a.T = T; a.H = H; a.max_len = max_len;
  a.scale = 0.125f;  // 1/sqrt(64)
  a.c2 = 1.4426950408889634f * a.scale;
  a.drop_thr = (uint32_t)fminf(p_drop * 4294967296.f, 4294967295.f);
  a.keep_scale = 1.f / (1.f - p_drop);
  a.seed = seed;
  a.seed_ptr = P<const uint64_t>(seed_ptr);
  return a;
}

static dim3 grid_of(const Args& a) { return dim3((a.max_len + kT - 1) / kT, (a.H + 3) / 4, a.B + 1); }

}  // namespace attn_varlen

void attn_varlen_fwd(uint64_t qkv, long qkv_ld, uint64_t cu_seqlens, uint64_t out, uint64_t out32, uint64_t lse,
                     int B, int T, int H, int max_len, float p_drop, uint64_t seed, uint64_t seed_ptr,
                     uint64_t stream) {
  using namespace attn_varlen;
  Args a = make_args(qkv, qkv_ld, cu_seqlens, B, T, H, max_len, p_drop, seed, seed_ptr);
  a.out = P<bf16>(out);
  a.out32 = P<float>(out32);
  a.lse = P<float>(lse);
  if (a.drop_thr) hipLaunchKernelGGL(attn_varlen_fwd_kernel<true>, grid_of(a), dim3(256), 0, as_stream(stream), a);
  else hipLaunchKernelGGL(attn_varlen_fwd_kernel<false>, grid_of(a), dim3(256), 0, as_stream(stream), a);
  FDT_LAUNCH_CHECK();
}

void attn_varlen_bwd(uint64_t qkv, long qkv_ld, uint64_t cu_seqlens, uint64_t o32, uint64_t dout, uint64_t lse,
                     uint64_t delta, uint64_t dqkv, long grad_ld, int B, int T, int H, int max_len, float p_drop,
                     uint64_t seed, uint64_t seed_ptr, uint64_t stream) {
  using namespace attn_varlen;
  Args a = make_args(qkv, qkv_ld, cu_seqlens, B, T, H, max_len, p_drop, seed, seed_ptr);
  FDT_CHECK(grad_ld >= 3L * H * kD && grad_ld % 8 == 0, "varlen attention: bad gradient row stride");
  FDT_CHECK(o32 != 0, "varlen attention: backward needs the forward's fp32 output copy");
  a.gld = grad_ld;
  a.o32 = P<const float>(o32);
  a.dout = P<const bf16>(dout);
  a.lse = P<float>(lse);
  a.delta = P<float>(delta);
  a.dqkv = P<bf16>(dqkv);
  hipStream_t st = as_stream(stream);
  const long rows = (long)T * H;
  hipLaunchKernelGGL(attn_varlen_delta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a);
  FDT_LAUNCH_CHECK();
  if (a.drop_thr) hipLaunchKernelGGL(attn_varlen_dkdv_kernel<true>, grid_of(a), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(attn_varlen_dkdv_kernel<false>, grid_of(a), dim3(256), 0, st, a);
  FDT_LAUNCH_CHECK();
  if (a.drop_thr) hipLaunchKernelGGL(attn_varlen_dq_kernel<true>, grid_of(a), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(attn_varlen_dq_kernel<false>, grid_of(a), dim3(256), 0, st, a);
  FDT_LAUNCH_CHECK();
}

}  // namespace fdt
