// Dense bf16 GEMM of the transformer's linear layers: forward and data gradient (MI355X / gfx950).
//
//   nt (forward)        y [M][N] = x [M][K]  . W[N][K]^T (+ bias[N])    both operands K-contiguous
//   nn (data gradient)  dx[M][N] = gy[M][K] . W[K][N]                  the reduction runs over W's rows
//
// bf16 operands and output, fp32 accumulation in mfma_f32_32x32x16_bf16, one rounding (RNE) at the
// end.  One kernel template for both kinds; no atomics, bitwise repeatable.
//
// Work split.  A workgroup owns a 128 x 128 output tile: 256 threads, 4 waves of 64 x 64 (2 x 2
// accumulators, 64 accumulator registers), the reduction walked in steps of BK = 64 (16 MFMAs per
// wave and step), __launch_bounds__(256, 2): two workgroups per CU by their 64 KB of LDS, as
// linear_wgrad_kernel<64>.  The weight fragment is the MFMA "A" operand and the token fragment
// the "B" operand, so an accumulator lane holds runs of 4 consecutive output features of ONE
// token (8 B after packing).
//
// Grid.  One-dimensional, XCD-mapped (xcd_remap): tile id = panel * (N / 128) + n-tile, so the
// N / 128 tiles of one 128-token panel run back to back on one XCD, whose L2 serves the panel's rows
// to all of them, and consecutive panels follow on that XCD.  W (at most a few MB) sits in every L2.
//
// Data movement.  Both operand tiles come through buffer descriptors in 16-B pieces, 4 per thread
// and operand; a token row past M lies wholly past the descriptor's range and reads as zeros (the
// operands are contiguous), as in linear_wgrad.hip.  The pieces are register-staged one step ahead
// into a double-buffered LDS ring of [token tile | weight tile] (2 x 2 x 16 KB).  The LDS-DMA
// ring of three stages (buffer_load ... lds) was not built or measured: this is the
// register-staged loop.
//
// LDS images and swizzles (bank = (byte address / 4) % 64, enumerated on the host over all 64
// lanes for every access below; a b128 access is served 16 lanes at a time, a b64 one 32):
//  * token tile (both kinds) and W in nt: [128 rows][64 k], 128-B rows of 8 chunks of 16 B, chunk c
//    of row r stored at c ^ ((r >> 1) & 7).  Two rows fill the 256-B bank image, so the 16 rows a
//    16-lane group reads (ds_read_b128, one chunk each, rows r0 .. r0 + 15) take the 8 XOR values
//    twice, once per row parity: 16 distinct 16-B slots, all 64 banks once.  The staging stores write
//    two rows' 8 chunks per 16 lanes: a permutation of 256 contiguous bytes.
//  * W in nn: [64 k rows][128 n], 256-B rows, chunk c of row r at c ^ 4 * (r & 3), read with the
//    transposing LDS read (ds_read_b64_tr_b16): linear_wgrad.hip's image and reads unchanged --
//    every bank once per 32 lanes, stores one row's 16 chunks per 16 lanes -- no transposed copy
//    of W.
//  * epilogue tile: [128 tokens][128 features] bf16, 256-B rows of 32 slots of 8 B, slot s of row r
//    at s ^ (r & 31).  A lane writes one slot (ds_write_b64); lanes 0-31 hold the same slot of 32
//    consecutive rows: 32 distinct slots, all 64 banks once (lanes 32-63: the slot's partner, the
//    same).  The XOR's low bit swaps the two halves of a 16-B chunk in odd rows; the read side
//    (ds_read_b128, one row's 16 chunks per 16 lanes: 256 contiguous bytes permuted) swaps them back.
//  Every access: no bank conflict.
//
// Epilogue.  bias (bf16, nt only, optional; fetched before the loop) is added in fp32, the sums are
// rounded once with pack_bf16x2 and go through the LDS ring, free after the last step's barrier, so
// the global stores are 16 B per lane and 256 B per row and 16 lanes.  Rows >= M are not stored
// (predicate, and the output descriptor ends at row M).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   nt: 158 VGPRs, 0 AGPRs, 40 SGPRs, no scratch, no spills, 64 KB dynamic LDS, 2 workgroups / CU
//   nn: 162 VGPRs, 0 AGPRs, 36 SGPRs, no scratch, no spills, 64 KB dynamic LDS, 2 workgroups / CU
#include "conv_igemm_impl.h"

namespace fdt {
namespace lgm {
using namespace conv;

typedef short bf16x4w_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4w_t lds_bf16x4w;

constexpr int kT = 128;   // output tile edge (tokens and features)
constexpr int kBK = 64;   // reduction step

struct Args {
  const bf16* a;     // [M][K]
  const bf16* w;     // nt: [N][K], nn: [K][N]
  const bf16* bias;  // [N] or nullptr (nt only)
  bf16* out;         // [M][N]
  int M, N, K, nbn, nblk;
  int a_bytes, w_bytes, o_bytes;
};

// 16-B chunk swizzles (see the file header): 128-B rows of k, 256-B rows of n
__device__ __forceinline__ int swz_k(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swz_n(int row) { return 4 * (row & 3); }

template <bool NN>
__global__ __launch_bounds__(256, 2) void linear_gemm_kernel(const Args a) {
  constexpr int TE = kT * kBK;  // one operand tile, bf16 elements (16 KB)
  constexpr int NP = 4;         // 16-B pieces per thread and operand
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* tiles = reinterpret_cast<bf16*>(smem);  // [2][token tile | weight tile]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int rid = xcd_remap(blockIdx.x, a.nblk);
  const int panel = rid / a.nbn, tn = rid - panel * a.nbn;
  const int m0 = panel * kT, n0 = tn * kT;
  const int nk = a.K / kBK;

  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)a.a, (short)0, a.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, (short)0, a.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, (short)0, a.o_bytes, 0x00020000);

  // per-thread staging pieces: fixed tile-local coordinates, the step moves the base
  uint32_t aoff[NP], woff[NP];
  int adst[NP], wdst[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int i = tid + j * 256;
    {
      const int row = i >> 3, cc = i & 7;
      aoff[j] = ((uint32_t)(m0 + row) * (uint32_t)a.K + (uint32_t)(8 * cc)) * 2u;
      adst[j] = row * kBK + 8 * (cc ^ swz_k(row));
    }
    if constexpr (NN) {
      const int row = i >> 4, cc = i & 15;  // k row, 16-B chunk of the 128 features
      woff[j] = ((uint32_t)row * (uint32_t)a.N + (uint32_t)(n0 + 8 * cc)) * 2u;
      wdst[j] = row * kT + 8 * (cc ^ swz_n(row));
    } else {
      const int row = i >> 3, cc = i & 7;  // feature row, 16-B chunk of the 64 k
      woff[j] = ((uint32_t)(n0 + row) * (uint32_t)a.K + (uint32_t)(8 * cc)) * 2u;
      wdst[j] = row * kBK + 8 * (cc ^ swz_k(row));
    }
  }
  uint4 rav[NP], rwv[NP];
  auto gload = [&](int c) {
    const uint32_t ab = (uint32_t)c * (uint32_t)(kBK * 2);
    const uint32_t wb = NN ? (uint32_t)c * (uint32_t)kBK * (uint32_t)a.N * 2u : ab;
#pragma unroll
    for (int j = 0; j < NP; ++j) rav[j] = ld_buf16(ra, ab + aoff[j]);
#pragma unroll
    for (int j = 0; j < NP; ++j) rwv[j] = ld_buf16(rw, wb + woff[j]);
  };
  auto lstore = [&](int buf) {
    bf16* Al = tiles + buf * 2 * TE;
    bf16* Wl = Al + TE;
#pragma unroll
    for (int j = 0; j < NP; ++j) *reinterpret_cast<uint4*>(Al + adst[j]) = rav[j];
#pragma unroll
    for (int j = 0; j < NP; ++j) *reinterpret_cast<uint4*>(Wl + wdst[j]) = rwv[j];
  };

  // this wave's 64 x 64 quarter; accumulator acc[i][j]: tokens 32 i .. + 31 (columns, lane & 31),
  // features 32 j .. + 31 (rows (r & 3) + 8 (r >> 2) + 4 h)
  const int wm = wid & 1, wn = wid >> 1, h = lane >> 5;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // bias of this lane's features, fetched ahead of the loop: 4 consecutive per (j, q)
  uint2 bv[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bv[j][q] = make_uint2(0u, 0u);
      if (!NN && a.bias != nullptr)
        bv[j][q] = *reinterpret_cast<const uint2*>(a.bias + n0 + wn * 64 + 32 * j + 8 * q + 4 * h);
    }

  // k-contiguous fragments (ds_read_b128): lane l reads row (l & 31) of its 32-row block, the 8 k
  // values 16 ks + 8 h ..; the row's swizzle depends on l alone (the blocks start at multiples of 32)
  const int frow = lane & 31, fsw = swz_k(frow);
  // transposed fragments of W in nn (linear_wgrad.hip): lane (gq, gp) of a 16-lane group supplies k
  // row gq's 4 features 4 gp ..; lane l receives feature l & 31, k rows 8 h .. 8 h + 7 of the step
  const int gq = (lane & 15) >> 2, gp = lane & 3;
  const int wcol = wn * 64 + ((lane >> 4) & 1) * 16 + 4 * gp;

  auto frag_k = [&](const bf16* T, int row, int ks) {
    return *reinterpret_cast<const bf16x8_t*>(T + row * kBK + 8 * ((2 * ks + h) ^ fsw));
  };
  auto frag_t = [&](const bf16* T, int r0, int col) {
    const int r1 = r0 + 4;
    const bf16* p0 = T + r0 * kT + 8 * ((col >> 3) ^ swz_n(r0)) + (col & 7);
    const bf16* p1 = T + r1 * kT + 8 * ((col >> 3) ^ swz_n(r1)) + (col & 7);
    const bf16x4w_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4w*)(p0));
    const bf16x4w_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4w*)(p1));
    return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  auto compute = [&](int buf) {
    const bf16* Al = tiles + buf * 2 * TE;
    const bf16* Wl = Al + TE;
#pragma unroll
    for (int ks = 0; ks < kBK / 16; ++ks) {
      bf16x8_t xf[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[i] = frag_k(Al, wm * 64 + 32 * i + frow, ks);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (NN) wf[j] = frag_t(Wl, ks * 16 + 8 * h + gq, wcol + 32 * j);
        else wf[j] = frag_k(Wl, wn * 64 + 32 * j + frow, ks);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
    }
  };

  gload(0);
  lstore(0);
  if (1 < nk) gload(1);
  __syncthreads();
  for (int c = 0; c < nk; ++c) {
    const int buf = c & 1;
    compute(buf);
    if (c + 1 < nk) {
      lstore(buf ^ 1);  // buffer buf^1 was last read in step c-1, before the previous barrier
      if (c + 2 < nk) gload(c + 2);
    }
    __syncthreads();
  }

  // epilogue (every wave is past its last tile read: the loop ends with a barrier).  The lane's
  // 4-feature runs as 8-B slots of the [128][128] bf16 tile, slot s of row r at s ^ (r & 31).
  uint2* ot = reinterpret_cast<uint2*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wm * 64 + 32 * i + frow;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 b = bv[j][q];
        const int s = 2 * (8 * wn + 4 * j + q) + h;
        uint2 u;
        u.x = pack_bf16x2(acc[i][j][4 * q] + bf16_lo(b.x), acc[i][j][4 * q + 1] + bf16_hi(b.x));
        u.y = pack_bf16x2(acc[i][j][4 * q + 2] + bf16_lo(b.y), acc[i][j][4 * q + 3] + bf16_hi(b.y));
        ot[row * 32 + (s ^ (row & 31))] = u;
      }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = tid + j * 256, row = p >> 4, cc = p & 15;
    const uint4 v = *reinterpret_cast<const uint4*>(ot + row * 32 + 2 * (cc ^ ((row & 31) >> 1)));
    const bool odd = row & 1;  // the slot XOR's low bit: the chunk's halves are exchanged
    const u32x4_t u = {odd ? v.z : v.x, odd ? v.w : v.y, odd ? v.x : v.z, odd ? v.y : v.w};
    if (m0 + row < a.M)
      __builtin_amdgcn_raw_buffer_store_b128(
          u, ro, ((uint32_t)(m0 + row) * (uint32_t)a.N + (uint32_t)(n0 + 8 * cc)) * 2u, 0, 0);
  }
}

}  // namespace lgm

// every byte offset the kernel forms -- up to 127 rows past M of either M-sided array -- stays
// below 2^31
bool linear_gemm_supported(long M, int N, int K) {
  constexpr long lim = 0x7FFFFFF0L;
  return M >= 1 && N >= lgm::kT && K >= lgm::kT && N % lgm::kT == 0 && K % lgm::kT == 0 &&
         (M + lgm::kT) * K * 2 < lim && (M + lgm::kT) * N * 2 < lim && (long)N * K * 2 < lim;
}

void linear_gemm(uint64_t a, uint64_t w, uint64_t bias, uint64_t out, long M, int N, int K, int kind,
                 uint64_t stream) {
  using namespace lgm;
  FDT_CHECK(kind == 0 || kind == 1, "linear_gemm: kind 0 (nt) or 1 (nn)");
  FDT_CHECK(linear_gemm_supported(M, N, K), "linear_gemm: N, K multiples of 128, operands and output below 2 GiB");
  FDT_CHECK(a % 16 == 0 && w % 16 == 0 && out % 16 == 0 && bias % 16 == 0 && a != 0 && w != 0 && out != 0,
            "linear_gemm: 16-B aligned operands, bias and output");
  FDT_CHECK(kind == 0 || bias == 0, "linear_gemm: bias with kind nt only");
  Args g{};
  g.a = P<const bf16>(a);
  g.w = P<const bf16>(w);
  g.bias = P<const bf16>(bias);
  g.out = P<bf16>(out);
  g.M = (int)M; g.N = N; g.K = K;
  g.nbn = N / kT;
  const long grid = ((M + kT - 1) / kT) * g.nbn;
  FDT_CHECK(grid < (1L << 24), "linear_gemm: grid too large");
  g.nblk = (int)grid;
  g.a_bytes = (int)(M * K * 2);
  g.w_bytes = (int)((long)N * K * 2);
  g.o_bytes = (int)(M * N * 2);
  hipStream_t st = as_stream(stream);
  constexpr int lds = 2 * 2 * kT * kBK * 2;  // 64 KB: the ring; the epilogue tile (32 KB) reuses it
#define FDT_LGM(NN_)                                                                                   \
  {                                                                                                    \
    auto k = linear_gemm_kernel<NN_>;                                                                  \
    static bool attr = false;                                                                          \
    if (!attr) {                                                                                       \
      FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k),                              \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds));             \
      attr = true;                                                                                     \
    }                                                                                                  \
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), lds, st, g);                                \
    FDT_LAUNCH_CHECK();                                                                                \
  }
  if (kind == 1) FDT_LGM(true) else FDT_LGM(false)
#undef FDT_LGM
}

}  // namespace fdt
