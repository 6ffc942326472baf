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
// FFN epilogues (template parameter EPI next to NN; launcher linear_gemm_gelu; EPI = none is the
// kernel above, unchanged).  The dropout mask is dropout_math.h keep8 of the flat [M][N] index: with
// N % 128 == 0 the 16-B chunk a store-phase thread holds (8 features of one token, byte offset off) is
// hash chunk off / 16; thr == 0 (p = 0) hashes nothing and keeps everything.
//  * nt + GELU-dropout forward (w_1's GEMM): the bf16 tile goes through LDS as above; in the store
//    phase a thread stores its chunk to a (the value the plain kernel stores) and
//    h = bf16(keep * gelu_erf(float(a)) * scale) of the ROUNDED a to the second output: one keep8 and
//    two 16-B stores per chunk.
//  * nn + GELU-dropout backward with column sums (w_2's data gradient; W_2 read as stored):
//    ga = bf16(keep * scale * gelu_erf_grad(a) * acc) from the fp32 accumulators.
//    - fp32 epilogue tile: [128 tokens][128 features] fp32 = the whole 64 KB ring, free after the
//      loop's last barrier; 512-B rows of 32 slots of 16 B (4 features), slot s of row r at
//      s ^ (r & 15).  A lane writes one slot per accumulator quad (ds_write_b128); the 16 lanes served
//      together hold one slot of 16 consecutive rows: 16 slots distinct mod 16, all 64 banks once.
//      Store phase: thread (rg = tid / 16, cc = tid % 16) owns chunk column cc of rows rg + 16 j,
//      j < 8, and reads its 8 features as slots 2 cc and 2 cc + 1 (two ds_read_b128); chunk columns
//      8-15 read the two in the other order, so the 16 lanes of a row read slots {0, 2, .., 14, 17,
//      .., 31} and then {1, .., 15, 16, .., 30}: distinct mod 16 both times.
//    - a: one 16-B chunk per thread and row (8 buffer loads through a descriptor that ends at row M),
//      issued in step nk - 2 after the last operand tile has been staged, so they are in flight across
//      the last step's MFMAs, the fp32 tile's stores and the barrier.  A row >= M keeps nothing
//      (predicate) and reads a as zeros: it adds exactly 0 to every sum and stores nothing.
//    - column sums (b_1's gradient), no atomics: a thread adds the fp32 ga values (before the bf16
//      rounding) of its 8 rows in j order into 8 partials, writes them to red[rg][128 words] -- word
//      64 half + 4 cc + e holds feature 8 cc + 4 half + e, so 16 lanes write 256 contiguous bytes twice
//      -- and threads 0-127 add the 16 row groups of one word in rg order (ds_read_b32 of 64
//      consecutive words) and store gbslab[panel][n0 + feature].  The caller folds the ceil(M / 128)
//      panel rows in order (linear_bias_fold): bitwise repeatable.
//    Every access of both images, enumerated on the host as above: no bank conflict.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   nt: 158 VGPRs, 0 AGPRs, 40 SGPRs, no scratch, no spills, 64 KB dynamic LDS, 2 workgroups / CU
//   nn: 162 VGPRs, 0 AGPRs, 36 SGPRs, no scratch, no spills, 64 KB dynamic LDS, 2 workgroups / CU
//   nt + GELU forward:  158 VGPRs, 0 AGPRs, 47 SGPRs, no scratch, no spills, 64 KB, 2 workgroups / CU
//   nn + GELU backward: 198 VGPRs, 0 AGPRs, 49 SGPRs, no scratch, no spills, 64 KB, 2 workgroups / CU
//                       (2 waves per SIMD by registers: still one wave per SIMD and workgroup)
#include "conv_igemm_impl.h"
#include "dropout_math.h"

#include <algorithm>

namespace fdt {
namespace lgm {
using namespace conv;

typedef short bf16x4w_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4w_t lds_bf16x4w;

constexpr int kT = 128;   // output tile edge (tokens and features)
constexpr int kBK = 64;   // reduction step

// FFN epilogues (see the file header): none | nt + GELU-dropout forward | nn + GELU-dropout backward
enum Epi : int { kEpiNone = 0, kEpiGeluFwd = 1, kEpiGeluBwd = 2 };

struct Args {
  const bf16* a;     // [M][K]
  const bf16* w;     // nt: [N][K], nn: [K][N]
  const bf16* bias;  // [N] or nullptr (nt only)
  bf16* out;         // [M][N]; GeluFwd: h, GeluBwd: ga
  int M, N, K, nbn, nblk;
  int a_bytes, w_bytes, o_bytes;
  // the FFN epilogues only
  bf16* act;         // [M][N] (o_bytes): GeluFwd writes a = acc + bias, GeluBwd reads it
  float* gbslab;     // GeluBwd: [ceil(M / 128)][N] column sums of ga, one row per panel
  uint32_t thr;      // dropout threshold (0: keep everything)
  float scale;       // 1 / (1 - p)
  uint64_t seed;
  const uint64_t* seed_ptr;
};

// 16-B chunk swizzles (see the file header): 128-B rows of k, 256-B rows of n
__device__ __forceinline__ int swz_k(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swz_n(int row) { return 4 * (row & 3); }

template <bool NN, int EPI = kEpiNone>
__global__ __launch_bounds__(256, 2) void linear_gemm_kernel(const Args a) {
  static_assert(EPI == kEpiNone || NN == (EPI == kEpiGeluBwd), "GELU forward rides nt, GELU backward nn");
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
  // FFN epilogues: the live dropout seed, and the descriptor of a [M][N] (ends at row M, like ro)
  [[maybe_unused]] uint64_t dseed = 0;
  [[maybe_unused]] __amdgpu_buffer_rsrc_t rx = ro;
  [[maybe_unused]] uint4 av[8];  // GeluBwd: this thread's 8 chunks of a (rows (tid >> 4) + 16 j, chunk tid & 15)
  if constexpr (EPI != kEpiNone) {
    dseed = drop::live_seed(a.seed, a.seed_ptr);
    rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.act, (short)0, a.o_bytes, 0x00020000);
  }
  if constexpr (EPI == kEpiGeluBwd) {
#pragma unroll
    for (int j = 0; j < 8; ++j) av[j] = make_uint4(0u, 0u, 0u, 0u);
  }
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
    if constexpr (EPI == kEpiGeluBwd) {
      // a's chunks, requested once the last operand tile has been staged (nk >= 2): in flight across
      // the last step, the fp32 tile's way into LDS and its barrier.  Rows >= M lie past rx: zeros.
      if (c == nk - 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          av[j] = ld_buf16(rx, ((uint32_t)(m0 + (tid >> 4) + 16 * j) * (uint32_t)a.N + (uint32_t)(n0 + 8 * (tid & 15))) * 2u);
      }
    }
    __syncthreads();
  }

  if constexpr (EPI == kEpiGeluBwd) {
    // ga = keep * scale * gelu'(a) * acc from the fp32 accumulators.  The tile as [128 tokens][128
    // features] fp32: 512-B rows of 32 slots of 16 B (4 features), slot s of row r at s ^ (r & 15); it
    // fills the ring.  A lane writes one slot per (i, j, q); 16 lanes hold 16 consecutive rows.
    float4* ft = reinterpret_cast<float4*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = wm * 64 + 32 * i + frow;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int s = 2 * (8 * wn + 4 * j + q) + h;
          ft[row * 32 + (s ^ (row & 15))] =
              make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
        }
    }
    __syncthreads();
    // store phase: thread (rg, cc) owns chunk column cc (8 features) of rows rg + 16 j.  The chunk is
    // slots 2 cc and 2 cc + 1; chunk columns 8-15 read them in the other order, so the 16 lanes of a
    // row touch 16 slots that differ mod 16 in each of the two reads.
    const int rg = tid >> 4, cc = tid & 15, sw = cc >> 3;
    float cs[8];  // column partials of the fp32 ga values, rows in j order
#pragma unroll
    for (int k = 0; k < 8; ++k) cs[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = rg + 16 * j;
      const float4 v0 = ft[row * 32 + ((2 * cc + sw) ^ (row & 15))];
      const float4 v1 = ft[row * 32 + ((2 * cc + (sw ^ 1)) ^ (row & 15))];
      const float4 lo = sw ? v1 : v0, hi = sw ? v0 : v1;
      const float g[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      const bool ok = m0 + row < a.M;
      const uint32_t off = ((uint32_t)(m0 + row) * (uint32_t)a.N + (uint32_t)(n0 + 8 * cc)) * 2u;
      // a row past M keeps nothing: it adds exactly 0 to the sums, whatever the accumulators hold
      const uint32_t mk = !ok ? 0u : a.thr ? drop::keep8((long)(off >> 4), dseed, a.thr) : 0xffu;
      const uint32_t aw[4] = {av[j].x, av[j].y, av[j].z, av[j].w};
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float ak = (k & 1) ? bf16_hi(aw[k >> 1]) : bf16_lo(aw[k >> 1]);
        f[k] = ((mk >> k) & 1u) ? g[k] * a.scale * drop::gelu_erf_grad(ak) : 0.f;
        cs[k] += f[k];
      }
      const u32x4_t u = {pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                         pack_bf16x2(f[6], f[7])};
      if (ok) __builtin_amdgcn_raw_buffer_store_b128(u, ro, off, 0, 0);
    }
    __syncthreads();  // every thread is past its tile reads
    // fold of the 16 row groups: red[rg][128 words], word 64 half + 4 cc + e = feature 8 cc + 4 half + e,
    // so 16 lanes write 256 contiguous bytes twice and the 128 adders read consecutive words
    float4* red4 = reinterpret_cast<float4*>(smem);
    red4[rg * 32 + cc] = make_float4(cs[0], cs[1], cs[2], cs[3]);
    red4[rg * 32 + 16 + cc] = make_float4(cs[4], cs[5], cs[6], cs[7]);
    __syncthreads();
    if (tid < kT) {
      const float* red = reinterpret_cast<const float*>(smem);
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += red[r * kT + tid];  // row groups in order: repeatable
      const int col = 8 * ((tid >> 2) & 15) + 4 * (tid >> 6) + (tid & 3);
      a.gbslab[panel * a.N + n0 + col] = t;
    }
    return;
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
    const uint32_t off = ((uint32_t)(m0 + row) * (uint32_t)a.N + (uint32_t)(n0 + 8 * cc)) * 2u;
    if constexpr (EPI == kEpiGeluFwd) {
      // the chunk is chunk off / 16 of the dropout hash; h from the rounded a, as the backward and the
      // standalone pass see it
      if (m0 + row < a.M) {
        __builtin_amdgcn_raw_buffer_store_b128(u, rx, off, 0, 0);
        const uint32_t mk = a.thr ? drop::keep8((long)(off >> 4), dseed, a.thr) : 0xffu;
        float f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float ak = (k & 1) ? bf16_hi(u[k >> 1]) : bf16_lo(u[k >> 1]);
          f[k] = ((mk >> k) & 1u) ? drop::gelu_erf(ak) * a.scale : 0.f;
        }
        const u32x4_t hv = {pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                            pack_bf16x2(f[6], f[7])};
        __builtin_amdgcn_raw_buffer_store_b128(hv, ro, off, 0, 0);
      }
    } else {
      if (m0 + row < a.M) __builtin_amdgcn_raw_buffer_store_b128(u, ro, off, 0, 0);
    }
  }
}

// shape fields of g and the launch of one instantiation
template <bool NN, int EPI>
void launch(Args g, long M, int N, int K, hipStream_t st) {
  g.M = (int)M; g.N = N; g.K = K;
  g.nbn = N / kT;
  const long grid = ((M + kT - 1) / kT) * g.nbn;
  FDT_CHECK(grid < (1L << 24), "linear_gemm: grid too large");
  g.nblk = (int)grid;
  g.a_bytes = (int)(M * K * 2);
  g.w_bytes = (int)((long)N * K * 2);
  g.o_bytes = (int)(M * N * 2);
  // 64 KB: the ring; the bf16 epilogue tile (32 KB) and the fp32 one of GeluBwd (64 KB) reuse it
  constexpr int lds = 2 * 2 * kT * kBK * 2;
  auto k = linear_gemm_kernel<NN, EPI>;
  static bool attr = false;
  if (!attr) {
    FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr = true;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), lds, st, g);
  FDT_LAUNCH_CHECK();
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
  if (kind == 1) launch<true, lgm::kEpiNone>(g, M, N, K, as_stream(stream));
  else launch<false, lgm::kEpiNone>(g, M, N, K, as_stream(stream));
}

void linear_gemm_gelu(uint64_t a, uint64_t w, uint64_t bias, uint64_t act, uint64_t out, uint64_t gbslab, long M,
                      int N, int K, int kind, float p, uint64_t seed, uint64_t seed_ptr, uint64_t stream) {
  using namespace lgm;
  FDT_CHECK(kind == 0 || kind == 1, "linear_gemm_gelu: kind 0 (nt, GELU-dropout forward) or 1 (nn, backward)");
  FDT_CHECK(linear_gemm_supported(M, N, K),
            "linear_gemm_gelu: N, K multiples of 128, operands and output below 2 GiB");
  FDT_CHECK(a % 16 == 0 && w % 16 == 0 && out % 16 == 0 && bias % 16 == 0 && a != 0 && w != 0 && out != 0,
            "linear_gemm_gelu: 16-B aligned operands, bias and output");
  FDT_CHECK(act % 16 == 0 && act != 0 && gbslab % 16 == 0, "linear_gemm_gelu: 16-B aligned a and column-sum slab");
  FDT_CHECK(kind == 0 ? (bias != 0 && gbslab == 0) : (bias == 0 && gbslab != 0),
            "linear_gemm_gelu: nt takes the (bf16) bias, nn the column-sum slab");
  FDT_CHECK(p >= 0.f && p < 1.f, "linear_gemm_gelu: dropout p in [0, 1)");
  Args g{};
  g.a = P<const bf16>(a);
  g.w = P<const bf16>(w);
  g.bias = P<const bf16>(bias);
  g.out = P<bf16>(out);
  g.act = P<bf16>(act);
  g.gbslab = P<float>(gbslab);
  g.thr = (uint32_t)std::min((double)p * 4294967296.0, 4294967295.0);
  g.scale = 1.f / (1.f - p);
  g.seed = seed;
  g.seed_ptr = P<const uint64_t>(seed_ptr);
  if (kind == 1) launch<true, lgm::kEpiGeluBwd>(g, M, N, K, as_stream(stream));
  else launch<false, lgm::kEpiGeluFwd>(g, M, N, K, as_stream(stream));
}

}  // namespace fdt

