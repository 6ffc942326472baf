// 3x3 stride-1 convolution with a halo-staged activation operand (MI355X / gfx950).
//
// Why a second main loop: the implicit-GEMM kernel (conv_igemm_impl.h) stages the activation
// operand as im2col rows -- every input pixel is fetched from L2 once per TAP (9x) and every
// 128-pixel workgroup re-reads all 9*Cx*BN weights.  At batch 1024 a 77-GFLOP 3x3 conv then
// pulls ~1.2 GB through L2 -> CU for 128x128 tiles: ~20 B/clk/CU, the rate an L2-served
// gather reaches at one workgroup per CU (MI355X_MICROARCH "Indexed rows: gather into LDS",
// 66-73 GB/s per CU), so the 3x3 layers sat at 21-33 % of their MFMA bound whatever the tile
// (profiles/pmc/r5_bs1024_roofline.md, profiles/r5/ring_probe_bs1024.txt).
//
// Here a workgroup owns BM = 256 CONSECUTIVE NHWC output pixels (whole image rows, or whole
// small images) x BN output channels and walks K in 16-channel chunks.  Per chunk it stages
//   * the zero-padded halo image of its pixels, [halo rows][16 ch] (rows padded to 48 B: 16
//     consecutive rows hit 16 distinct bank quads -> conflict-free ds_read_b128), ONCE for all
//     nine taps: a tap is a constant row offset dh*(W+2) + dw into the halo, so the B fragment
//     of pixel p at tap t is the 16-B row segment q(p) + off(t) -- no im2col address math, no
//     bounds checks in the MFMA loop (the padding is zeros in LDS);
//   * the nine taps' weights [9][BN][16 ch] (16-B halves XOR-swizzled by row bit 3:
//     conflict-free A-fragment reads),
// register-staged one chunk ahead into a double-buffered LDS ring (one barrier per chunk =
// 9 taps x TN x TM MFMAs per wave).  L2 -> CU traffic per 256 pixels drops from ~1.2 MB
// (2 x 128-pixel im2col tiles) to ~0.38 MB (weights once + a ~1.3x halo), and the weight
// bytes per FLOP halve with the 256-pixel tile.
//
// mfma_f32_32x32x16_bf16, weights = A (rows = output channels), halo pixels = B (columns):
// the accumulator layout, and so the fused epilogue (conv_epilogue: BN statistics / the
// producer's activation backward / plain store), are those of the implicit-GEMM kernel.
// Used for the forward 3x3 convolutions on their materialised (normalised + activated)
// inputs and the stride-1 3x3 data gradients on the pre-folded gradient (the taps of a
// stride-1 dgrad are the flipped forward taps, |dh|, |dw| <= 1).
//
// Reference semantics: resnet.py:72-113 (FusedConvBN forward / backward), resnet.py:201-227.
#include "conv_igemm_impl.h"

namespace fdt {
namespace conv {

constexpr int kH3Taps = 9;
constexpr int kH3Row = 16;  // halo row stride in bf16 elements (32 B: the chunk's 16 channels)

// one 16-B-per-lane LDS-DMA piece: lane l fills lds + 16 l (device-only helper)
__device__ __forceinline__ void h3_dma16(__amdgpu_buffer_rsrc_t r, void* lds, uint32_t off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, off, 0, 0, 0);
}

// Halo blocks (one per image, or one per Rb-row slab of a larger image) are laid out every bhr
// rows, bhr = (Rb+2)(W+2) padded so that bhr = 16/NI (mod 16): see H3Geom.
template <int BM>
constexpr int h3_halo_rows_max() {  // BM/16 images of 4x4 -> 36-row (6x6) blocks (BM = 128 / 256:
  return BM / 16 * 36;              // 288 / 576 rows, whole 1-KiB LDS-DMA pieces of 32 rows)
}

// Tile geometry + the MFMA-column -> pixel map of the halo loop.  A ds_read_b128 serves a wave in
// four fixed 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32); a 32-B halo
// row = 2 bank quads whose 16-B halves are XOR-swizzled by row bit 3 (quad of row q, half h:
// 2q + (h ^ q>>3 & 1) mod 16), so 16 CONSECUTIVE halo rows hit 16 distinct quads.  Columns are
// therefore permuted so each lane group reads a 16-pixel set: 16 consecutive pixels of one image
// row (W >= 16), or one row segment of W pixels from each of NI = 16/W images (W = 8, 4) whose
// halo blocks sit bhr rows apart with bhr = 16/NI (mod 16) -- the NI segments then take disjoint
// quad sets.  Conflict-free for every tap (a tap shifts every row alike; checked exhaustively
// for every CIFAR geometry); the identity column order on 48-B rows conflicted 2-3x at W = 16 /
// 8 / 4 (measured 27.5 % bank-conflict cycles, 16x16).
struct H3Geom {
  int W, Rb, W2, bhr, NI, GW, SPR;
  __device__ __forceinline__ H3Geom(int W_, int H_, int BM) {
    W = W_;
    Rb = H_ < BM / W_ ? H_ : BM / W_;
    W2 = W_ + 2;
    GW = W_ < 16 ? W_ : 16;
    NI = 16 / GW;
    SPR = W_ / GW;
    int b = (Rb + 2) * W2;
    if (NI > 1) b += ((16 / NI) - b % 16 + 16) % 16;
    bhr = b;
  }
  // tile-local pixel of MFMA column n of 32-column block blk
  __device__ __forceinline__ int pix(int blk, int n) const {
    const int pn = n < 4 ? n : n < 12 ? n + 12 : n < 16 ? n - 8 : n < 20 ? n + 8 : n < 28 ? n - 12 : n;
    const int s = blk * 2 + (pn >> 4), i = pn & 15;           // 16-pixel set s, position i
    const int per = Rb * SPR;                                   // sets per image group
    const int gi = s / per, rr = s - gi * per, r = rr / SPR, seg = rr - r * SPR;
    const int img = NI * gi + i / GW, col = seg * GW + i % GW;
    return img * (Rb * W) + r * W + col;
  }
  // bf16 element offset of half h of halo row q (the XOR swizzle)
  static __device__ __forceinline__ int elem(int q, int h) { return q * kH3Row + 8 * (h ^ ((q >> 3) & 1)); }
  __device__ __forceinline__ int halo_row(int p) const {
    const int b = p / (Rb * W), r = (p / W) % Rb, c = p % W;
    return b * bhr + (r + 1) * W2 + c + 1;
  }
};

template <int BM, int BN, int WM, int WN, int TP = kH3Taps>
constexpr size_t h3_stage_elems() { return (size_t)TP * BN * 16 + (size_t)h3_halo_rows_max<BM>() * kH3Row; }

// DMA: the chunk's pieces move global -> LDS by LDS-DMA (buffer_load ... lds) issued at the top of
// the previous chunk's MFMAs (no staging registers, no ds_write phase); otherwise register-staged.
// NS: LDS stages.  2 = double-buffered (one workgroup per CU); 1 (LDS-DMA only) = one stage
// (load -> barrier -> MFMAs -> barrier), small enough for TWO workgroups per CU, whose phases
// interleave -- and whose prologues / epilogues overlap the other's main loop.
// TP: taps (9 = a stride-1 3x3; 4 / 2 = an output-parity class of a stride-2 3x3 data gradient,
// whose taps are the class's subset of the flipped 3x3 neighbourhood on the output-gradient grid;
// the epilogue scatters the class grid into the full-resolution gradient, conv_epilogue's OS / oy
// / ox mapping)
template <int BM, int BN, int EPI, int ACT, int WM, int WN, bool DMA, int NS = 2, int TP = kH3Taps>
__global__ __launch_bounds__(64 * WM * WN, (NS == 1 || BN == 64) ? 4 : 1) void h3_kernel(const ConvArgs a) {
  static_assert(NS == 2 || (NS == 1 && DMA), "single-stage: LDS-DMA staging");
  constexpr int NT = 64 * WM * WN;
  constexpr int TN = BN / WN / 32, TM = BM / WM / 32;
  static_assert(TN >= 1 && TM >= 1, "wave tile >= 32x32");
  constexpr int WP = TP * BN * 2;              // weight 16-B pieces per chunk
  constexpr int NWP = (WP + NT - 1) / NT;
  constexpr int HRM = h3_halo_rows_max<BM>();
  constexpr int NHP = (2 * HRM + NT - 1) / NT;  // halo 16-B pieces per thread (upper bound)
  constexpr int NQ = EPI == kEpiJoinBwd ? 3 : 2;
  constexpr int WTILE = TP * BN * 16;           // bf16 elements of the weight tile
  constexpr int STAGE = (int)h3_stage_elems<BM, BN, WM, WN, TP>();

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);              // [NT/64][NQ][BN]
  int* ttab = reinterpret_cast<int*>(red + (NT / 64) * NQ * BN);  // [9]: wt | [9]: tap row offset
  constexpr int HDR = (((NT / 64) * NQ * BN + 2 * kH3Taps) * 4 + 15) & ~15;
  bf16* tiles = reinterpret_cast<bf16*>(smem + HDR);        // [2][STAGE]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid % WN, wm = wid / WN;
  const int rid = xcd_remap(blockIdx.x, a.nbm * a.nbn);
  const int bn = rid % a.nbn, bm = rid / a.nbn;
  const long m0 = (long)bm * BM;
  const int n0 = bn * BN;
  const float inv_alpha = ACT == kActCelu ? 1.f / a.epi_alpha : 1.f;

  // ---- tile geometry: BM consecutive pixels = nbk blocks of Rb whole rows of one image each
  const int W = a.Wi, H = a.Hi, W2 = W + 2, HW = H * W;
  const H3Geom geo(W, H, BM);
  const int Rb = geo.Rb;
  const int nbk = BM / (Rb * W), bhr = geo.bhr, bh0 = (Rb + 2) * W2, HR = nbk * bhr;
  const int img0 = (int)(m0 / HW), h0 = (int)((m0 / W) % H);

  if (tid < TP) {
    ttab[tid] = a.wt[tid];
    ttab[kH3Taps + tid] = a.dh[tid] * W2 + a.dw[tid];
  }
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rx_d = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0,
                                                                        (int)(a.Nb_HiWi_Cx_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw_d = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, (short)0, (int)(a.w_bytes),
                                                                        0x00020000);

  // ---- per-thread staging pieces (fixed across chunks: only the channel offset moves)
  uint32_t woff[NWP], hoff[NHP];
  int wdst[NWP], hdst[NHP];
#pragma unroll
  for (int j = 0; j < NWP; ++j) {
    const int idx = tid + j * NT;
    const bool v = idx < WP;
    const int tap = v ? idx / (2 * BN) : 0;
    const int rem = idx - tap * 2 * BN;
    const int n = rem >> 1, lh = rem & 1;
    woff[j] = v ? ((uint32_t)(n0 + n) * (uint32_t)a.ldw + (uint32_t)(ttab[tap] * a.Cx + 8 * lh)) * 2u : kOOB;
    wdst[j] = v ? (tap * BN + n) * 16 + 8 * (lh ^ ((n >> 3) & 1)) : -1;
  }
#pragma unroll
  for (int j = 0; j < NHP; ++j) {
    const int idx = tid + j * NT;
    const bool v = idx < 2 * HR;
    const int q = idx >> 1, lh = idx & 1;
    const int b = q / bhr, r2 = q - b * bhr;
    const int hr = r2 / W2, hc = r2 - hr * W2;
    const int h = h0 + hr - 1, w = hc - 1;
    const bool in = v && r2 < bh0 && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
    hoff[j] = in ? ((uint32_t)((img0 + b) * HW + h * W + w) * (uint32_t)a.Cx + 8u * lh) * 2u : kOOB;
    hdst[j] = v ? WTILE + H3Geom::elem(q, lh) : -1;  // padding rows store the zeros the OOB load returned
  }
  // ---- per-thread B-fragment halo rows (tap (0, 0)) and the nine tap offsets
  int qb[TM];
#pragma unroll
  for (int j = 0; j < TM; ++j) qb[j] = geo.halo_row(geo.pix(wm * TM + j, lane & 31));
  int toff[TP];
#pragma unroll
  for (int t = 0; t < TP; ++t) toff[t] = ttab[kH3Taps + t];
  const int h = lane >> 5;
  const int ahalf = 8 * (h ^ ((lane >> 3) & 1));  // A-fragment half (the weight tile's swizzle)

  uint4 rw[NWP], rh[NHP];
  auto gload = [&](int ch) {
    const uint32_t cb = (uint32_t)ch * 32u;  // 16 channels * 2 B
#pragma unroll
    for (int j = 0; j < NWP; ++j) rw[j] = ld_buf16(rw_d, woff[j] == kOOB ? kOOB : woff[j] + cb);
#pragma unroll
    for (int j = 0; j < NHP; ++j) rh[j] = ld_buf16(rx_d, hoff[j] == kOOB ? kOOB : hoff[j] + cb);
  };
  auto lstore = [&](int buf) {
    bf16* base = tiles + buf * STAGE;
#pragma unroll
    for (int j = 0; j < NWP; ++j)
      if (wdst[j] >= 0) *reinterpret_cast<uint4*>(base + wdst[j]) = rw[j];
#pragma unroll
    for (int j = 0; j < NHP; ++j)
      if (hdst[j] >= 0) *reinterpret_cast<uint4*>(base + hdst[j]) = rh[j];
  };

  f32x16 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Fragments are double-buffered in registers across taps: tap t+1's LDS reads are issued
  // before tap t's MFMAs and interleaved with them (sched_group_barrier), so each read's latency
  // hides behind MFMAs instead of stalling the wave (the compiler's default order reused one
  // fragment set: 4 reads -> lgkmcnt wait -> 4 MFMAs, the LDS latency exposed every tap).
  auto compute = [&](int buf) {
    const bf16* Wl = tiles + buf * STAGE;
    const bf16* Hl = Wl + WTILE;
    bf16x8_t wf[2][TN], xf[2][TM];
    auto fetch = [&](int t, int sl) {
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int row = wn * (BN / WN) + i * 32 + (lane & 31);
        wf[sl][i] = *reinterpret_cast<const bf16x8_t*>(Wl + (t * BN + row) * 16 + ahalf);
      }
#pragma unroll
      for (int j = 0; j < TM; ++j)
        xf[sl][j] = *reinterpret_cast<const bf16x8_t*>(Hl + H3Geom::elem(qb[j] + toff[t], h));
    };
    fetch(0, 0);
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      const int sl = t & 1;
      if (t + 1 < TP) fetch(t + 1, sl ^ 1);
      __builtin_amdgcn_sched_barrier(0);  // next tap's reads stay ahead of this tap's MFMAs
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[sl][i], xf[sl][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  const int nch = a.Cx >> 4;
  if constexpr (DMA) {
    // LDS image = piece-linear: weight piece (tap*BN + n)*2 + physical half at byte 16*piece;
    // halo piece q*2 + physical half at WTILE*2 + 16*piece (the lane filling physical half ph
    // fetches logical half ph ^ (q>>3 & 1): the swizzle applied on the source side).  A wave
    // instruction fills 64 consecutive pieces (1 KiB at the wave-uniform M0 base); WP is a
    // multiple of 64 (every weight instruction full) and the halo region holds 2*HRM pieces, a
    // multiple of 64, so a partly-valid last halo instruction's extra lanes land inside it
    // (zeros from the OOB offset, rows nobody reads).
    static_assert(WP % 64 == 0 && (2 * HRM) % 64 == 0, "whole 1-KiB DMA pieces");
    constexpr int NWI = WP / 64, NHI = 2 * HRM / 64;  // wave-instructions per chunk
    constexpr int NW = NT / 64;
    const int wv = __builtin_amdgcn_readfirstlane(wid);
    uint32_t wsrc[(NWI + NW - 1) / NW], hsrc[(NHI + NW - 1) / NW];
#pragma unroll
    for (int j = 0; j * NW < NWI; ++j) {
      const int piece = (j * NW + wv) * 64 + lane;
      const bool v = piece < WP;
      const int tap = v ? piece / (2 * BN) : 0;
      const int rem = piece - tap * 2 * BN;
      const int n = rem >> 1, lh = (rem & 1) ^ ((n >> 3) & 1);
      wsrc[j] = v ? ((uint32_t)(n0 + n) * (uint32_t)a.ldw + (uint32_t)(ttab[tap] * a.Cx + 8 * lh)) * 2u : kOOB;
    }
#pragma unroll
    for (int j = 0; j * NW < NHI; ++j) {
      const int piece = (j * NW + wv) * 64 + lane;
      const int q = piece >> 1, part = (piece & 1) ^ ((q >> 3) & 1);  // logical half
      const int b = q / bhr, r2 = q - b * bhr;
      const int hr = r2 / W2, hc = r2 - hr * W2;
      const int hh = h0 + hr - 1, w = hc - 1;
      const bool in = q < HR && r2 < bh0 && (unsigned)hh < (unsigned)H && (unsigned)w < (unsigned)W;
      hsrc[j] = in ? ((uint32_t)((img0 + b) * HW + hh * W + w) * (uint32_t)a.Cx + 8u * part) * 2u : kOOB;
    }
    const int nhi = (2 * HR + 63) / 64;  // halo wave-instructions actually needed (uniform)
    auto issue = [&](int ch, int buf) {
      const uint32_t cb = (uint32_t)ch * 32u;
      char* base = reinterpret_cast<char*>(tiles + buf * STAGE);
#pragma unroll
      for (int j = 0; j * NW < NWI; ++j) {
        const int wi = j * NW + wv;
        if (wi < NWI)
          h3_dma16(rw_d, base + wi * 1024, wsrc[j] == kOOB ? kOOB : wsrc[j] + cb);
      }
#pragma unroll
      for (int j = 0; j * NW < NHI; ++j) {
        const int wi = j * NW + wv;
        if (wi < nhi)
          h3_dma16(rx_d, base + WTILE * 2 + wi * 1024, hsrc[j] == kOOB ? kOOB : hsrc[j] + cb);
      }
    };
    // cost probes (scripts/h3_probe.py; a.dbg, wave-uniform): bit 1 skips the DMA, bit 2 the MFMA
    // phase -- timing only, the output is garbage
    const bool no_dma = a.dbg & 2, no_mma = a.dbg & 4;
    if constexpr (NS == 1) {
      for (int c = 0; c < nch; ++c) {
        if (!no_dma) issue(c, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // chunk c landed for everyone
        if (!no_mma) compute(0);
        __syncthreads();  // everyone's reads of chunk c retired: the stage is free
      }
    } else {
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      // buffer (c+1)&1 was last read in chunk c-1: every wave retired those reads before the
      // barrier that ended it
      if (c + 1 < nch && !no_dma) issue(c + 1, (c + 1) & 1);
      if (!no_mma) compute(c & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMAs of chunk c+1 landed ...
      __syncthreads();                                   // ... and everyone's: read in chunk c+1
    }
    }
  } else {
    gload(0);
    lstore(0);
    if (nch > 1) gload(1);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      compute(c & 1);
      if (c + 1 < nch) {
        lstore((c + 1) & 1);  // buffer (c+1)&1 was last read in chunk c-1, before the previous barrier
        if (c + 2 < nch) gload(c + 2);
      }
      __syncthreads();
    }
  }

  if (a.dbg & 8) return;  // cost probe: no epilogue (every wave returns: no barrier is left waiting)
  struct PixH3 {
    H3Geom g;
    __device__ __forceinline__ int operator()(int wm_, int j, int n) const { return g.pix(wm_ * TM + j, n); }
  };
  conv_epilogue<BM, BN, EPI, ACT, NT, WM, WN, PixH3>(a, acc, m0, n0, bm, tid, reinterpret_cast<float*>(smem + HDR), red,
                                                     true, inv_alpha, PixH3{geo});
}

// host ------------------------------------------------------------------------------------
template <int BM, int BN, int EPI, int ACT, int WM, int WN, bool DMA, int NS, int TP = kH3Taps>
static void h3_launch_one(const ConvArgs& a, hipStream_t st) {
  constexpr int NT = 64 * WM * WN;
  constexpr int NQ = EPI == kEpiJoinBwd ? 3 : 2;
  constexpr size_t hdr = ((((size_t)(NT / 64) * NQ * BN + 2 * kH3Taps) * 4 + 15) & ~(size_t)15);
  const size_t tiles = NS * h3_stage_elems<BM, BN, WM, WN, TP>() * 2, stage = (size_t)WM * 32 * (BN + 4) * 4;
  const size_t lds = hdr + (tiles > stage ? tiles : stage);
  auto kern = h3_kernel<BM, BN, EPI, ACT, WM, WN, DMA, NS, TP>;
  static bool attr = false;
  if (!attr) {
    FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL(kern, dim3(a.nbm * a.nbn), dim3(NT), lds, st, a);
  FDT_LAUNCH_CHECK();
}

// Geometry the halo loop admits (checked on the host before any launch)
bool h3_supported(const ConvArgs& a, int BM) {
  // 9 taps: a stride-1 3x3 (dense output); 2 / 4 taps: a parity class of a stride-2 3x3 data
  // gradient (output scattered to every OS-th pixel of the full-resolution gradient)
  const bool dense = a.OS == 1 && a.oy == 0 && a.ox == 0 && a.Hout == a.Ho && a.Wout == a.Wo;
  const bool cls = (a.ntaps == 2 || a.ntaps == 4) && a.OS == 2 && a.oy >= 0 && a.oy < 2 && a.ox >= 0 && a.ox < 2 &&
                   a.Hout == 2 * a.Ho && a.Wout == 2 * a.Wo;
  if (!((a.ntaps == kH3Taps && dense) || cls) || a.S != 1 || a.Hi != a.Ho || a.Wi != a.Wo || a.nsplit != 1 ||
      (a.Cx & 15) != 0)
    return false;
  for (int t = 0; t < a.ntaps; ++t)
    if (a.dh[t] < -1 || a.dh[t] > 1 || a.dw[t] < -1 || a.dw[t] > 1 || a.wt[t] < 0 || a.wt[t] >= kH3Taps) return false;
  const int W = a.Wi, H = a.Hi;
  if (W < 4 || (W & (W - 1)) != 0 || BM % W != 0 || a.M % BM != 0) return false;
  const int Rb = H < BM / W ? H : BM / W;
  if (Rb < H ? (H % Rb != 0) : (BM % (H * W) != 0)) return false;
  const int nbk = BM / (Rb * W);
  const int GW = W < 16 ? W : 16, NI = 16 / GW;
  int bhr = (Rb + 2) * (W + 2);
  if (NI > 1) bhr += ((16 / NI) - bhr % 16 + 16) % 16;
  // 16-pixel lane-group sets (pixel map, H3Geom): NI images per set need nbk % NI == 0 for W < 16
  if (NI > 1 && (nbk % NI != 0 || Rb != H)) return false;
  if (NI == 1 && (W % 16 != 0)) return false;
  return nbk * bhr <= BM / 16 * 36;
}

bool launch_h3(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int kg, hipStream_t st) {
  if (pro != kProNone) return false;
  FDT_CHECK(h3_supported(a, BM), "halo 3x3 conv: unsupported geometry");
  FDT_CHECK(a.Cout % BN == 0, "halo 3x3 conv: Cout % BN");
  if (a.ntaps != kH3Taps) {
    // stride-2 data-gradient parity classes: the double-buffered LDS-DMA loop (kg 6) only
    FDT_CHECK(kg == 6, "halo 3x3 conv: parity classes run kg 6");
#define FDT_H3C(BM_, BN_, WM_, WN_, TP_)                                                                                 \
    if (BM == BM_ && BN == BN_ && a.ntaps == TP_) {                                                                     \
      if (epi == kEpiActBwd && act == kActRelu) { h3_launch_one<BM_, BN_, kEpiActBwd, kActRelu, WM_, WN_, true, 2, TP_>(a, st); return true; } \
      if (epi == kEpiActBwd && act == kActCelu) { h3_launch_one<BM_, BN_, kEpiActBwd, kActCelu, WM_, WN_, true, 2, TP_>(a, st); return true; } \
      if (epi == kEpiStore && act == kActNone) { h3_launch_one<BM_, BN_, kEpiStore, kActNone, WM_, WN_, true, 2, TP_>(a, st); return true; } \
      return false;                                                                                                     \
    }
    FDT_H3C(256, 128, 4, 2, 4)
    FDT_H3C(256, 128, 4, 2, 2)
    FDT_H3C(256, 64, 8, 1, 4)
    FDT_H3C(256, 64, 8, 1, 2)
#undef FDT_H3C
    return false;
  }
#define FDT_H3E(BM_, BN_, WM_, WN_, D_, NS_)                                                                  \
  if (epi == kEpiStats && act == kActNone) { h3_launch_one<BM_, BN_, kEpiStats, kActNone, WM_, WN_, D_, NS_>(a, st); return true; } \
  if (epi == kEpiActBwd && act == kActRelu) { h3_launch_one<BM_, BN_, kEpiActBwd, kActRelu, WM_, WN_, D_, NS_>(a, st); return true; } \
  if (epi == kEpiActBwd && act == kActCelu) { h3_launch_one<BM_, BN_, kEpiActBwd, kActCelu, WM_, WN_, D_, NS_>(a, st); return true; } \
  if (epi == kEpiStore && act == kActNone) { h3_launch_one<BM_, BN_, kEpiStore, kActNone, WM_, WN_, D_, NS_>(a, st); return true; } \
  if (epi == kEpiNormAct && act == kActNone) { h3_launch_one<BM_, BN_, kEpiNormAct, kActNone, WM_, WN_, D_, NS_>(a, st); return true; } \
  if (epi == kEpiNormAct && act == kActRelu) { h3_launch_one<BM_, BN_, kEpiNormAct, kActRelu, WM_, WN_, D_, NS_>(a, st); return true; } \
  if (epi == kEpiNormAct && act == kActCelu) { h3_launch_one<BM_, BN_, kEpiNormAct, kActCelu, WM_, WN_, D_, NS_>(a, st); return true; }
#define FDT_H3(BM_, BN_, WM_, WN_)                          \
  if (BM == BM_ && BN == BN_) {                             \
    if (kg == 6) { FDT_H3E(BM_, BN_, WM_, WN_, true, 2) }       \
    else if (kg == 7) { FDT_H3E(BM_, BN_, WM_, WN_, true, 1) }  \
    else { FDT_H3E(BM_, BN_, WM_, WN_, false, 2) }             \
    return false;                                           \
  }
  // kg 8: the double-buffered LDS-DMA loop with 16 waves (1024 threads) on the 256 x 128 tile:
  // four waves per SIMD (the MFMA issue rate of the single-stage two-workgroup form) AND the DMA of
  // chunk c+1 under chunk c's MFMAs, in ONE workgroup per CU (the phase-lock of two identical
  // workgroups cannot happen)
  if (kg == 8) {
    if (BM == 256 && BN == 128) { FDT_H3E(256, 128, 8, 2, true, 2) }
    return false;
  }
  FDT_H3(256, 128, 4, 2)
  FDT_H3(256, 64, 8, 1)
  FDT_H3(128, 128, 2, 2)
#undef FDT_H3
#undef FDT_H3E
  return false;
}

}  // namespace conv
}  // namespace fdt

// ---------------------------------------------------------------------------- LDS poison (test aid)
// Fills the whole LDS of every CU with 0xFFFF (a bf16 / fp32 NaN pattern) so a following kernel
// that reads LDS it never wrote shows NaNs instead of the previous kernel's leftovers
// (scripts/h3_repeat.py --poison).  ``flag`` is never set by callers: it only keeps the stores
// observable to the compiler.
namespace fdt {
namespace {
constexpr int kPoisonBytes = 160 * 1024;
__global__ __launch_bounds__(256) void lds_poison_kernel(uint32_t* __restrict__ sink, int flag) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint4* p = reinterpret_cast<uint4*>(lds);
  const uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
  for (int i = threadIdx.x; i < kPoisonBytes / 16; i += 256) p[i] = v;
  __syncthreads();
  if (flag) sink[blockIdx.x * 256 + threadIdx.x] = p[(threadIdx.x * 977) % (kPoisonBytes / 16)].x;
}
}  // namespace

void lds_poison(uint64_t sink, int nblocks, uint64_t stream) {
  static bool attr = false;
  if (!attr) {
    FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lds_poison_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kPoisonBytes));
    attr = true;
  }
  FDT_CHECK(nblocks > 0 && sink != 0, "lds_poison: sink buffer of nblocks * 256 words");
  lds_poison_kernel<<<nblocks, 256, kPoisonBytes, as_stream(stream)>>>(reinterpret_cast<uint32_t*>(sink), 0);
  FDT_HIP_CHECK(hipGetLastError());
}
}  // namespace fdt
