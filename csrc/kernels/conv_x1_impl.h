// Activation-stationary 1x1 convolution (kg 10): the expanding 1x1 convolutions and the data
// gradients of the reducing ones, where Cout (the GEMM's N) is 2-16 column tiles wide and K is
// short (64-512).  igemm_kernel gives every BM x BN output tile its own workgroup, so the same
// BM x K activation rows are loaded, unpacked, transformed by the prologue, repacked, written
// to LDS and read back as fragments once per column tile.  Here a workgroup owns BM pixels:
//
//   phase 1  the BM x K rows are loaded ONCE and the prologue (none / lazy batch-norm + ReLU /
//            fold) is applied ONCE with store_tile's arithmetic; each 64-wide K tile passes
//            through a swizzled [BM][64] LDS image (igemm_kernel's) and every wave reads its MFMA
//            fragments of it into REGISTERS, where they stay for the workgroup's lifetime
//            (BM/2 x K bf16 per wave: 8 VGPRs per 16-deep K step at BM = 128);
//   phase 2  the workgroup walks its nbn/xn column tiles; each tile's weights [BN][K] stream
//            through a 4-buffer ring of [BN][32] chunks by LDS-DMA (swizzle on the source
//            address, counted vmcnt + raw s_barrier, as igemm_kernel's KG 3 ring).  The ring
//            runs over the flat (tile, chunk) sequence, three chunks ahead, so the first chunks
//            of tile n+1 are requested before the epilogue of tile n -- whose first barrier
//            drains them: the first three chunks of every tile need no wait at all, and in
//            particular none behind the epilogue's output stores.
//
// (The activations resident in LDS instead -- the first form of this kernel -- left room for one
// 4-wave workgroup per CU from K = 128 on, with nothing to overlap its epilogue: measured 14-50 %
// SLOWER than igemm_kernel there, profiles/x4/README.md.  With the fragments in registers the
// LDS footprint is the ring, the epilogue staging and the header: two workgroups per CU at
// every K, and the main loop reads only weight fragments from LDS.)
//
// MFMA fragment mapping, K order (ascending 16-element steps) and the epilogue (conv_epilogue,
// once per column tile with that tile's n0) are igemm_kernel's: for the same (BM, BN) and
// nsplit = 1 the output and the statistics slots are bit-identical to it.  A statistics slot
// still has one writer per (row block, channel).
//
// LDS: [prologue params | per-wave statistics | weight ring | epilogue staging]; phase 1's
// transient activation images use the staging rows (two [BM][64] images fit).
//
// Grid: nbm x xn workgroups; column group g of a row block takes tiles [g nbn/xn, (g+1) nbn/xn).
// xn = 1 is fully stationary; xn > 1 restores parallelism where nbm is small (the 4x4 stage).
// The XCD remap keeps a row block's column groups on one L2.
#pragma once
#include "conv_igemm_impl.h"

namespace fdt {
namespace conv {

constexpr int kX1BKX = 64;  // K width of a phase-1 activation image ([BM][64], 8 chunks per row)
constexpr int kX1BKW = 32;  // K width of a weight ring chunk ([BN][32], 4 chunks per row)
constexpr int kX1NB = 4;    // ring buffers

__host__ __device__ constexpr size_t x1_hdr_bytes(int nprm, int nq, int Cx, int BN) {
  return (((size_t)nprm * Cx + 4 * nq * BN) * 4 + 15) & ~(size_t)15;
}
__host__ __device__ constexpr size_t x1_ring_bytes(int BN) { return (size_t)kX1NB * BN * kX1BKW * 2; }
__host__ __device__ constexpr size_t x1_stage_bytes(int BN) { return (size_t)64 * (BN + 4) * 4; }

// NKT: K / 64 (the K loop is unrolled: the resident fragments are registers)
// PF: the epilogue's operand prefetch depth (conv_epilogue).  Every prefetched load is requested
// and consumed inside the epilogue, after the column tile's last counted wait: the vmcnt counts
// of the weight ring are those of PF = 0.
template <int BM, int BN, int NKT, int PRO, int EPI, int ACT, int PF = 0>
__global__ __launch_bounds__(256, 2) void x1_kernel(const ConvArgs a, const int xn) {
  static_assert(PRO == kProNone || PRO == kProAffineAct || PRO == kProFold, "prologues: none, affine, fold");
  static_assert(ACT == kActNone || ACT == kActRelu, "activations: none, ReLU");
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int NXL = BM / 32;  // activation chunks per thread per image (8 chunks per row)
  constexpr int NWL = BN / 64;  // weight chunks per thread per ring chunk (4 chunks per row)
  constexpr int XT = BM * kX1BKX, WT = BN * kX1BKW;
  constexpr int NKC = NKT * (kX1BKX / kX1BKW);  // ring chunks per column tile
  constexpr bool TWOX = PRO == kProFold;
  constexpr int NPRM = PRO == kProFold ? 3 : (PRO == kProAffineAct ? 2 : 0);
  constexpr int NQ = EPI == kEpiJoinBwd ? 3 : 2;
  static_assert(2 * XT * 2 <= (int)x1_stage_bytes(BN), "two phase-1 images in the staging rows");
  static_assert(NKT * 4 * TM * 4 <= 128, "resident fragments: at most 128 VGPRs");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* pst = reinterpret_cast<float*>(smem);  // [NPRM][Cx]
  float* red = pst + NPRM * a.Cx;               // [4 waves][NQ][BN]
  const size_t hdr = x1_hdr_bytes(NPRM, NQ, a.Cx, BN);
  bf16* ring = reinterpret_cast<bf16*>(smem + hdr);                      // [4][BN][32]
  float* stg = reinterpret_cast<float*>(smem + hdr + x1_ring_bytes(BN));  // [64][BN + 4]
  bf16* ximg = reinterpret_cast<bf16*>(stg);                             // phase 1: [2][BM][64]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid & 1, wm = wid >> 1;
  const int rid = xcd_remap(blockIdx.x, a.nbm * xn);
  const int bm = rid / xn, cgrp = rid - bm * xn;
  const int nct = a.nbn / xn;   // column tiles of this workgroup
  const int col0 = cgrp * nct;  // ... starting at this one
  const long m0 = (long)bm * BM;

  const __amdgpu_buffer_rsrc_t rx_d = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.x, (short)0, (int)(a.Nb_HiWi_Cx_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t ry_d = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(TWOX ? a.x2 : a.x), (short)0, (int)(a.Nb_HiWi_Cx_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw_d = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.w, (short)0, (int)(a.w_bytes), 0x00020000);

  // ---- weight ring.  Chunk image: lane l of a wave instruction writes LDS base + 16 l, so the
  // slot of (row, chunk) is row*4 + chunk = tid + 256 j; the lane filling physical chunk c
  // fetches logical chunk c ^ swz(row) (rows 64 apart share a swizzle).
  const int wave_slot = __builtin_amdgcn_readfirstlane(wid) * 64;
  const int wrow = tid >> 2;
  const uint32_t wsrc = ((uint32_t)wrow * (uint32_t)a.ldw + (uint32_t)(((tid & 3) ^ swz<4>(wrow)) * 8)) * 2u;
  int iti = 0, ikc = 0, ibuf = 0;  // next chunk to request: column tile, chunk, ring buffer
  auto issue = [&]() {
    // (past the last tile the request reads the OOB offset: the vmcnt counts below stay exact)
    const uint32_t tb = ((uint32_t)((col0 + iti) * BN) * (uint32_t)a.ldw + (uint32_t)(ikc * kX1BKW)) * 2u;
    const bool live = iti < nct;
    bf16* Wl = ring + ibuf * WT;
#pragma unroll
    for (int j = 0; j < NWL; ++j) {
      const uint32_t off = live ? tb + wsrc + (uint32_t)(j * 64) * (uint32_t)a.ldw * 2u : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rw_d, (__attribute__((address_space(3))) void*)(Wl + (wave_slot + j * 256) * 8), 16, off, 0, 0, 0);
    }
    ibuf = ibuf == kX1NB - 1 ? 0 : ibuf + 1;
    if (++ikc == NKC) {
      ikc = 0;
      ++iti;
    }
  };
  // the first chunks are requested ahead of phase 1, whose barriers drain them
#pragma unroll
  for (int i = 0; i < kX1NB - 1; ++i) issue();

  // ------------------------------------------------------------------ phase 1: resident X
  const int cc = tid & 7, r0 = tid >> 3;  // this thread's 16-B chunk column and first row of an image
  bool rv[NXL];
  uint32_t xoff[NXL];
#pragma unroll
  for (int j = 0; j < NXL; ++j) {
    const long m = m0 + r0 + j * 32;
    rv[j] = m < a.M;
    xoff[j] = (((uint32_t)m << a.log2Cx) + cc * 8) * 2u;
  }
  struct Stage {
    uint4 rx[NXL], rx2[TWOX ? NXL : 1];
  };
  // (unconditional loads: a row past M reads the OOB offset and returns zeros)
  auto load_x = [&](Stage& S, int kt) {
#pragma unroll
    for (int j = 0; j < NXL; ++j) {
      const uint32_t off = rv[j] ? xoff[j] + (uint32_t)kt * (kX1BKX * 2) : kOOB;
      S.rx[j] = ld_buf16(rx_d, off);
      if constexpr (TWOX) S.rx2[j] = ld_buf16(ry_d, off);
    }
  };
  // store_tile's activation half (conv_igemm_impl.h): the same fma1 / pk_act / pack_bf16x2 and
  // the same zero-select for rows past M
  auto store_x = [&](const Stage& S, int kt) {
    bf16* Xl = ximg + (kt & 1) * XT;
    const int kci = kt * kX1BKX + cc * 8;
    float sv[8], tv[8], gv[8];
    if constexpr (PRO == kProFold) {
      const float4* gp = reinterpret_cast<const float4*>(pst + 2 * a.Cx + kci);
      float4 g0 = gp[0], g1 = gp[1];
      gv[0] = g0.x; gv[1] = g0.y; gv[2] = g0.z; gv[3] = g0.w; gv[4] = g1.x; gv[5] = g1.y; gv[6] = g1.z; gv[7] = g1.w;
    }
    if constexpr (PRO != kProNone) {
      const float4* sp = reinterpret_cast<const float4*>(pst + kci);
      const float4* tp = reinterpret_cast<const float4*>(pst + a.Cx + kci);
      float4 s0 = sp[0], s1 = sp[1], t0 = tp[0], t1 = tp[1];
      sv[0] = s0.x; sv[1] = s0.y; sv[2] = s0.z; sv[3] = s0.w; sv[4] = s1.x; sv[5] = s1.y; sv[6] = s1.z; sv[7] = s1.w;
      tv[0] = t0.x; tv[1] = t0.y; tv[2] = t0.z; tv[3] = t0.w; tv[4] = t1.x; tv[5] = t1.y; tv[6] = t1.z; tv[7] = t1.w;
    }
#pragma unroll
    for (int j = 0; j < NXL; ++j) {
      const int row = r0 + j * 32;
      uint4 o = S.rx[j];
      if constexpr (PRO == kProAffineAct) {
        float v[8];
        const uint32_t u[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[2 * q] = bf16_lo(u[q]); v[2 * q + 1] = bf16_hi(u[q]); }
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = fma1(v[q], sv[q], tv[q]);
        o = make_uint4(pk_act<ACT>(v[0], v[1]), pk_act<ACT>(v[2], v[3]), pk_act<ACT>(v[4], v[5]),
                       pk_act<ACT>(v[6], v[7]));
        if (!rv[j]) o = make_uint4(0, 0, 0, 0);
      } else if constexpr (PRO == kProFold) {
        float g[8], y[8];
        const uint32_t u[4] = {o.x, o.y, o.z, o.w};
        const uint32_t uy[4] = {S.rx2[j].x, S.rx2[j].y, S.rx2[j].z, S.rx2[j].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g[2 * q] = bf16_lo(u[q]); g[2 * q + 1] = bf16_hi(u[q]);
          y[2 * q] = bf16_lo(uy[q]); y[2 * q + 1] = bf16_hi(uy[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = fma1(g[q], gv[q], fma1(tv[q], y[q], sv[q]));
        o = make_uint4(pk_bf16(g[0], g[1]), pk_bf16(g[2], g[3]), pk_bf16(g[4], g[5]), pk_bf16(g[6], g[7]));
        if (!rv[j]) o = make_uint4(0, 0, 0, 0);
      }
      *reinterpret_cast<uint4*>(Xl + row * kX1BKX + 8 * (cc ^ swz<8>(row))) = o;
    }
  };

  bf16x8_t xr[NKT * 4][TM];  // this wave's fragments: [16-deep K step][32-pixel block]
  {
    Stage SA, SB;
    load_x(SA, 0);  // requested before the LDS header set-up and its barrier
    if constexpr (PRO != kProNone) {
      for (int i = tid; i < a.Cx; i += 256) {
        pst[i] = a.ps[i];
        pst[a.Cx + i] = a.pt[i];
        if constexpr (PRO == kProFold) pst[2 * a.Cx + i] = a.pg ? a.pg[i] : 1.f;
      }
      __syncthreads();
    }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      // the next image's rows are requested before this one is transformed; image kt & 1 was
      // last read before the barrier of image kt - 1
      if (kt + 1 < NKT) load_x((kt & 1) ? SA : SB, kt + 1);
      store_x((kt & 1) ? SB : SA, kt);
      __syncthreads();
      const bf16* Xl = ximg + (kt & 1) * XT;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int ch = ks * 2 + (lane >> 5);
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          const int row = wm * (BM / 2) + j * 32 + (lane & 31);
          xr[kt * 4 + ks][j] = *reinterpret_cast<const bf16x8_t*>(Xl + row * kX1BKX + 8 * (ch ^ swz<8>(row)));
        }
      }
    }
  }
  // (the first epilogue's opening barrier orders the last image's reads before its staging writes;
  // every load and ring request so far has been drained by the barriers above)

  // ------------------------------------------------------------------ phase 2: column tiles
  f32x16 acc[TN][TM];
  int cbuf = 0;
  for (int ct = 0; ct < nct; ++ct) {
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      // Chunks 0 .. NB-2 of a tile were requested before the full drain that precedes the tile
      // (phase 1's barriers, the previous epilogue's opening barrier): landed.  A later chunk
      // has landed when all but the NB-2 chunks requested after it have (this wave's requests),
      // then everyone's at the barrier.
      // lgkmcnt(0): this wave's fragment reads of the previous chunk have RETURNED before it
      // lets the others past the barrier -- the request below refills that chunk's buffer, and a
      // weight tile that hits in the vector cache lands within a few hundred cycles, sooner than
      // a read still queued behind the other workgroup's epilogue traffic (the scheduler
      // otherwise leaves the last reads in flight across the s_barrier).
      if (kc >= kX1NB - 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NWL * (kX1NB - 2)) : "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // the buffer requested next held the previous chunk: every wave's reads of it completed
      // before this barrier
      issue();
      const bf16* Wl = ring + cbuf * WT;
#pragma unroll
      for (int ks = 0; ks < kX1BKW / 16; ++ks) {
        const int ch = ks * 2 + (lane >> 5);
        bf16x8_t wf[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          const int row = wn * (BN / 2) + i * 32 + (lane & 31);
          wf[i] = *reinterpret_cast<const bf16x8_t*>(Wl + row * kX1BKW + 8 * (ch ^ swz<4>(row)));
        }
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
          for (int j = 0; j < TM; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], xr[kc * 2 + ks][j], acc[i][j], 0, 0, 0);
      }
      cbuf = cbuf == kX1NB - 1 ? 0 : cbuf + 1;
    }
    conv_epilogue<BM, BN, EPI, ACT, 256, 2, 2, PixLinear, PF>(a, acc, m0, (col0 + ct) * BN, bm, tid, stg, red, true,
                                                              1.f);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the zero chunks past the last tile)
}

template <int BM, int BN, int NKT, int PRO, int EPI, int ACT, int PF = 0>
void x1_launch_one(const ConvArgs& a, int xn, size_t lds, hipStream_t st) {
  auto kern = x1_kernel<BM, BN, NKT, PRO, EPI, ACT, PF>;
  static size_t attr_set = 64 * 1024;  // default dynamic-LDS limit; raise only when needed
  if (lds > attr_set) {
    FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    attr_set = lds;
  }
  hipLaunchKernelGGL(kern, dim3(a.nbm * xn), dim3(256), lds, st, a, xn);
  FDT_LAUNCH_CHECK();
}

// the instantiated (BM, K) pairs: 128 pixels up to K = 256, 64 pixels at K = 512 (the resident
// fragments are 128 VGPRs at both ends)
template <int PRO, int EPI, int ACT>
bool x1_launch_tile(const ConvArgs& a, int BM, int BN, int xn, size_t lds, hipStream_t st) {
  if (BN != 128) return false;
  if constexpr (EPI == kEpiJoinBwd && ACT == kActRelu) {
    // the epilogue's operand prefetch (set_conv_epi_prefetch): a whole pass (4 sweeps).  Not at
    // K = 256: beside the 128 resident-fragment VGPRs even groups of 2 sweeps spill (28 VGPRs)
    // (its descriptors carry the output's byte size, which must stay below the kOOB offset)
    if (conv_epi_prefetch() && a.M * a.Cout * 2 < 0x7FFFFFF0L) {
      if (BM == 128 && a.K == 64) { x1_launch_one<128, 128, 1, PRO, EPI, ACT, 4>(a, xn, lds, st); return true; }
      if (BM == 128 && a.K == 128) { x1_launch_one<128, 128, 2, PRO, EPI, ACT, 4>(a, xn, lds, st); return true; }
      if (BM == 64 && a.K == 512) { x1_launch_one<64, 128, 8, PRO, EPI, ACT, 4>(a, xn, lds, st); return true; }
    }
  }
  if (BM == 128 && a.K == 64) { x1_launch_one<128, 128, 1, PRO, EPI, ACT>(a, xn, lds, st); return true; }
  if (BM == 128 && a.K == 128) { x1_launch_one<128, 128, 2, PRO, EPI, ACT>(a, xn, lds, st); return true; }
  if (BM == 128 && a.K == 256) { x1_launch_one<128, 128, 4, PRO, EPI, ACT>(a, xn, lds, st); return true; }
  if (BM == 64 && a.K == 512) { x1_launch_one<64, 128, 8, PRO, EPI, ACT>(a, xn, lds, st); return true; }
  return false;
}

// (PRO, EPI, ACT) groups, one translation unit each (conv_x1.hip, conv_x1_inst_fold.hip)
bool x1_launch_stats(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int xn, size_t lds, hipStream_t st);
bool x1_launch_fold(int pro, int epi, int act, const ConvArgs& a, int BM, int BN, int xn, size_t lds, hipStream_t st);

}  // namespace conv
}  // namespace fdt
