// Fused backward of the expanding 1x1 convolutions (Cin -> 4 Cin, stride 1, no padding): the
// data gradient and the weight gradient in ONE pass over g, y and x.
//
//   G~ = g*gs + alpha + beta*y          (BN-backward fold, rounded to bf16 as store_tile /
//                                        wgrad_kernel round it; gs = nullptr means 1)
//   dX[px][ci]  = G~[px][:] . Wd[ci][:]                   -> EPI_ACTBWD or EPI_STORE epilogue
//   dW[co][ci] += sum_px G~[px][co] * A[px][ci],  A = relu(x*xs + xt)  (ACTBWD) or x (STORE)
//
// The two-launch path (igemm_kernel + wgrad_kernel) streams g and y -- the largest operands of
// the step, M x 4 Cin each -- twice and folds them twice.  Here a persistent workgroup (one per
// CU, 8 waves) owns a contiguous range of 128-pixel chunks and keeps the whole dW in registers
// (32 per lane) and its statistics sums in LDS across them, flushed once at the end.
//
// Per chunk: g and y pass through the fold into a swizzled [128 px][64 co] LDS image, one 64-
// channel K tile at a time (double-buffered).  ONE image serves both products: the data gradient
// reads it row-wise (ds_read_b128, pixels = MFMA columns, as igemm_kernel), the weight gradient
// column-wise (ds_read_b64_tr_b16, as wgrad_kernel).  The chunk swizzle
//     chunk ^ (bit1(row) << 2 | bits 3:2 (row))
// is conflict-free for both: a b128 lane group (16 rows) meets 8 distinct values x 2 row
// parities = the 16 slots of a bank row, and the four rows of a transposed 32-lane read take
// both 64-B halves of both parities.  x is loaded once per chunk: its transformed form is the
// weight gradient's other operand (LDS image, same swizzle), its raw form waits in a per-thread
// LDS slot for the ACTBWD epilogue.  Wd (32 KB) is staged once per workgroup.
//
// Latency hiding: the register stages hold the four K tiles of the NEXT chunk (64 KB of g + y
// per CU in flight, reloaded as each tile is consumed) plus the next chunk's x.  246 VGPRs, no
// scratch, 154 KB of LDS: one workgroup per CU, two waves per SIMD (profiles/x6/README.md).
//
// Rows past M (partial last chunk) load as zeros, which the fold would turn into alpha: both
// images zero those rows, the epilogue skips them.  A workgroup without chunks is not launched.
//
// Flush: fp32 atomics into the OIHW gradient and one statistics slot row per workgroup; in
// deterministic mode a per-workgroup slab summed by wgrad_reduce and slot = workgroup index.
#include "conv_igemm_impl.h"

namespace fdt {

void wgrad_reduce(uint64_t slab, uint64_t out, int nsplit, int Cout, int Cin, int ntaps, int Cxp, int accumulate,
                  uint64_t stream);

namespace bp {

using namespace conv;

typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4_t lds_bf16x4;

constexpr int kPX = 128;  // pixels per chunk
constexpr int kNT = 512;  // threads
constexpr int kKT = 64;   // channels of g / y per K tile

struct PairArgs {
  const bf16 *g, *y;   // [M][CO]
  const bf16* wd;      // [CI][CO] packed data-gradient weights
  const bf16* x;       // [M][CI] conv input (raw)
  const float *al, *be, *gs;  // fold [CO] (gs may be nullptr)
  const float *xs, *xt;       // ACTBWD: input transform of the weight gradient [CI]
  const float *es, *et;       // ACTBWD: producer scale / shift of the epilogue [CI]
  bf16* dx;            // [M][CI]
  float* part;         // ACTBWD: statistics slots [rows][2][CI]
  float* dw;           // fp32 [CO][CI] gradient (atomics) or the slab [wgs][CO][CI] (deterministic)
  long M;
  int nchunks, cpw;    // 128-pixel chunks; chunks per workgroup
  unsigned slot_mask;
  int det, wthru;
  long g_bytes, x_bytes;
};

__host__ __device__ constexpr size_t pair_lds_bytes(int CI) {
  const int CO = 4 * CI;
  return (size_t)CI * CO * 2 + 2 * kPX * kKT * 2 + 2 * kPX * CI * 2 + (size_t)kPX * (CI + 4) * 4 +
         (size_t)(3 * CO + 4 * CI) * 4 + (size_t)(kNT / 64) * 2 * CI * 4 + (size_t)2 * kNT * 16;
}

// chunk swizzle of a [rows][64 x bf16] image read by ds_read_b128 and ds_read_b64_tr_b16
__device__ __forceinline__ int gswz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

template <int CI, bool ACTBWD>
__global__ __launch_bounds__(kNT, 1) void bwd_pair_kernel(const PairArgs a) {
  static_assert(CI == 64, "instantiated for 64 -> 256");
  constexpr int CO = 4 * CI, NKT = CO / kKT;
  constexpr int SW = CI + 4;  // staged fp32 row stride (conv_epilogue's padding)
  constexpr int WCH = CO / 8;  // 16-B chunks per Wd row

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* Wl = reinterpret_cast<bf16*>(smem);        // [CI][CO]
  bf16* Gl = Wl + CI * CO;                         // [2][128][64]
  bf16* Al = Gl + 2 * kPX * kKT;                   // [2][128][CI]
  float* stg = reinterpret_cast<float*>(Al + 2 * kPX * CI);  // [128][SW]
  float* prm = stg + kPX * SW;                     // al | be | gs [CO], xs | xt | es | et [CI]
  float* red = prm + 3 * CO + 4 * CI;              // [8 waves][2][CI]
  uint4* xraw = reinterpret_cast<uint4*>(red + (kNT / 64) * 2 * CI);  // [2][512]: each thread's raw x rows

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int c_begin = blockIdx.x * a.cpw;
  int c_end = c_begin + a.cpw;
  if (c_end > a.nchunks) c_end = a.nchunks;
  if (c_begin >= c_end) return;  // (the launcher starts no such workgroup)

  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)a.g, (short)0, (int)a.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, (short)0, (int)a.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.dx, (short)0, (int)a.x_bytes, 0x00020000);

  // staging map (loads, image stores and the epilogue's row pass): 16-B chunk cc of rows
  // r0 and r0 + 64
  const int cc = tid & 7, r0 = tid >> 3;

  struct Stage {
    uint4 g[2], y[2];
  };
  // (unconditional loads: a row past M or a chunk past this workgroup's range reads the OOB
  // offset and returns zeros, so the compiler counts the loads in flight exactly)
  auto load_tile = [&](Stage& S, int c, int kt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long p = (long)c * kPX + r0 + 64 * j;
      const bool ok = (c < c_end) & (p < a.M);
      const uint32_t off = ok ? ((uint32_t)p * (uint32_t)CO + (uint32_t)(kt * kKT + cc * 8)) * 2u : kOOB;
      S.g[j] = ld_buf16(rg, off);
      S.y[j] = ld_buf16(ry, off);
    }
  };
  auto load_x = [&](uint4 (&X)[2], int c) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long p = (long)c * kPX + r0 + 64 * j;
      const bool ok = (c < c_end) & (p < a.M);
      X[j] = ld_buf16(rx, ok ? ((uint32_t)p * (uint32_t)CI + (uint32_t)(cc * 8)) * 2u : kOOB);
    }
  };
  // fold -> Gl[buf]; store_tile's arithmetic and rounding
  auto store_g = [&](const Stage& S, int c, int kt, int buf) {
    bf16* G = Gl + buf * (kPX * kKT);
    const float4* ap = reinterpret_cast<const float4*>(prm + kt * kKT + cc * 8);
    const float4* bp_ = reinterpret_cast<const float4*>(prm + CO + kt * kKT + cc * 8);
    const float4* gp = reinterpret_cast<const float4*>(prm + 2 * CO + kt * kKT + cc * 8);
    const float4 a0 = ap[0], a1 = ap[1], b0 = bp_[0], b1 = bp_[1], g0 = gp[0], g1 = gp[1];
    const float alv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float bev[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float gsv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = r0 + 64 * j;
      const uint32_t u[4] = {S.g[j].x, S.g[j].y, S.g[j].z, S.g[j].w};
      const uint32_t uy[4] = {S.y[j].x, S.y[j].y, S.y[j].z, S.y[j].w};
      float v[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[2 * q] = fma1(bf16_lo(u[q]), gsv[2 * q], fma1(bev[2 * q], bf16_lo(uy[q]), alv[2 * q]));
        v[2 * q + 1] = fma1(bf16_hi(u[q]), gsv[2 * q + 1], fma1(bev[2 * q + 1], bf16_hi(uy[q]), alv[2 * q + 1]));
      }
      uint4 o = make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
      if ((long)c * kPX + row >= a.M) o = make_uint4(0, 0, 0, 0);  // a zero row folds to alpha
      *reinterpret_cast<uint4*>(G + row * kKT + 8 * (cc ^ gswz(row))) = o;
    }
  };
  // A = relu(x*xs + xt) (ACTBWD) or x -> Al[buf]; store_tile's arithmetic
  auto store_a = [&](const uint4 (&X)[2], int c, int buf) {
    bf16* A = Al + buf * (kPX * CI);
    float sv[8], tv[8];
    if constexpr (ACTBWD) {
      const float4* sp = reinterpret_cast<const float4*>(prm + 3 * CO + cc * 8);
      const float4* tp = reinterpret_cast<const float4*>(prm + 3 * CO + CI + cc * 8);
      const float4 s0 = sp[0], s1 = sp[1], t0 = tp[0], t1 = tp[1];
      sv[0] = s0.x; sv[1] = s0.y; sv[2] = s0.z; sv[3] = s0.w; sv[4] = s1.x; sv[5] = s1.y; sv[6] = s1.z; sv[7] = s1.w;
      tv[0] = t0.x; tv[1] = t0.y; tv[2] = t0.z; tv[3] = t0.w; tv[4] = t1.x; tv[5] = t1.y; tv[6] = t1.z; tv[7] = t1.w;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = r0 + 64 * j;
      uint4 o = X[j];
      if constexpr (ACTBWD) {
        xraw[j * kNT + tid] = o;  // for this thread's epilogue rows (no other thread touches it)
        const uint32_t u[4] = {o.x, o.y, o.z, o.w};
        float v[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[2 * q] = bf16_lo(u[q]); v[2 * q + 1] = bf16_hi(u[q]); }
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = fma1(v[q], sv[q], tv[q]);
        o = make_uint4(pk_act<kActRelu>(v[0], v[1]), pk_act<kActRelu>(v[2], v[3]), pk_act<kActRelu>(v[4], v[5]),
                       pk_act<kActRelu>(v[6], v[7]));
        if ((long)c * kPX + row >= a.M) o = make_uint4(0, 0, 0, 0);  // relu(xt) is not zero
      }
      *reinterpret_cast<uint4*>(A + row * CI + 8 * (cc ^ gswz(row))) = o;
    }
  };

  // ---- requests of the first chunk, then the LDS set-up behind them
  Stage S[NKT];
  uint4 xc[2], xn[2];
  load_x(xc, c_begin);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) load_tile(S[kt], c_begin, kt);

  for (int i = tid; i < CO; i += kNT) {
    prm[i] = a.al[i];
    prm[CO + i] = a.be[i];
    prm[2 * CO + i] = a.gs ? a.gs[i] : 1.f;
  }
  if constexpr (ACTBWD) {
    for (int i = tid; i < CI; i += kNT) {
      prm[3 * CO + i] = a.xs[i];
      prm[3 * CO + CI + i] = a.xt[i];
      prm[3 * CO + 2 * CI + i] = a.es[i];
      prm[3 * CO + 3 * CI + i] = a.et[i];
    }
  }
  for (int i = tid; i < (kNT / 64) * 2 * CI; i += kNT) red[i] = 0.f;  // statistics sums across chunks
  // Wd image: 512-B rows (two bank rows), chunk ^ (row & 15): the 16 rows of a b128 lane group
  // take 16 distinct slots
#pragma unroll
  for (int j = 0; j < CI * WCH / kNT; ++j) {
    const int e = tid + j * kNT;
    const int row = e / WCH, ch = e % WCH;
    *reinterpret_cast<uint4*>(Wl + row * CO + 8 * (ch ^ (row & 15))) =
        *reinterpret_cast<const uint4*>(a.wd + row * CO + ch * 8);
  }
  __syncthreads();

  // wave roles.  Data gradient: 32 pixels (pb) x 32 input channels (cb) of the chunk, every K
  // tile.  Weight gradient: the 32 x 32 tile (cw, cb) of the 64 co x 64 ci of K tiles 2 kh and
  // 2 kh + 1 over all 128 pixels -- 32 accumulator registers per lane; waves w and w + 4 take
  // turns (K tiles 0-1 / 2-3), so the MFMAs per tile are the same for every pair.
  const int cb = wid & 1, pb = wid >> 1, cw = (wid >> 1) & 1;
  const int kh = __builtin_amdgcn_readfirstlane(wid >> 2);
  const int gq = (lane & 15) >> 2, gp4 = lane & 3;
  const int colg = ((lane >> 4) & 1) * 16;

  f32x16 accw[2], accx;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[i][r] = 0.f;

  auto compute = [&](int kt, int gbuf, int abuf) {
    const bf16* G = Gl + gbuf * (kPX * kKT);
    const bf16* A = Al + abuf * (kPX * CI);
    // data gradient: K = this tile's 64 co
    const int wrow = cb * 32 + l31, grow = pb * 32 + l31;
#pragma unroll
    for (int ks = 0; ks < kKT / 16; ++ks) {
      const int ch = ks * 2 + h;
      const bf16x8_t wf =
          *reinterpret_cast<const bf16x8_t*>(Wl + wrow * CO + 8 * ((kt * (kKT / 8) + ch) ^ (wrow & 15)));
      const bf16x8_t gf = *reinterpret_cast<const bf16x8_t*>(G + grow * kKT + 8 * (ch ^ gswz(grow)));
      accx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, gf, accx, 0, 0, 0);
    }
    // weight gradient: K = the chunk's 128 pixels (a wave-uniform branch: the transposed reads
    // need every lane)
    if ((kt >> 1) != kh) return;
    const int colG = cw * 32 + colg + 4 * gp4, colA = cb * 32 + colg + 4 * gp4;
#pragma unroll
    for (int ks = 0; ks < kPX / 16; ++ks) {
      const int q0 = ks * 16 + 8 * h + gq, q1 = q0 + 4;
      const bf16x4_t glo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4*)(G + q0 * kKT + 8 * ((colG >> 3) ^ gswz(q0)) + (colG & 7)));
      const bf16x4_t ghi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4*)(G + q1 * kKT + 8 * ((colG >> 3) ^ gswz(q1)) + (colG & 7)));
      const bf16x4_t alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4*)(A + q0 * CI + 8 * ((colA >> 3) ^ gswz(q0)) + (colA & 7)));
      const bf16x4_t ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4*)(A + q1 * CI + 8 * ((colA >> 3) ^ gswz(q1)) + (colA & 7)));
      const bf16x8_t af = {glo[0], glo[1], glo[2], glo[3], ghi[0], ghi[1], ghi[2], ghi[3]};
      const bf16x8_t bf = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
      accw[kt & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, accw[kt & 1], 0, 0, 0);
    }
  };


  for (int c = c_begin; c < c_end; ++c) {
    const int ab = (c - c_begin) & 1;
#pragma unroll
    for (int r = 0; r < 16; ++r) accx[r] = 0.f;
    // Buffer reuse, one barrier per K tile: Gl[kt & 1] was last read in the compute two tiles
    // back, which every wave left before the previous barrier; Al[ab] two chunks back.
    // (__syncthreads() waits for this wave's LDS reads, lgkmcnt(0), before the barrier.)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      store_g(S[kt], c, kt, kt & 1);
      if (kt == 0) store_a(xc, c, ab);
      load_tile(S[kt], c + 1, kt);
      if (kt == 0) load_x(xn, c + 1);
      __syncthreads();
      compute(kt, kt & 1, ab);
    }
    // ---- data-gradient epilogue (conv_epilogue's transposition): stage fp32 rows, then each
    // thread finishes 8 channels of two whole rows; the staging rows were last read before the
    // chunk's first barrier
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int g = 2 * p;
      float v[8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float lo = accx[4 * g + q], hi = accx[4 * g + 4 + q];
        swap32(lo, hi);
        v[q] = lo;
        v[4 + q] = hi;
      }
      float* dst = stg + (pb * 32 + l31) * SW + cb * 32 + 16 * p + 8 * h;
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    float esv[8], etv[8];  // (re-read per chunk: 16 registers the K tiles' stages need)
    if constexpr (ACTBWD) {
      const float4* sp = reinterpret_cast<const float4*>(prm + 3 * CO + 2 * CI + cc * 8);
      const float4* tp = reinterpret_cast<const float4*>(prm + 3 * CO + 3 * CI + cc * 8);
      const float4 s0 = sp[0], s1 = sp[1], t0 = tp[0], t1 = tp[1];
      esv[0] = s0.x; esv[1] = s0.y; esv[2] = s0.z; esv[3] = s0.w; esv[4] = s1.x; esv[5] = s1.y; esv[6] = s1.z; esv[7] = s1.w;
      etv[0] = t0.x; etv[1] = t0.y; etv[2] = t0.z; etv[3] = t0.w; etv[4] = t1.x; etv[5] = t1.y; etv[6] = t1.z; etv[7] = t1.w;
    }
    float q0s[8], q1s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { q0s[k] = 0.f; q1s[k] = 0.f; }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int lr = r0 + 64 * j;
      const long m = (long)c * kPX + lr;
      if (m < a.M) {
        const uint32_t e = (uint32_t)m * (uint32_t)CI + (uint32_t)(cc * 8);
        const float4 va = *reinterpret_cast<const float4*>(stg + lr * SW + cc * 8);
        const float4 vb = *reinterpret_cast<const float4*>(stg + lr * SW + cc * 8 + 4);
        float v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
        if constexpr (ACTBWD) {
          const uint4 xr = xraw[j * kNT + tid];
          const uint32_t u[4] = {xr.x, xr.y, xr.z, xr.w};
          float x8[8];
#pragma unroll
          for (int q = 0; q < 4; ++q) { x8[2 * q] = bf16_lo(u[q]); x8[2 * q + 1] = bf16_hi(u[q]); }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float gpv = v[k] * actg<kActRelu>(fmaf(x8[k], esv[k], etv[k]), 1.f);
            v[k] = gpv * esv[k];
            q0s[k] = fmaf(gpv, x8[k], q0s[k]);
            q1s[k] += gpv;
          }
        }
        st_out(ro, e * 2u, a.dx + e, v, a.wthru);
      }
    }
    if constexpr (ACTBWD) {
      // the chunk's sums join the wave's running sums in LDS (16 registers less across the K
      // tiles): lanes l, l + 8, ... of a wave hold the same channels
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          q0s[k] += __shfl_xor(q0s[k], o, 64);
          q1s[k] += __shfl_xor(q1s[k], o, 64);
        }
      }
      if (lane < 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          red[(wid * 2 + 0) * CI + cc * 8 + k] += q0s[k];
          red[(wid * 2 + 1) * CI + cc * 8 + k] += q1s[k];
        }
      }
    }
    xc[0] = xn[0];
    xc[1] = xn[1];
  }

  // ---- flush
  __syncthreads();
  if constexpr (ACTBWD) {
    if (tid < 2 * CI) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < kNT / 64; ++w) t += red[w * 2 * CI + tid];
      const int q = tid / CI, ch = tid - q * CI;
      atomicAdd(&a.part[((long)(blockIdx.x & a.slot_mask) * 2 + q) * CI + ch], t);
    }
  }
  // C[co][ci]: lane column ci = lane & 31, rows co = (r & 3) + 8 (r >> 2) + 4 h
  float* dst = a.dw + (a.det ? (long)blockIdx.x * CO * CI : 0L) +
               ((kh * 2) * kKT + cw * 32 + 4 * h) * CI + cb * 32 + l31;
  if (a.det) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(i * kKT + (r & 3) + 8 * (r >> 2)) * CI] = accw[i][r];
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) atomicAdd(&dst[(i * kKT + (r & 3) + 8 * (r >> 2)) * CI], accw[i][r]);
  }
}

template <int CI, bool ACTBWD>
void launch(const PairArgs& a, int wgs, hipStream_t st) {
  auto k = bwd_pair_kernel<CI, ACTBWD>;
  constexpr size_t lds = pair_lds_bytes(CI);
  static bool set = false;
  if (!set) {
    FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    set = true;
  }
  hipLaunchKernelGGL(k, dim3(wgs), dim3(kNT), lds, st, a);
  FDT_LAUNCH_CHECK();
}

}  // namespace bp

bool conv_bwd_pair_supported(int Cin, int Cout, int epi, int act, int xaff) {
  if (Cin != 64 || Cout != 4 * Cin) return false;
  if (epi == conv::kEpiActBwd) return act == kActRelu && xaff;
  return epi == conv::kEpiStore && act == kActNone && !xaff;
}

// epi: EPI_ACTBWD (ReLU; xs / xt / es / et / part set) or EPI_STORE (identity input).  dw: the
// fp32 [Cout][Cin] gradient; slab: deterministic mode's [wgs][Cout][Cin] workspace.  wgs: the
// most workgroups to use (each takes ceil(chunks / wgs) chunks; fewer are started when that
// leaves some without work).
void conv_bwd_pair(uint64_t g, uint64_t y, uint64_t al, uint64_t be, uint64_t gs, uint64_t wd, uint64_t x, uint64_t xs,
                   uint64_t xt, uint64_t es, uint64_t et, uint64_t dx, uint64_t part, int part_rows, uint64_t dw,
                   uint64_t slab, long M, int Cin, int Cout, int epi, int act, int wgs, int accumulate,
                   uint64_t stream) {
  using namespace bp;
  FDT_CHECK(conv_bwd_pair_supported(Cin, Cout, epi, act, xs != 0), "conv_bwd_pair: unsupported launch");
  FDT_CHECK(g && y && al && be && wd && x && dx && dw, "conv_bwd_pair: missing operand");
  FDT_CHECK((xs == 0) == (xt == 0), "paired params");
  const bool actbwd = epi == conv::kEpiActBwd;
  FDT_CHECK(!actbwd || (es && et && part && part_rows > 0), "conv_bwd_pair: ACTBWD needs es / et / slots");
  FDT_CHECK(M >= 1 && wgs >= 1, "conv_bwd_pair: M, wgs >= 1");
  PairArgs a{};
  a.g = P<const bf16>(g); a.y = P<const bf16>(y); a.wd = P<const bf16>(wd); a.x = P<const bf16>(x);
  a.al = P<const float>(al); a.be = P<const float>(be); a.gs = P<const float>(gs);
  a.xs = P<const float>(xs); a.xt = P<const float>(xt); a.es = P<const float>(es); a.et = P<const float>(et);
  a.dx = P<bf16>(dx);
  a.part = P<float>(part);
  a.M = M;
  a.g_bytes = M * Cout * 2;
  a.x_bytes = M * Cin * 2;
  FDT_CHECK(a.g_bytes < 0x7FFFFFF0L, "conv_bwd_pair: operand exceeds the 2 GiB descriptor range");
  a.nchunks = (int)((M + kPX - 1) / kPX);
  a.cpw = (a.nchunks + wgs - 1) / wgs;
  const int active = (a.nchunks + a.cpw - 1) / a.cpw;
  a.det = deterministic() ? 1 : 0;
  a.wthru = conv_write_through() ? 1 : 0;
  a.slot_mask = actbwd ? stat_slot_mask(part_rows, active) : 0u;
  FDT_CHECK(!a.det || slab != 0, "conv_bwd_pair: deterministic mode needs the slab");
  a.dw = a.det ? P<float>(slab) : P<float>(dw);
  hipStream_t st = as_stream(stream);
  if (!a.det && !accumulate) FDT_HIP_CHECK(hipMemsetAsync(P<float>(dw), 0, (size_t)Cout * Cin * 4, st));
  if (actbwd) launch<64, true>(a, active, st);
  else launch<64, false>(a, active, st);
  if (a.det) wgrad_reduce(slab, dw, active, Cout, Cin, 1, Cin, accumulate, stream);
}

}  // namespace fdt
