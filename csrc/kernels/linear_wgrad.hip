// Split-K weight gradient of the transformer's linear layers (MI355X / gfx950).
//
//   slab[s][o][i] = sum_{m in split s} gy[m][o] * x[m][i]      (fp32)
//   bslab[s][o]   = sum_{m in split s} gy[m][o]                (fp32, optional)
//
// for bf16 gy [M][out] and x [M][in], both row-contiguous.  The output is small (512 .. 1536
// wide) and the reduction deep (32K tokens), so the tokens are split over workgroups and the
// fp32 slabs summed afterwards in split order (mlp.hip slab_sum_acc; linear_bias_fold below):
// no atomics anywhere, bitwise repeatable.
//
// Work split.  A workgroup owns one (out tile, in tile, token split) triple: a 128 x 128 output
// tile, 4 waves of 64 x 64 (2 x 2 accumulators of mfma_f32_32x32x16_bf16), and walks the
// split's contiguous token range in chunks of KC tokens (64: two workgroups per CU, the default;
// 128: one, measured slower).
// The grid is XCD-mapped (xcd_remap) so the tiles of one token split run on one XCD and share
// its L2 copy of the chunk.  A split covers whole chunks except the last one of the range;
// rows past M are answered with zeros by the buffer descriptors' range check, a split with no
// chunks writes zeros.
//
// Data movement.  The gy and x chunks are register-staged one chunk ahead into a
// double-buffered LDS ring as row images [KC tokens][128 features].  The reduction runs over
// tokens, which are LDS rows, so both MFMA operands are read with the transposing LDS read
// (ds_read_b64_tr_b16): no transposed copy of either operand.
//
// Swizzle.  A row is 256 B = 16 chunks of 16 B; chunk c of row r is stored at chunk
// c ^ 4 * (r & 3).  A transposing read takes, per 16 lanes, 4 consecutive token rows x 32 B;
// lanes 0-31 of a wave cover rows r .. r+3 x 64 B (chunks 4j .. 4j+3 for a 32-column block j).
// The XOR moves row r's 64 B to chunk group j ^ (r & 3): the four rows fall on the four
// distinct 64-B quarters of the 256-B bank image, every bank once per 32 lanes; lanes 32-63
// (rows + 8, the same r & 3) repeat the pattern in the second pass.  Checked by enumerating
// bank = (byte address / 4) % 64 of all 64 lanes for every 16-token step and both operands on
// the host: each half wave touches 64 distinct banks.  The staging stores write one row's 16
// chunks per 16 lanes (a permutation of 256 contiguous bytes) and the bias reads one row's
// 256 B per wave: conflict-free as well.
//
// Bias partials.  The workgroups of in-tile 0 column-sum the gy chunk they staged: wave w sums
// rows [w KC/4, (w+1) KC/4) of the chunk, lane l the column pair 2l, 2l+1 (one 4-B LDS read per
// row, fp32 adds); the four waves' sums are combined in wave order at the end.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   KC =  64: 158 VGPRs, 0 AGPRs, 42 SGPRs, no scratch, no spills, 64 KB dynamic LDS, 2 workgroups / CU
//   KC = 128: 140 VGPRs + 64 AGPRs, 42 SGPRs, no scratch, no spills, 128 KB dynamic LDS, 1 workgroup / CU
//   linear_bias_fold: 6 VGPRs, 14 SGPRs, no LDS
#include "conv_igemm_impl.h"

namespace fdt {
namespace lwg {
using namespace conv;

typedef short bf16x4w_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4w_t lds_bf16x4w;

constexpr int kT = 128;       // output tile edge (out and in)

struct Args {
  const bf16* gy;  // [M][out]
  const bf16* x;   // [M][in]
  float* slab;     // [nsplit][out][in]
  float* bslab;    // [nsplit][out] or nullptr
  int out, in, nbo, nbi, nsplit, nchunks, cps;  // tiles, splits, chunks, chunks per split
  int gy_bytes, x_bytes;
};

// 16-B chunk swizzle of a 256-B row (see the file header)
__device__ __forceinline__ int swz(int row) { return 4 * (row & 3); }

template <int KC>
__global__ __launch_bounds__(256, KC == 64 ? 2 : 1) void linear_wgrad_kernel(const Args a) {
  constexpr int TE = KC * kT;        // one operand tile, bf16 elements
  constexpr int NP = KC * 16 / 256;  // 16-B pieces per thread and operand
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* tiles = reinterpret_cast<bf16*>(smem);  // [2][gy tile | x tile]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ntile = a.nbo * a.nbi;
  const int rid = xcd_remap(blockIdx.x, ntile * a.nsplit);
  const int split = rid / ntile, tile = rid - split * ntile;
  const int bo = tile / a.nbi, bi = tile - bo * a.nbi;
  const int o0 = bo * kT, i0 = bi * kT;
  const int c_begin = split * a.cps;
  int c_end = c_begin + a.cps;
  if (c_end > a.nchunks) c_end = a.nchunks;
  const bool bias = a.bslab != nullptr && bi == 0;  // workgroup-uniform

  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)a.gy, (short)0, a.gy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);

  // per-thread staging pieces: fixed tile-local coordinates, the chunk moves the base.  A row
  // past M lies wholly past the descriptor's range (the operands are contiguous): zeros.
  uint32_t goff[NP], xoff[NP];
  int dst[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int i = tid + j * 256, row = i >> 4, cc = i & 15;
    goff[j] = ((uint32_t)row * (uint32_t)a.out + (uint32_t)(o0 + 8 * cc)) * 2u;
    xoff[j] = ((uint32_t)row * (uint32_t)a.in + (uint32_t)(i0 + 8 * cc)) * 2u;
    dst[j] = row * kT + 8 * (cc ^ swz(row));
  }
  uint4 rgv[NP], rxv[NP];
  auto gload = [&](int c) {
    const uint32_t gb = (uint32_t)c * (uint32_t)KC * (uint32_t)a.out * 2u;
    const uint32_t xb = (uint32_t)c * (uint32_t)KC * (uint32_t)a.in * 2u;
#pragma unroll
    for (int j = 0; j < NP; ++j) rgv[j] = ld_buf16(rg, gb + goff[j]);
#pragma unroll
    for (int j = 0; j < NP; ++j) rxv[j] = ld_buf16(rx, xb + xoff[j]);
  };
  auto lstore = [&](int buf) {
    bf16* Gl = tiles + buf * 2 * TE;
    bf16* Xl = Gl + TE;
#pragma unroll
    for (int j = 0; j < NP; ++j) *reinterpret_cast<uint4*>(Gl + dst[j]) = rgv[j];
#pragma unroll
    for (int j = 0; j < NP; ++j) *reinterpret_cast<uint4*>(Xl + dst[j]) = rxv[j];
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.f;
  float bs0 = 0.f, bs1 = 0.f;

  // transposed fragment reads (conv_wh3.hip): lane (gq, gp) of a 16-lane group supplies row
  // gq's 4 columns 4gp..4gp+3; lane l receives column l & 31, rows 8h..8h+7 of the 16-row step
  const int gq = (lane & 15) >> 2, gp = lane & 3, h = lane >> 5;
  const int colg = ((lane >> 4) & 1) * 16;
  const int wo = wid & 1, wi = wid >> 1;  // this wave's 64 x 64 quarter of the tile
  const int gcol = wo * 64 + colg + 4 * gp, xcol = wi * 64 + colg + 4 * gp;

  auto frag = [&](const bf16* T, int r0, int col) {
    const int r1 = r0 + 4;
    const bf16* p0 = T + r0 * kT + 8 * ((col >> 3) ^ swz(r0)) + (col & 7);
    const bf16* p1 = T + r1 * kT + 8 * ((col >> 3) ^ swz(r1)) + (col & 7);
    const bf16x4w_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4w*)(p0));
    const bf16x4w_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4w*)(p1));
    return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  auto compute = [&](int buf) {
    const bf16* Gl = tiles + buf * 2 * TE;
    const bf16* Xl = Gl + TE;
#pragma unroll
    for (int ks = 0; ks < KC / 16; ++ks) {
      const int r0 = ks * 16 + 8 * h + gq;
      bf16x8_t af[2], bfv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = frag(Gl, r0, gcol + 32 * i);
#pragma unroll
      for (int n = 0; n < 2; ++n) bfv[n] = frag(Xl, r0, xcol + 32 * n);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfv[n], acc[i][n], 0, 0, 0);
    }
    if (bias) {
#pragma unroll
      for (int rr = 0; rr < KC / 4; ++rr) {
        const int row = wid * (KC / 4) + rr;
        const uint32_t u =
            *reinterpret_cast<const uint32_t*>(Gl + row * kT + 8 * ((lane >> 2) ^ swz(row)) + 2 * (lane & 3));
        bs0 += bf16_lo(u);
        bs1 += bf16_hi(u);
      }
    }
  };

  if (c_begin < c_end) {
    gload(c_begin);
    lstore(0);
    if (c_begin + 1 < c_end) gload(c_begin + 1);
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
      const int buf = (c - c_begin) & 1;
      compute(buf);
      if (c + 1 < c_end) {
        lstore(buf ^ 1);  // buffer buf^1 was last read in chunk c-1, before the previous barrier
        if (c + 2 < c_end) gload(c + 2);
      }
      __syncthreads();
    }
  }

  // epilogue: accumulator row o = (r&3) + 8(r>>2) + 4h, column i = lane & 31
  float* d = a.slab + (long)split * a.out * a.in;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int ci = i0 + wi * 64 + 32 * n + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = o0 + wo * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
        d[(long)co * a.in + ci] = acc[i][n][r];
      }
    }
  if (bias) {  // (every wave is past its last tile read: the loop ends with a barrier)
    float* red = reinterpret_cast<float*>(smem);  // [4 waves][128 columns]
    red[wid * kT + 2 * lane] = bs0;
    red[wid * kT + 2 * lane + 1] = bs1;
    __syncthreads();
    if (tid < kT)
      a.bslab[(long)split * a.out + o0 + tid] = ((red[tid] + red[kT + tid]) + red[2 * kT + tid]) + red[3 * kT + tid];
  }
}

// dst[c] += sum_s bslab[s * ld + c] for c < n, in split order (one thread per column)
__global__ __launch_bounds__(256) void linear_bias_fold_kernel(const float* __restrict__ bslab,
                                                               float* __restrict__ dst, int nsplit, int ld, int n) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  float s = 0.f;
  for (int j = 0; j < nsplit; ++j) s += bslab[(long)j * ld + c];
  dst[c] += s;
}

inline int& chunk_ref() {
  static int kc = 64;  // measured faster than 128 on every transformer shape
  return kc;
}

}  // namespace lwg

int linear_wgrad_chunk(int kc) {
  const int old = lwg::chunk_ref();
  if (kc > 0) {
    FDT_CHECK(kc == 64 || kc == 128, "linear_wgrad: token chunk 64 or 128");
    lwg::chunk_ref() = kc;
  }
  return old;
}

bool linear_wgrad_supported(long M, int out, int in) {
  return M >= 1 && out >= lwg::kT && in >= lwg::kT && out % lwg::kT == 0 && in % lwg::kT == 0 &&
         M * out * 2 < 0x7FFFFFF0L - 0x1000000L && M * in * 2 < 0x7FFFFFF0L - 0x1000000L;
}

// Two workgroups per CU over the tiles (KC = 64: two resident per CU by their 64 KB of LDS;
// one for KC = 128), but at most 16 splits and at least 8 chunks per split: past that the
// slabs' write and fold traffic costs more than the shorter token walk saves (measured,
// profiles/linear_wgrad/README.md).  No split is empty.
int linear_wgrad_splits(long M, int out, int in) {
  FDT_CHECK(linear_wgrad_supported(M, out, in), "linear_wgrad_splits: unsupported shape");
  const int kc = lwg::chunk_ref();
  const long nchunks = (M + kc - 1) / kc;
  const long tiles = (long)(out / lwg::kT) * (in / lwg::kT);
  long s = (kc == 64 ? 512 : 256) / tiles;
  if (s > nchunks / 8) s = nchunks / 8;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  const long cps = (nchunks + s - 1) / s;
  return (int)((nchunks + cps - 1) / cps);
}

void linear_wgrad(uint64_t gy, uint64_t x, uint64_t slab, uint64_t bslab, long M, int out, int in, int nsplit,
                  uint64_t stream) {
  using namespace lwg;
  FDT_CHECK(linear_wgrad_supported(M, out, in), "linear_wgrad: out, in multiples of 128, operands below 2 GiB");
  FDT_CHECK(gy % 16 == 0 && x % 16 == 0 && slab % 16 == 0 && bslab % 4 == 0 && gy != 0 && x != 0 && slab != 0,
            "linear_wgrad: 16-B aligned operands and slab");
  if (nsplit == 0) nsplit = linear_wgrad_splits(M, out, in);
  FDT_CHECK(nsplit >= 1 && nsplit <= 1024, "linear_wgrad: 1 <= nsplit <= 1024");
  const int kc = chunk_ref();
  Args a{};
  a.gy = P<const bf16>(gy);
  a.x = P<const bf16>(x);
  a.slab = P<float>(slab);
  a.bslab = P<float>(bslab);
  a.out = out; a.in = in;
  a.nbo = out / kT; a.nbi = in / kT;
  a.nsplit = nsplit;
  a.nchunks = (int)((M + kc - 1) / kc);
  a.cps = (a.nchunks + nsplit - 1) / nsplit;  // (splits past the last chunk are empty: zeros)
  a.gy_bytes = (int)(M * out * 2);
  a.x_bytes = (int)(M * in * 2);
  const long grid = (long)a.nbo * a.nbi * nsplit;
  FDT_CHECK(grid < (1L << 24), "linear_wgrad: grid too large");
  hipStream_t st = as_stream(stream);
#define FDT_LWG(KC_)                                                                                     \
  if (kc == KC_) {                                                                                       \
    auto k = linear_wgrad_kernel<KC_>;                                                                   \
    constexpr int lds = 2 * 2 * KC_ * kT * 2;                                                            \
    static bool attr = false;                                                                            \
    if (!attr) {                                                                                         \
      FDT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k),                                \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds));               \
      attr = true;                                                                                       \
    }                                                                                                    \
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), lds, st, a);                                  \
    FDT_LAUNCH_CHECK();                                                                                  \
    return;                                                                                              \
  }
  FDT_LWG(128)
  FDT_LWG(64)
#undef FDT_LWG
}

void linear_bias_fold(uint64_t bslab, uint64_t dst, int nsplit, int ld, int n, uint64_t stream) {
  FDT_CHECK(nsplit >= 1 && n >= 0 && ld >= n && bslab % 4 == 0 && dst % 4 == 0 && bslab != 0 && dst != 0,
            "linear_bias_fold: nsplit >= 1, n <= ld");
  if (n == 0) return;
  lwg::linear_bias_fold_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream)>>>(P<const float>(bslab), P<float>(dst),
                                                                              nsplit, ld, n);
  FDT_LAUNCH_CHECK();
}

}  // namespace fdt
