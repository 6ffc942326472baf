// MFMA fragment helpers shared by the head-dim-64 attention kernels (attention.hip: dense
// (B, L, H, 64) batches; attention_varlen.hip: packed variable-length sequences).
//
// mfma_f32_32x32x16_bf16; C[row][col]: col = lane & 31, row = (r&3) + 8(r>>2) + 4(lane>>5).
// Every product is oriented so that the accumulator of the first GEMM is already the B operand
// of the next one (its k index = the accumulator's row index, in the permuted order
// row(j) = 16s + 8(j>>2) + 4h + (j&3)); the other operand is read in that same permuted order
// from a [row][kRowLd] LDS row image with the gfx950 transposing read (ds_read_b64_tr_b16).
#pragma once
#include "common.h"

namespace fdt {
namespace attn {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = 64;
constexpr int kRowLd = kD + 8;  // [row][d] images: 144-B rows -> ds_read_b128 of 16 rows hits 64 distinct banks

// 32-bit murmur3 finaliser of a linear (head, query, key) index under the per-call seed (two
// 32-bit multiplies; the 64-bit mix it replaces cost ~3x the VALU work per score element);
// an element is dropped iff the hash is below p * 2^32
__device__ __forceinline__ uint32_t drop_hash(uint64_t seed, uint32_t lin) {
  uint32_t x = lin ^ (uint32_t)seed;
  x += (uint32_t)(seed >> 32);
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// raw v_exp_f32 (exp2f adds a compare / select / ldexp per call for denormal results, which
// probabilities below 2^-126 do not need); exp2(-inf) = 0
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ bf16x8_t ld8(const bf16* p) { return *reinterpret_cast<const bf16x8_t*>(p); }

typedef __attribute__((address_space(3))) bf16x4_t lds_bf16x4;

// Transposed MFMA fragment straight from a ROW image [row][kRowLd] (gfx950 ds_read_b64_tr_b16,
// no transposed LDS copy): lane l gets column c0 + (l & 31) and the k elements = rows
// R..R+3 (lo) and R+8..R+11 (hi), R = r0 + 4h -- the permuted order of the accumulator rows.
// In each 16-lane group lane 4q+p supplies row R+q, columns 16g + 4p..4p+3 (g = (l >> 4) & 1).
__device__ __forceinline__ bf16x8_t ldtr(const bf16* img, int r0, int c0, int lane) {
  const int q = (lane & 15) >> 2, p = lane & 3, g = (lane >> 4) & 1, h = lane >> 5;
  const bf16* p0 = img + (r0 + 4 * h + q) * kRowLd + c0 + 16 * g + 4 * p;
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p0));
  const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p0 + 8 * kRowLd));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ bf16x8_t pack8(const float* v) {
  const uint4 u = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                             pack_bf16x2(v[6], v[7]));
  return __builtin_bit_cast(bf16x8_t, u);
}

__device__ __forceinline__ f32x16 mfma(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

}  // namespace attn
}  // namespace fdt
