// LDS reads of v_mfma_f32_16x16x32_bf16 operands, in ONE copy: the transposed pair read (mha.hip, rcda.hip, conv_wgrad.hip)
// and the swizzled 32-row x 32-channel tile of the attention kernels with its two fragment reads (mha.hip, rcda.hip).
// Integer and bit-cast code only: the per-file floating-point flags of the including translation units do not reach it.
#pragma once
#include "common.h"

// two ds_read_b64_tr_b16 (each: a 16 x 4 block of 16-bit elements, transposed across the 16 lanes of a group) as one 8-slot
// operand: slots 0..3 from base0, 4..7 from base1
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
__device__ __forceinline__ bf16x8 tr_read2(const char* base0, const char* base1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base1));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}

// LDS tile of 32 rows x 32 d (64-byte rows), 16-byte chunks XOR-swizzled by (row >> 2) & 3 for the direct b128
// fragment reads and -- equivalently for 32-byte groups -- (row >> 2) & 1 for the transpose reads.
__device__ __forceinline__ int tile_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// direct fragment: lane (t = row, g) -> 8 consecutive d = 8g..8g+7 of row (r16*16 + t)
__device__ __forceinline__ bf16x8 frag_rows(const char* T, int r16, int t, int g) {
  return __builtin_bit_cast(bf16x8, *(const u32x4*)(T + tile_off(r16 * 16 + t, g)));
}
// transposed fragment for the B operand "rows as k slots": lane (t = d within group j, g) -> rows 4g+{0..3} and
// 16+4g+{0..3}; d group j in {0,1}
__device__ __forceinline__ bf16x8 frag_cols(const char* T, int j, int t, int g) {
  const int r0 = 4 * g + (t >> 2), r1 = 16 + r0;
  // 32-byte group j of a row sits at chunks 2j, 2j+1 -> swizzled by the same XOR (it preserves the pair: the XOR
  // value's low bit moves within the pair only if odd, so build the address per 8-byte piece explicitly)
  const int piece = t & 3;                    // 8-byte piece inside the 32-byte group
  const int c0 = 2 * j + (piece >> 1);        // 16-byte chunk holding the piece
  const int a0 = tile_off(r0, c0) + (piece & 1) * 8;
  const int a1 = tile_off(r1, c0) + (piece & 1) * 8;
  return tr_read2(T + a0, T + a1);
}
