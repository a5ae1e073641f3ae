// Operand helpers shared by the attention kernels over the 8-bit KV pools (attn_decode.hip: the decode step and the
// quantiser; attn_prefill_q8.hip: a prompt chunk).  Pool layouts: see the comment above q8_group_params in attn_decode.hip.
#pragma once
#include <string.h>

#include "common.hpp"

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
// 8 u8 -> 8 fp16 values 1024 + n, ONE v_perm_b32 per two elements: byte n under the constant byte 0x64 is the half-precision
// number 0x64nn = 1024 + n exactly (10 mantissa bits).  The constant 1024 is taken out again in the affine forms of the kernels
// (scale * (q . (1024 + n)) + (bias - 1024 scale) * sum(q)), so no subtraction is spent per element - the u8 -> operand
// conversion costs 4 VALU instructions per 8 elements instead of 12 (v_cvt_f32_ubyte + v_cvt_pk_bf16_f32).
__device__ __forceinline__ f16x8_t q8_frag(const u32x2_t w) {
  const unsigned x = w[0], y = w[1], k = 0x64646464u;
  const u32x4_t v = {__builtin_amdgcn_perm(k, x, 0x04010400u), __builtin_amdgcn_perm(k, x, 0x04030402u),
                     __builtin_amdgcn_perm(k, y, 0x04010400u), __builtin_amdgcn_perm(k, y, 0x04030402u)};
  return __builtin_bit_cast(f16x8_t, v);
}
__device__ __forceinline__ unsigned pack_h2(float lo, float hi) {      // two fp32 -> packed fp16x2 (round to nearest even)
  typedef _Float16 h2_t_ __attribute__((ext_vector_type(2)));
  const h2_t_ v = {(_Float16)lo, (_Float16)hi};
  return __builtin_bit_cast(unsigned, v);
}
// `queries *= scale` (base.py:272) with a python float: MLX converts the weak scalar to the ARRAY's dtype first, so the
// typed multiply uses bf16(scale) (128 ** -0.5 -> 0.08837890625) - pinned by tests/golden/kvquant_ref.npz, where the
// reference's own function runs; round-to-nearest-even on the host
static inline float vlm_bf16_scale(float scale) {
  unsigned u;
  memcpy(&u, &scale, 4);
  u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
  memcpy(&scale, &u, 4);
  return scale;
}
