// mx.quantize(w, group_size = 64, bits = 4) on gfx950: a bf16 matrix -> the engine's 4-bit layout (Wq words + fused
// scale | bias words, include/vlm_hip.h "MLX affine 4-bit weights").  What `mlx_vlm.convert -q` runs on every Linear /
// Embedding it quantises (reference mlx_vlm/quant_utils.py:98-104 -> nn.quantize); reached through vlm_dequant_w4 with
// n_table_rows == -1 (csrc/gemv_w4.hip), the quantise direction of that symbol.
//
// Arithmetic: oracle/quant.py::quantize_affine, the 4-bit twin of q8_group_params / q8_value (csrc/attn_decode.hip) -
// fp32 min / max of the group, scale = max((max - min) / 15, 1e-7) signed so that the edge of larger magnitude lands on an
// integer, q = clip(rint((w - bias) / scale), 0, 15) from the fp32 scale / bias, which are rounded to bf16 (RNE) only when
// stored.  Every division is the IEEE one (__fdiv_rn: v_div_scale / v_div_fmas / v_div_fixup, never v_rcp_f32) and every
// rounding is rintf (ties to even, torch.round's rule): bit-exact with the oracle (tests/test_convert_gpu.py).
//
// Shape: 8 lanes per 64-element group, 8 elements per lane - one 16-byte load per lane, so a wave reads its 8 groups as
// 1 KiB contiguous (rows with ld == K; otherwise 128 contiguous bytes per group).  The group's min / max cross the 8 lanes in
// three DPP steps (the first three of wave_max: the two quad swaps and row_half_mirror stay inside an aligned 8-lane run).
// A lane's 8 nibbles are exactly one output word: coalesced 4-byte stores, 256 contiguous bytes per wave; the lane with
// sub == 0 stores the group's Wsb word.  All indices are size_t (a 7B embedding table is 545 M elements); the grid is capped
// and strides over the rest.
#include "common.hpp"
#include "internal.h"

namespace {

__device__ __forceinline__ float oct_max(float v) {
  v = fmaxf(v, vlm_dpp<0xB1, 0xf>(v, v));      // quad_perm [1,0,3,2]
  v = fmaxf(v, vlm_dpp<0x4E, 0xf>(v, v));      // quad_perm [2,3,0,1]
  return fmaxf(v, vlm_dpp<0x141, 0xf>(v, v));  // row_half_mirror: lane i <-> 7 - i of its 8-lane run = the other quad
}

struct Q4Group { float scale, bias; };
__device__ __forceinline__ Q4Group q4_group_params(float w_max, float w_min) {
  const bool mask = fabsf(w_min) > fabsf(w_max);
  float scale = fmaxf(__fdiv_rn(__fsub_rn(w_max, w_min), 15.0f), 1e-7f);
  scale = mask ? scale : -scale;
  const float edge = mask ? w_min : w_max;
  const float q0 = rintf(__fdiv_rn(edge, scale));
  scale = q0 != 0.f ? __fdiv_rn(edge, q0) : scale;
  return Q4Group{scale, q0 == 0.f ? 0.f : edge};
}
__device__ __forceinline__ unsigned q4_value(float w, Q4Group p) {
  return (unsigned)fminf(fmaxf(rintf(__fdiv_rn(__fsub_rn(w, p.bias), p.scale)), 0.f), 15.f);
}

// thread t = group t / 8, eighth t % 8 of it; group gi = row gi / (K / 64), columns 64 (gi % (K / 64)) .. + 63
__global__ __launch_bounds__(256) void quantize_w4_kernel(const bf16_t* __restrict__ w, unsigned* __restrict__ Wq,
                                                          unsigned* __restrict__ Wsb, size_t n_groups, int groups_per_row,
                                                          size_t ldw) {
  const size_t n_threads = n_groups * 8;
  for (size_t base = (size_t)blockIdx.x * 256; base < n_threads; base += (size_t)gridDim.x * 256) {
    const size_t t = base + threadIdx.x;
    const bool live = t < n_threads;                    // whole 8-lane runs are live or not (n_threads % 8 == 0)
    const size_t gi = live ? t >> 3 : n_groups - 1;     // dead lanes re-read the last group: every lane takes the DPP steps
    const int sub = (int)(t & 7);
    const size_t row = gi / (size_t)groups_per_row, gcol = gi - row * (size_t)groups_per_row;
    const uint4 u = nt_load16(w + row * ldw + gcol * 64 + (size_t)sub * 8);
    float v[8];
    v[0] = bf_lo(u.x); v[1] = bf_hi(u.x); v[2] = bf_lo(u.y); v[3] = bf_hi(u.y);
    v[4] = bf_lo(u.z); v[5] = bf_hi(u.z); v[6] = bf_lo(u.w); v[7] = bf_hi(u.w);
    float mx = v[0], mn = v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) { mx = fmaxf(mx, v[j]); mn = fminf(mn, v[j]); }
    mx = oct_max(mx);
    mn = -oct_max(-mn);
    const Q4Group p = q4_group_params(mx, mn);
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) word |= q4_value(v[j], p) << (4 * j);
    if (live) {
      Wq[t] = word;                                     // [N][K / 8] is contiguous: word index == thread index
      if (sub == 0) Wsb[gi] = (unsigned)f2bf(p.scale) | ((unsigned)f2bf(p.bias) << 16);
    }
  }
}

}  // namespace

int vlm_quantize_w4(const void* w, void* Wq, void* Wsb, int n_rows, int K, int ldw, void* stream) {
  if (!w || !Wq || !Wsb || n_rows < 0 || K <= 0) return VLM_ERR_ARG;
  if (K % 64 != 0 || ldw < K || ldw % 8 != 0 || ((uintptr_t)w & 15) != 0) return VLM_ERR_SHAPE;    // 16-byte loads
  if (n_rows == 0) return VLM_OK;
  const size_t n_groups = (size_t)n_rows * (size_t)(K / 64);
  const size_t blocks = (n_groups * 8 + 255) / 256;
  hipLaunchKernelGGL(quantize_w4_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w, (unsigned*)Wq, (unsigned*)Wsb, n_groups, K / 64, (size_t)ldw);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
