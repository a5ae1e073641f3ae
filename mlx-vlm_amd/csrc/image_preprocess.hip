// Image preprocessing for gfx950: Pillow's 8-bit resize and the Qwen2-VL patchify, u8 RGB in, the ViT's bf16 patch
// matrix out.  Entered through vlm_cast_f32_bf16_pad with ld_src == -1 (embed.hip; include/vlm_hip.h documents the mode):
// the kernels replace the host's resize + patchify + fp32 upload + cast of that entry point.
//
// resample_h_kernel   Pillow's ImagingResampleHorizontal_8bpc (src/libImaging/Resample.c): out = clip8((2^21 + sum_i
//                     px[xmin + i] * k[i]) >> 22) in int32 along a row, u8 [H][W][3] -> u8 [H][rw][3]
// resample_v_kernel   ImagingResampleVertical_8bpc: the same arithmetic down the columns, on the u8 the horizontal pass
//                     rounded to (Pillow's order: horizontal, round, vertical)
// patchify_kernel     reference mlx_vlm/models/qwen3_vl/processing_qwen3_vl.py:302-354 (_process_one): rescale + normalise as
//                     a bf16 [3][256] table the host built with the float32 operations of that code, both temporal copies,
//                     rows in merge-window order (gh/m, gw/m, m, m), columns (C, T, ph, pw), the pad columns zero
//
// The coefficient tables come from the host (image_ops.py::resample_coeffs).  Every source index is clamped into the image
// and every tap count into the table, so a bad table gives a wrong picture and never a fault.  The work is a few MB of byte
// traffic: one thread per output byte in the passes (lanes walk consecutive bytes of a row, the taps of a vertical pass are
// whole coalesced rows), one thread per 16-byte store in the patchify.
#include "common.hpp"
#include "internal.h"
#include "../../include/vlm_hip.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;   // Pillow's PRECISION_BITS

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned char clip8(int acc) { return (unsigned char)clampi(acc >> kPrecisionBits, 0, 255); }

// grid (ceil(rw * 3 / 256), H): thread = one byte (x, c) of output row y
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* __restrict__ src, size_t src_stride, int W,
                                                         const int* __restrict__ coeffs, const int* __restrict__ bounds,
                                                         int ksize, unsigned char* __restrict__ dst, int rw) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= rw * 3) return;
  const int x = j / 3, c = j - x * 3;
  const int xmin = bounds[2 * x], n = clampi(bounds[2 * x + 1], 0, ksize);
  const unsigned char* row = src + (size_t)blockIdx.y * src_stride;
  const int* k = coeffs + (size_t)x * ksize;
  int acc = 1 << (kPrecisionBits - 1);
  for (int i = 0; i < n; ++i) acc += (int)row[(size_t)clampi(xmin + i, 0, W - 1) * 3 + c] * k[i];
  dst[(size_t)blockIdx.y * rw * 3 + j] = clip8(acc);
}

// grid (ceil(row_bytes / 256), rh): thread = one byte of output row y; the taps are rows ymin.. of the source
__global__ __launch_bounds__(256) void resample_v_kernel(const unsigned char* __restrict__ src, size_t src_stride, int H,
                                                         const int* __restrict__ coeffs, const int* __restrict__ bounds,
                                                         int ksize, unsigned char* __restrict__ dst, int row_bytes) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= row_bytes) return;
  const int y = blockIdx.y;
  const int ymin = bounds[2 * y], n = clampi(bounds[2 * y + 1], 0, ksize);
  const int* k = coeffs + (size_t)y * ksize;
  int acc = 1 << (kPrecisionBits - 1);
  for (int i = 0; i < n; ++i) acc += (int)src[(size_t)clampi(ymin + i, 0, H - 1) * src_stride + j] * k[i];
  dst[(size_t)y * row_bytes + j] = clip8(acc);
}

// thread = 8 consecutive columns of one output row (one 16-byte store); columns >= cols are zeros
__global__ __launch_bounds__(256) void patchify_kernel(const unsigned char* __restrict__ frame, size_t stride, int gh, int gw,
                                                       const bf16_t* __restrict__ lut, bf16_t* __restrict__ dst, int ld,
                                                       int cols, int ps, int ms, int tps) {
  __shared__ bf16_t s_lut[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) s_lut[i] = lut[i];
  __syncthreads();
  const int cpr = ld >> 3;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)gh * gw * cpr) return;
  const int r = (int)(idx / cpr), ch = (int)(idx - (long)r * cpr);
  // row r = ((bh * (gw / m) + bw) * m + mh) * m + mw  ->  patch (bh * m + mh, bw * m + mw) of the grid
  const int mw = r % ms, mh = (r / ms) % ms, blk = r / (ms * ms);
  const int bw = blk % (gw / ms), bh = blk / (gw / ms);
  const unsigned char* p0 = frame + (size_t)(bh * ms + mh) * ps * stride + (size_t)(bw * ms + mw) * ps * 3;
  const int pp = ps * ps, per_c = tps * pp;
  bf16_t v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int col = ch * 8 + e;
    bf16_t o = 0;
    if (col < cols) {
      const int c = col / per_c, q = (col - c * per_c) % pp;   // the temporal copies are equal: t drops out
      const int py = q / ps, px = q - py * ps;
      o = s_lut[c * 256 + p0[(size_t)py * stride + px * 3 + c]];
    }
    v[e] = o;
  }
  uint4 o4;
  o4.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
  o4.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
  o4.z = (uint32_t)v[4] | ((uint32_t)v[5] << 16);
  o4.w = (uint32_t)v[6] | ((uint32_t)v[7] << 16);
  reinterpret_cast<uint4*>(dst + (size_t)r * ld)[ch] = o4;
}

}  // namespace

VLM_INTERNAL int vlm_image_patches(const vlm_image_patch_args* a, void* dst, int rows, int cols, int ld_dst, void* stream) {
  if (!a || !a->src || a->height <= 0 || a->width <= 0 || a->resized_height <= 0 || a->resized_width <= 0) return VLM_ERR_ARG;
  const int H = a->height, W = a->width, rh = a->resized_height, rw = a->resized_width;
  if (a->src_stride < (long long)W * 3) return VLM_ERR_ARG;
  if (H > 65535 || rh > 65535 || (long long)rw * 3 > 0x7fffffffLL || (long long)W * 3 > 0x7fffffffLL) return VLM_ERR_SHAPE;
  const bool pass_h = a->coeffs_h != nullptr, pass_v = a->coeffs_v != nullptr;
  if (pass_h && (!a->bounds_h || a->ksize_h < 1)) return VLM_ERR_ARG;
  if (pass_v && (!a->bounds_v || a->ksize_v < 1)) return VLM_ERR_ARG;
  if ((!pass_h && rw != W) || (!pass_v && rh != H)) return VLM_ERR_SHAPE;   // a skipped pass keeps the size
  if ((pass_h || pass_v) && !a->frame) return VLM_ERR_ARG;
  if (pass_h && pass_v && !a->tmp_h) return VLM_ERR_ARG;
  const bool patches = a->patch != 0;
  int gh = 0, gw = 0;
  if (patches) {
    if (!dst || !a->lut || a->patch < 0 || a->merge <= 0 || a->temporal <= 0 || a->row_offset < 0 || rows < 0 || cols <= 0 ||
        ld_dst < cols)
      return VLM_ERR_ARG;
    const int win = a->patch * a->merge;
    if (((size_t)dst & 15) != 0) return VLM_ERR_ARG;   // 16-byte stores: with ld_dst % 8 == 0 every row start is aligned
    if (ld_dst % 8 || rh % win || rw % win || (long long)3 * a->temporal * a->patch * a->patch != cols) return VLM_ERR_SHAPE;
    gh = rh / a->patch;
    gw = rw / a->patch;
    if ((long long)a->row_offset + (long long)gh * gw > rows) return VLM_ERR_ARG;
    if ((long long)gh * gw * (ld_dst / 8) > 0x7fffffffLL * 256) return VLM_ERR_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* cur = (const unsigned char*)a->src;
  size_t cur_stride = (size_t)a->src_stride;
  if (pass_h) {
    unsigned char* out = (unsigned char*)(pass_v ? a->tmp_h : a->frame);
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)vlm_cdiv(rw * 3, 256), (unsigned)H), dim3(256), 0, st, cur, cur_stride,
                       W, (const int*)a->coeffs_h, (const int*)a->bounds_h, a->ksize_h, out, rw);
    VLM_CHECK_LAUNCH();
    cur = out;
    cur_stride = (size_t)rw * 3;
  }
  if (pass_v) {
    hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)vlm_cdiv(rw * 3, 256), (unsigned)rh), dim3(256), 0, st, cur,
                       cur_stride, H, (const int*)a->coeffs_v, (const int*)a->bounds_v, a->ksize_v, (unsigned char*)a->frame,
                       rw * 3);
    VLM_CHECK_LAUNCH();
    cur = (const unsigned char*)a->frame;
    cur_stride = (size_t)rw * 3;
  }
  if (patches) {
    const long total = (long)gh * gw * (ld_dst / 8);
    hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cur, cur_stride, gh, gw,
                       (const bf16_t*)a->lut, (bf16_t*)dst + (size_t)a->row_offset * ld_dst, ld_dst, cols, a->patch, a->merge,
                       a->temporal);
    VLM_CHECK_LAUNCH();
  }
  return VLM_OK;
}
