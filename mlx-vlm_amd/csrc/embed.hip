// Row gather / scatter / cast kernels for gfx950 (HBM-bound, 16-byte vectors).
//
// vlm_embed_gather        nn.Embedding (reference mlx_vlm/models/qwen2_vl/language.py:164,179)
// vlm_scatter_image_rows  Model.merge_input_ids_with_image_features
//                         (reference mlx_vlm/models/qwen2_vl/qwen2_vl.py:78-148): the cumsum /
//                         gather / where there collapses to "row dst_rows[i] of the embeddings :=
//                         image feature row i" once the image-token positions are known on the host
//                         n < 0: the add form, dst[dst_rows[i]] += src[i] over -n rows (DeepStack,
//                         qwen3_vl/language.py:231-283)
// vlm_cast_f32_bf16_pad   pixel_values.astype(weight dtype) (qwen2_vl.py:44-45) fused with the
//                         zero padding of K = 1176 -> 1216 the patch GEMM wants; ld_src == -1: the rows are made from
//                         a raw u8 image on the device instead (image_preprocess.hip)
// vlm_decode_advance      per-step bookkeeping of the decode loop: KVCache.offset += 1
//                         (reference mlx_vlm/models/cache.py:362) and pos = offset + rope_delta
//                         (language.py:476-509) kept in device memory so a step can be graph-replayed
#include "common.hpp"
#include "internal.h"
#include "../../include/vlm_hip.h"

namespace {

__global__ __launch_bounds__(256) void embed_gather_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ table,
                                                           bf16_t* __restrict__ out, int T, int D, int ldo, int vocab) {
  const int cpr = D >> 3;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * cpr) return;
  const int t = (int)(idx / cpr), c = (int)(idx % cpr);
  int id = ids[t];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  reinterpret_cast<uint4*>(out + (size_t)t * ldo)[c] = reinterpret_cast<const uint4*>(table + (size_t)id * D)[c];
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const bf16_t* __restrict__ src, const int* __restrict__ dst_rows,
                                                           bf16_t* __restrict__ dst, int n, int D, int lds_, int ldd) {
  const int cpr = D >> 3;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * cpr) return;
  const int r = (int)(idx / cpr), c = (int)(idx % cpr);
  reinterpret_cast<uint4*>(dst + (size_t)dst_rows[r] * ldd)[c] = reinterpret_cast<const uint4*>(src + (size_t)r * lds_)[c];
}

// DeepStack (reference mlx_vlm/models/qwen3_vl/language.py:231-283 _deepstack_process): dst[rows[i]] = T(dst[rows[i]] + src[i]),
// one typed bf16 add per element; the rows are distinct, so no two threads meet
__global__ __launch_bounds__(256) void add_rows_kernel(const bf16_t* __restrict__ src, const int* __restrict__ dst_rows,
                                                       bf16_t* __restrict__ dst, int n, int D, int lds_, int ldd) {
  const int cpr = D >> 3;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * cpr) return;
  const int r = (int)(idx / cpr), c = (int)(idx % cpr);
  uint4* d = reinterpret_cast<uint4*>(dst + (size_t)dst_rows[r] * ldd) + c;
  const uint4 a = *d, b = reinterpret_cast<const uint4*>(src + (size_t)r * lds_)[c];
  uint4 o;
  o.x = pack_bf2(bf_lo(a.x) + bf_lo(b.x), bf_hi(a.x) + bf_hi(b.x));
  o.y = pack_bf2(bf_lo(a.y) + bf_lo(b.y), bf_hi(a.y) + bf_hi(b.y));
  o.z = pack_bf2(bf_lo(a.z) + bf_lo(b.z), bf_hi(a.z) + bf_hi(b.z));
  o.w = pack_bf2(bf_lo(a.w) + bf_lo(b.w), bf_hi(a.w) + bf_hi(b.w));
  *d = o;
}

__global__ __launch_bounds__(256) void cast_pad_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int rows,
                                                       int cols, int ld_src, int ld_dst) {
  const int cpr = ld_dst >> 3;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)rows * cpr) return;
  const int r = (int)(idx / cpr), c = (int)(idx % cpr);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = c * 8 + j;
    v[j] = col < cols ? src[(size_t)r * ld_src + col] : 0.f;
  }
  uint4 o;
  o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]); o.z = pack_bf2(v[4], v[5]); o.w = pack_bf2(v[6], v[7]);
  reinterpret_cast<uint4*>(dst + (size_t)r * ld_dst)[c] = o;
}

__global__ void decode_advance_kernel(int* __restrict__ ctx, int* __restrict__ pos, const int* __restrict__ tok,
                                      int* __restrict__ out_ring, int ring_len, int* __restrict__ step, int B, VlmWindow wn) {
  const int b = threadIdx.x;
  const int s = *step;
  if (b < B) {
    vlm_window_advance(ctx, pos, B, b, wn);
    if (out_ring) vlm_ring_store(out_ring, (size_t)(s % ring_len) * B + b, tok[b], wn);
  }
  __syncthreads();
  if (b == 0) *step = s + 1;
}

}  // namespace

extern "C" int vlm_embed_gather(const void* ids, const void* table, void* out, int T, int D, int ldo, int vocab,
                                void* stream) {
  if (!ids || !table || !out || T < 0 || D <= 0 || vocab <= 0) return VLM_ERR_ARG;
  if (D % 8 || ldo % 8) return VLM_ERR_SHAPE;
  if (T == 0) return VLM_OK;
  const long total = (long)T * (D / 8);
  hipLaunchKernelGGL(embed_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const int*)ids, (const bf16_t*)table, (bf16_t*)out, T, D, ldo, vocab);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_scatter_image_rows(const void* src, const void* dst_rows, void* dst, int n, int D, int ld_src,
                                      int ld_dst, void* stream) {
  if (n < 0) return vlm_add_rows(src, dst_rows, dst, -n, D, ld_src, ld_dst, stream);      // the add form (DeepStack)
  if (!src || !dst_rows || !dst || D <= 0) return VLM_ERR_ARG;
  if (D % 8 || ld_src % 8 || ld_dst % 8) return VLM_ERR_SHAPE;
  if (n == 0) return VLM_OK;
  const long total = (long)n * (D / 8);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src, (const int*)dst_rows, (bf16_t*)dst, n, D, ld_src, ld_dst);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

VLM_INTERNAL int vlm_add_rows(const void* src, const void* dst_rows, void* dst, int n, int D, int ld_src, int ld_dst, void* stream) {
  if (!src || !dst_rows || !dst || n < 0 || D <= 0) return VLM_ERR_ARG;
  if (D % 8 || ld_src % 8 || ld_dst % 8) return VLM_ERR_SHAPE;
  if (n == 0) return VLM_OK;
  const long total = (long)n * (D / 8);
  hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src, (const int*)dst_rows, (bf16_t*)dst, n, D, ld_src, ld_dst);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_cast_f32_bf16_pad(const void* src, void* dst, int rows, int cols, int ld_src, int ld_dst,
                                     void* stream) {
  if (ld_src == -1) return vlm_image_patches((const vlm_image_patch_args*)src, dst, rows, cols, ld_dst, stream);   // image mode
  if (!src || !dst || rows < 0 || cols <= 0 || ld_dst < cols) return VLM_ERR_ARG;
  if (ld_dst % 8) return VLM_ERR_SHAPE;
  if (rows == 0) return VLM_OK;
  const long total = (long)rows * (ld_dst / 8);
  hipLaunchKernelGGL(cast_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)src, (bf16_t*)dst, rows, cols, ld_src, ld_dst);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

VLM_INTERNAL int vlm_decode_advance_win(void* ctx, void* pos, const void* tok, void* out_ring, int ring_len, void* step, int B,
                                        VlmWindow wn, void* stream) {
  if (!ctx || !pos || !tok || !step || B <= 0 || B > 256) return VLM_ERR_ARG;
  if (out_ring && ring_len <= 0) return VLM_ERR_ARG;
  if (wn.M > 0 && (wn.K < 0 || wn.M <= wn.K + 1)) return VLM_ERR_ARG;
  hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int*)ctx, (int*)pos,
                     (const int*)tok, (int*)out_ring, ring_len, (int*)step, B, wn);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_decode_advance(void* ctx, void* pos, const void* tok, void* out_ring, int ring_len, void* step, int B,
                                  void* stream) {
  return vlm_decode_advance_win(ctx, pos, tok, out_ring, ring_len, step, B, VlmWindow{0, 0, 0}, stream);
}
