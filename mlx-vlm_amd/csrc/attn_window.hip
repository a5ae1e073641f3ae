// One-tile attention for gfx950: non-causal attention over segments of 1..64 tokens at head_dim 80 - the window blocks of
// the Qwen2.5-VL vision tower (reference mlx_vlm/models/qwen2_5_vl/vision.py:149-163 with cu_window_seqlens: 112-pixel
// windows = at most 8 x 8 patches).
//
// attn_prefill_kernel (csrc/attn_prefill.hip) gives every segment whole 128-row query blocks and walks the keys in 64-key
// tiles under an online softmax: for a 64-token window half of the workgroup's waves have no query rows, and the running
// max / rescale / double buffer serve a loop of ONE iteration.  Here a segment's whole K and V ARE the one tile:
//   * softmax in a single pass - row max, exp, sum - with nothing to rescale;
//   * one wave = 32 query rows of one (segment, head) pair, two waves share the pair's K / V tile, and a workgroup of four
//     waves carries TWO pairs (consecutive heads of one segment: one contiguous 320-byte run of every token row), so a
//     64-token window fills every wave's MFMA tiles; 46 KiB of LDS -> three workgroups per CU;
//   * rows / keys past the segment end (4, 16, 32-token windows at image edges) are masked; K / V rows past it are staged as
//     zeros, and a 32-key block with no valid key is skipped (wave-uniform).
// The MFMA mapping, the LDS layouts (K rows padded by 16 B, V row pitch 96 with the transposing LDS read) and the spare V
// column of ones that makes the P.V MFMAs return the row sums are attn_prefill_kernel's at D = 80; P is rounded to bf16 for
// the second MFMA, numerator and denominator from the same rounded P.
#include <stdlib.h>

#include "common.hpp"
#include "internal.h"
#include "../../include/vlm_hip.h"

namespace {

constexpr int WD = 80;             // head dim
constexpr int WDP = 96;            // ... padded to the 32-wide d blocks of O^T
constexpr int WT = 64;             // tokens of the one tile
constexpr int WK_LD = WD + 8;      // padded K row (elements)
constexpr int WV_LD = WDP;         // V row pitch: 48 dwords
constexpr int WPAIRS = 2;          // (segment, head) pairs per workgroup
constexpr int WNKS = WD / 16, WNDB = WDP / 32;
constexpr int WCH = WT * WD / 8;   // 16-byte chunks of a K (or V) tile: 640
constexpr int WNCH = 2 * WCH / 128;   // staged chunks per thread of a pair's 128: 10
typedef short w_s16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(4))) __bf16 w_bf16x4_t;

__global__ __launch_bounds__(256, 3) void attn_window_kernel(const bf16_t* __restrict__ qp, const bf16_t* __restrict__ kp,
                                                             const bf16_t* __restrict__ vp, bf16_t* __restrict__ op, int q_stride,
                                                             int k_stride, int v_stride, int o_stride, const int* __restrict__ cu,
                                                             int nseg, int H, float scale_log2) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks2[WPAIRS][WT * WK_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vs2[WPAIRS][WT * WV_LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  __builtin_assume(tid >= 0 && tid < 256);
  const int pw = wave >> 1, wq = wave & 1, t2 = tid & 127;
  const int pair = blockIdx.x * WPAIRS + pw;                       // wave-uniform
  int seg = 0, head = 0, seg_start = 0, seg_len = 0;
  if (pair < nseg * H) {
    seg = pair / H;
    head = pair % H;
    seg_start = cu[seg];
    seg_len = min(cu[seg + 1] - seg_start, WT);                    // (the entry point refuses a declared maximum past the tile)
  }
  const bool active = seg_len > 0;
  bf16_t* Ks = Ks2[pw];
  bf16_t* Vs = Vs2[pw];
  const int qrow = wq * 32 + (lane & 31);                          // row inside the segment
  bf16x8_t qf[WNKS];

  if (active) {
    // ---- the pair's K and V tiles: 1280 16-byte chunks over its 128 threads, every load issued before the first LDS write
    const bf16_t* kbase = kp + (size_t)seg_start * k_stride + (size_t)head * WD;
    const bf16_t* vbase = vp + (size_t)seg_start * v_stride + (size_t)head * WD;
    u32x4_t rs[WNCH];
#pragma unroll
    for (int i = 0; i < WNCH; ++i) {
      const bool isk = i < WNCH / 2;                               // chunks 0 .. 639 are K, the rest V
      const int c = t2 + 128 * i - (isk ? 0 : WCH);
      const int row = c / (WD / 8), ch = c % (WD / 8);
      const u32x4_t z = {0u, 0u, 0u, 0u};
      rs[i] = z;
      if (row < seg_len)
        rs[i] = *reinterpret_cast<const u32x4_t*>((isk ? kbase + (size_t)row * k_stride : vbase + (size_t)row * v_stride) + ch * 8);
    }
    // Q fragments (B operand of S^T): q = lane & 31, d = ks * 16 + 8 h .. + 8
    {
      const bf16_t* qr = qp + (size_t)(seg_start + min(qrow, seg_len - 1)) * q_stride + (size_t)head * WD + 8 * h;
#pragma unroll
      for (int ks = 0; ks < WNKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8_t*>(qr + ks * 16);
    }
#pragma unroll
    for (int i = 0; i < WNCH; ++i) {
      const bool isk = i < WNCH / 2;
      const int c = t2 + 128 * i - (isk ? 0 : WCH);
      const int row = c / (WD / 8), ch = c % (WD / 8);
      *reinterpret_cast<u32x4_t*>(isk ? &Ks[row * WK_LD + ch * 8] : &Vs[row * WV_LD + ch * 8]) = rs[i];
    }
    // the spare columns 80 .. 95 of V: 1.0 in column 80 (row 80 of O^T = the row sums), zeros behind it
    {
      const int row = t2 >> 1, x = t2 & 1;
      const u32x4_t v = {x == 0 ? 0x00003F80u : 0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4_t*>(&Vs[row * WV_LD + WD + 8 * x]) = v;
    }
  }
  __syncthreads();
  if (!active || wq * 32 >= seg_len) return;                        // no barrier below
  const int nkb = seg_len > 32 ? 2 : 1;                             // 32-key blocks that hold a key

  // ---- S^T = K . Q^T ----
  f32x16_t st[2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
  const bf16_t* krow = &Ks[(lane & 31) * WK_LD + 8 * h];
#pragma unroll
  for (int ks = 0; ks < WNKS; ++ks)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
      if (kb < nkb) {
        const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(krow + kb * 32 * WK_LD + ks * 16);
        st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], st[kb], 0, 0, 0);
      }

  // ---- softmax, one pass: q = lane & 31 is lane-local, lane ^ 32 holds the other keys ----
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      st[kb][r] = key < seg_len ? st[kb][r] : -INFINITY;
    }
  float mt = __builtin_elementwise_maximum(st[0][0], st[1][0]);
#pragma unroll
  for (int r = 1; r < 16; ++r) mt = __builtin_elementwise_maximum(mt, __builtin_elementwise_maximum(st[0][r], st[1][r]));
  float ma, mb;
  vlm_xor32_pair(mt, ma, mb);
  const float neg_m = -fmaxf(ma, mb) * scale_log2;                  // key 0 is valid: the max is finite; scale_log2 > 0
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) st[kb][r] = __builtin_amdgcn_exp2f(fmaf(st[kb][r], scale_log2, neg_m));

  // ---- P fragments (B operand of O^T): registers 8 m .. 8 m + 7 of block kb ----
  bf16x8_t pf[2][2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {
      const u32x4_t u = {pack_bf2(st[kb][8 * mm + 0], st[kb][8 * mm + 1]), pack_bf2(st[kb][8 * mm + 2], st[kb][8 * mm + 3]),
                         pack_bf2(st[kb][8 * mm + 4], st[kb][8 * mm + 5]), pack_bf2(st[kb][8 * mm + 6], st[kb][8 * mm + 7])};
      pf[kb][mm] = __builtin_bit_cast(bf16x8_t, u);
    }

  // ---- O^T = V^T . P^T (V^T fragments through the transposing LDS read, as attn_prefill_kernel) ----
  f32x16_t ot[WNDB];
#pragma unroll
  for (int i = 0; i < WNDB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[i][r] = 0.f;
  const bf16_t* vlane = &Vs[(4 * h + ((lane & 15) >> 2)) * WV_LD + 16 * ((lane >> 4) & 1) + 4 * (lane & 3)];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
    if (kb < nkb) {
#pragma unroll
      for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int db = 0; db < WNDB; ++db) {
          const bf16_t* p0 = vlane + (kb * 32 + 16 * mm) * WV_LD + db * 32;
          const w_s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) w_s16x4_t*)(p0));
          const w_s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) w_s16x4_t*)(p0 + 8 * WV_LD));
          const bf16x8_t vf = __builtin_shufflevector(__builtin_bit_cast(w_bf16x4_t, lo), __builtin_bit_cast(w_bf16x4_t, hi), 0, 1, 2,
                                                      3, 4, 5, 6, 7);
          ot[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[kb][mm], ot[db], 0, 0, 0);
        }
    }

  // ---- normalise and store: lane holds O^T[d = db * 32 + (r & 3) + 8 (r >> 2) + 4 h][q = lane & 31]; the row sum is row 80
  //      of O^T: register ot[2][8] of the lanes with h == 0 ----
  float l_a, l_b;
  vlm_xor32_pair(ot[WD / 32][((WD % 32) / 8) * 4], l_a, l_b);
  const float inv = l_a > 0.f ? 1.0f / l_a : 0.f;
  if (qrow < seg_len) {
    bf16_t* orow = op + (size_t)(seg_start + qrow) * o_stride + (size_t)head * WD;
#pragma unroll
    for (int db = 0; db < WNDB; ++db)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int d0 = db * 32 + 8 * r4 + 4 * h;
        if (d0 < WD) {
          uint2 o;
          o.x = pack_bf2(ot[db][4 * r4 + 0] * inv, ot[db][4 * r4 + 1] * inv);
          o.y = pack_bf2(ot[db][4 * r4 + 2] * inv, ot[db][4 * r4 + 3] * inv);
          *reinterpret_cast<uint2*>(orow + d0) = o;
        }
      }
  }
}

}  // namespace

// what vlm_attn_prefill does with bit 3 of its flag word (include/vlm_hip.h); max_seg = the caller's declared longest segment
VLM_INTERNAL int vlm_attn_window(const void* q, const void* k, const void* v, void* out, int q_stride, int k_stride, int v_stride,
                                 int o_stride, const void* cu_seqlens, int nseg, int max_seg, int Hq, int Hkv, int D, float scale,
                                 void* stream) {
  if (D != WD || Hq != Hkv || max_seg > WT) return VLM_ERR_SHAPE;
  if (max_seg <= 0) return VLM_OK;
  if (scale <= 0.f) return VLM_ERR_ARG;
  const long pairs = (long)nseg * Hq;
  if (pairs > 0x7fffffffL) return VLM_ERR_SHAPE;
  hipLaunchKernelGGL(attn_window_kernel, dim3((unsigned)((pairs + WPAIRS - 1) / WPAIRS)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, q_stride, k_stride, v_stride, o_stride,
                     (const int*)cu_seqlens, nseg, Hq, scale * 1.44269504088896340736f);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
