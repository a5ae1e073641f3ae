// Rotary embeddings + paged KV write for gfx950 (HBM-bound element kernels,
// 16-byte vector accesses, fp32 math, one bf16 rounding).
//
// vlm_rope2d_vision  replaces apply_rotary_pos_emb_vision
//     (reference mlx_vlm/models/qwen2_vl/vision.py:35-50,141-142)
// vlm_mrope_kvwrite  replaces MRoPERotaryEmbedding.apply_rotary - the fused
//     Metal kernel's numerics (reference mlx_vlm/models/rope_utils.py:567-651,
//     1243-1286; selector rope_utils.py:519-526) - together with
//     KVCache.update_and_fetch (reference mlx_vlm/models/cache.py:345-367),
//     writing into a PAGED cache instead of a contiguous, 256-step-grown one.
//
// Paged KV layout (ours; 64 tokens per page, sized for decode reads):
//   K pool: [page][Hkv][D/8][64][8]  - a wave reading one 8-wide d-chunk of the
//           64 keys of a page issues one contiguous 1 KiB load (lane = key)
//   V pool: [page][Hkv][D][64 slots] - transposed, key slots in the k-slot order of the decode P.V MFMA
//           (vlm_vslot), so a V^T operand fragment (d = lane&15, 8 key slots) is one 16-byte load
#include "common.hpp"
#include "internal.h"
#include "../../include/vlm_hip.h"

namespace {

__device__ __forceinline__ void unpack8(const uint4& u, float* v) {
  v[0] = bf_lo(u.x); v[1] = bf_hi(u.x); v[2] = bf_lo(u.y); v[3] = bf_hi(u.y);
  v[4] = bf_lo(u.z); v[5] = bf_hi(u.z); v[6] = bf_lo(u.w); v[7] = bf_hi(u.w);
}
__device__ __forceinline__ uint4 pack8(const float* v) {
  uint4 o;
  o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]); o.z = pack_bf2(v[4], v[5]); o.w = pack_bf2(v[6], v[7]);
  return o;
}

// qkv [N][3][H][D] bf16 (row stride ld elements); cos/sin [N][D/2] fp32.
// out[d]     = T(x[d] c[d] - x[d+D/2] s[d]);  out[d+D/2] = T(x[d+D/2] c[d] + x[d] s[d]),  d < D/2
__global__ __launch_bounds__(256) void rope2d_vision_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ cs,
                                                            const float* __restrict__ sn, int N, int H, int D, int ld) {
  const int half = D >> 1, cph = half >> 3;  // 8-wide chunks per half head
  const long total = (long)N * 2 * H * cph;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % cph);
  long t = idx / cph;
  const int h = (int)(t % H); t /= H;
  const int which = (int)(t % 2);
  const int n = (int)(t / 2);
  bf16_t* base = qkv + (size_t)n * ld + ((size_t)which * H + h) * D + c * 8;
  const uint4 lo = *reinterpret_cast<const uint4*>(base), hi = *reinterpret_cast<const uint4*>(base + half);
  float a[8], b[8], co[8], si[8], oa[8], ob[8];
  unpack8(lo, a); unpack8(hi, b);
  const float4* cp = reinterpret_cast<const float4*>(cs + (size_t)n * half + c * 8);
  const float4* sp = reinterpret_cast<const float4*>(sn + (size_t)n * half + c * 8);
  const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
  co[0] = c0.x; co[1] = c0.y; co[2] = c0.z; co[3] = c0.w; co[4] = c1.x; co[5] = c1.y; co[6] = c1.z; co[7] = c1.w;
  si[0] = s0.x; si[1] = s0.y; si[2] = s0.z; si[3] = s0.w; si[4] = s1.x; si[5] = s1.y; si[6] = s1.z; si[7] = s1.w;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    oa[j] = a[j] * co[j] - b[j] * si[j];
    ob[j] = b[j] * co[j] + a[j] * si[j];
  }
  *reinterpret_cast<uint4*>(base) = pack8(oa);
  *reinterpret_cast<uint4*>(base + half) = pack8(ob);
}

// One thread = one 8-wide chunk of the low half of a q/k head (+ its partners
// in the high half), or one 8-wide chunk of a v head (copy to the cache).
// IDENT: no block table - the identity layout of the decode step's fused qkv kernels (sequence s owns pages
// [s * max_pages, (s + 1) * max_pages)): vlm_mrope_kvwrite_decode behind a narrow step's qkv projection.
template <bool IDENT>
__global__ __launch_bounds__(256) void mrope_kvwrite_kernel(
    bf16_t* __restrict__ qkv, int ld, int T, int Hq, int Hkv, int D, const int* __restrict__ pos_t,
    const int* __restrict__ pos_h, const int* __restrict__ pos_w, const float* __restrict__ inv_freq, int sec0, int sec1,
    const int* __restrict__ kv_seq, const int* __restrict__ kv_slot, const int* __restrict__ block_table, int max_pages,
    bf16_t* __restrict__ kpool, bf16_t* __restrict__ vpool, float qk_scale, int long_from) {
  const int half = D >> 1, cph = half >> 3;
  // SuScaledRoPE's per-call regime decided on the device (decode steps: T <= 64 rows, kv_slot = the rows' cache offsets):
  // inv_freq holds [2][D/2] (short, long) and the LONG row applies to EVERY row of the call when ANY row's offset has
  // reached original_max_position_embeddings (rope_utils.py:168-172) - the rule of the fused qkv kernels of gemv_*.hip
  if (long_from > 0) {
    bool any_long = false;
    for (int r = 0; r < T; ++r) any_long |= kv_slot[r] >= long_from;
    if (any_long) inv_freq += half;
  }
  const int rot_items = (Hq + Hkv) * cph;      // rotary chunks per token
  const int v_items = Hkv * (D >> 3);          // v copy chunks per token
  const int per_tok = rot_items + v_items;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * per_tok) return;
  const int tok = (int)(idx / per_tok);
  const int it = (int)(idx % per_tok);
  bf16_t* row = qkv + (size_t)tok * ld;

  long page = -1;
  int within = 0;
  if (kpool) {
    const int seq = kv_seq ? kv_seq[tok] : tok;
    const int slot = kv_slot[tok];
    page = IDENT ? (long)seq * max_pages + (slot >> 6) : block_table[(size_t)seq * max_pages + (slot >> 6)];
    within = slot & 63;
  }

  if (it < rot_items) {
    const int head = it / cph, c = it % cph;
    bf16_t* base = row + (size_t)head * D + c * 8;
    float a[8], b[8], oa[8], ob[8];
    unpack8(*reinterpret_cast<const uint4*>(base), a);
    unpack8(*reinterpret_cast<const uint4*>(base + half), b);
    const float pt = (float)pos_t[tok], ph = (float)pos_h[tok], pw = (float)pos_w[tok];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = c * 8 + j;
      const float p = f < sec0 ? pt : (f < sec0 + sec1 ? ph : pw);
      const float ang = p * inv_freq[f];
      float s, co;
      sincosf(ang, &s, &co);
      // SuScaledRoPE multiplies q / k by T(scale) first (a typed op: one rounding; exact no-op at scale 1)
      const float za = rbf(a[j] * qk_scale), zb = rbf(b[j] * qk_scale);
      oa[j] = za * co - zb * s;
      ob[j] = zb * co + za * s;
    }
    const uint4 lo = pack8(oa), hi = pack8(ob);
    *reinterpret_cast<uint4*>(base) = lo;
    *reinterpret_cast<uint4*>(base + half) = hi;
    if (head >= Hq && kpool) {
      const int g = head - Hq;
      const size_t kb = ((size_t)page * Hkv + g) * (size_t)(D >> 3);
      *reinterpret_cast<uint4*>(kpool + ((kb + c) * 64 + within) * 8) = lo;
      *reinterpret_cast<uint4*>(kpool + ((kb + c + cph) * 64 + within) * 8) = hi;
    }
  } else if (vpool) {
    const int vi = it - rot_items;
    const int g = vi / (D >> 3), c = vi % (D >> 3);
    const uint4 v = *reinterpret_cast<const uint4*>(row + (size_t)(Hq + Hkv + g) * D + c * 8);
    bf16_t* vb = vpool + (((size_t)page * Hkv + g) * D + c * 8) * 64 + vlm_vslot(within);   // [D][64 slots]
    vb[0 * 64] = (bf16_t)(v.x & 0xffffu); vb[1 * 64] = (bf16_t)(v.x >> 16);
    vb[2 * 64] = (bf16_t)(v.y & 0xffffu); vb[3 * 64] = (bf16_t)(v.y >> 16);
    vb[4 * 64] = (bf16_t)(v.z & 0xffffu); vb[5 * 64] = (bf16_t)(v.z >> 16);
    vb[6 * 64] = (bf16_t)(v.w & 0xffffu); vb[7 * 64] = (bf16_t)(v.w >> 16);
  }
}

// sum over the 8 lanes {l & ~7 .. l | 7} on the DPP data path (common.hpp wave_sum's first three steps, on the two halves of a
// double); result in all 8.  Every lane of such a group must be active (a disabled source lane reads as 0).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double group8_sum(double v) {
  v += dpp_f64<0xB1>(v);      // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);      // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);     // row_half_mirror
  return v;
}

// The QK-norm form (Qwen3-VL: reference mlx_vlm/models/qwen3_vl/language.py:84-89 q_norm / k_norm = nn.RMSNorm(head_dim) on
// every head between the projection and the rotation; selector rope_utils.py:511-526).  D == 128: the 8 threads that own the
// 8-wide chunk pairs (c, c + 8) of a q / k head are 8 consecutive lanes (per_tok % 8 == 0), so the head's sum of squares is
// 16 values per lane and three DPP steps.  Per head: y = T(w * T(x * rsqrt(mean(x^2) + eps))) - vlm_rmsnorm_residual's
// roundings - then the fp32 rotation of the kernel above on y, one rounding; v is copied as it is.
// INTERLEAVED: frequency f takes the h position when f % 3 == 1 and f < lim_h (= 3 * mrope_section[1]), the w position when
// f % 3 == 2 and f < lim_w (= 3 * mrope_section[2]), else t; chunked: f < lim_h ? t : f < lim_w ? h : w (lim = sec0, sec0 + sec1).
// qw / kw: fp32 [D] norm weights.  eps < 0: eps is read from the float in FRONT of qw (the op-level table of
// vlm_mrope_kvwrite_scaled: [D/2 inv_freq | eps | D q_norm_w | D k_norm_w]).
template <bool IDENT, bool INTERLEAVED>
__global__ __launch_bounds__(256) void mrope_qknorm_kvwrite_kernel(
    bf16_t* __restrict__ qkv, int ld, int T, int Hq, int Hkv, const int* __restrict__ pos_t, const int* __restrict__ pos_h,
    const int* __restrict__ pos_w, const float* __restrict__ inv_freq, int lim_h, int lim_w, const float* __restrict__ qw,
    const float* __restrict__ kw, float eps, const int* __restrict__ kv_seq, const int* __restrict__ kv_slot,
    const int* __restrict__ block_table, int max_pages, bf16_t* __restrict__ kpool, bf16_t* __restrict__ vpool) {
  constexpr int D = 128, half = 64, cph = 8;
  const int rot_items = (Hq + Hkv) * cph, v_items = Hkv * (D >> 3), per_tok = rot_items + v_items;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * per_tok) return;
  const int tok = (int)(idx / per_tok);
  const int it = (int)(idx % per_tok);
  bf16_t* row = qkv + (size_t)tok * ld;

  long page = -1;
  int within = 0;
  if (kpool) {
    const int seq = kv_seq ? kv_seq[tok] : tok;
    const int slot = kv_slot[tok];
    page = IDENT ? (long)seq * max_pages + (slot >> 6) : block_table[(size_t)seq * max_pages + (slot >> 6)];
    within = slot & 63;
  }

  if (it < rot_items) {
    const int head = it / cph, c = it % cph;
    bf16_t* base = row + (size_t)head * D + c * 8;
    float a[8], b[8], oa[8], ob[8];
    unpack8(*reinterpret_cast<const uint4*>(base), a);
    unpack8(*reinterpret_cast<const uint4*>(base + half), b);
    // The head's sum of squares in fp64: a bf16 square has 16 significant bits, so 128 of them add up EXACTLY (no rounding until
    // the values of a head span more than 2^18) - the mean is the correctly rounded one whatever lanes own the head, today's
    // eight or a later form's.  Then 1 / sqrt in two correctly rounded steps (the host's formula, not v_rsq_f32's approximation).
    // An ulp of `inv` moves x * inv across a bf16 rounding boundary for a few elements per million, and behind the rotation such
    // a flip is more than the rotation's own error; 16 fp64 FMAs and 6 DPP moves per thread cost a launch of this size nothing.
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += (double)a[j] * (double)a[j] + (double)b[j] * (double)b[j];
    if (eps < 0.f) eps = qw[-1];
    const float inv = 1.0f / sqrtf((float)(group8_sum(ss) * (1.0 / D)) + eps);
    const float* nw = (head < Hq ? qw : kw) + c * 8;
    const float pt = (float)pos_t[tok], ph = (float)pos_h[tok], pw = (float)pos_w[tok];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = c * 8 + j;
      float p;
      if (INTERLEAVED) p = (f % 3 == 1 && f < lim_h) ? ph : ((f % 3 == 2 && f < lim_w) ? pw : pt);
      else p = f < lim_h ? pt : (f < lim_w ? ph : pw);
      const float ang = p * inv_freq[f];
      float s, co;
      sincosf(ang, &s, &co);
      const float za = rbf(nw[j] * rbf(a[j] * inv)), zb = rbf(nw[j + half] * rbf(b[j] * inv));
      oa[j] = za * co - zb * s;
      ob[j] = zb * co + za * s;
    }
    const uint4 lo = pack8(oa), hi = pack8(ob);
    *reinterpret_cast<uint4*>(base) = lo;
    *reinterpret_cast<uint4*>(base + half) = hi;
    if (head >= Hq && kpool) {
      const int g = head - Hq;
      const size_t kb = ((size_t)page * Hkv + g) * (size_t)(D >> 3);
      *reinterpret_cast<uint4*>(kpool + ((kb + c) * 64 + within) * 8) = lo;
      *reinterpret_cast<uint4*>(kpool + ((kb + c + cph) * 64 + within) * 8) = hi;
    }
  } else if (vpool) {
    const int vi = it - rot_items;
    const int g = vi / (D >> 3), c = vi % (D >> 3);
    const uint4 v = *reinterpret_cast<const uint4*>(row + (size_t)(Hq + Hkv + g) * D + c * 8);
    bf16_t* vb = vpool + (((size_t)page * Hkv + g) * D + c * 8) * 64 + vlm_vslot(within);   // [D][64 slots]
    vb[0 * 64] = (bf16_t)(v.x & 0xffffu); vb[1 * 64] = (bf16_t)(v.x >> 16);
    vb[2 * 64] = (bf16_t)(v.y & 0xffffu); vb[3 * 64] = (bf16_t)(v.y >> 16);
    vb[4 * 64] = (bf16_t)(v.z & 0xffffu); vb[5 * 64] = (bf16_t)(v.z >> 16);
    vb[6 * 64] = (bf16_t)(v.w & 0xffffu); vb[7 * 64] = (bf16_t)(v.w >> 16);
  }
}

// the fetch half of KVCache.update_and_fetch (reference cache.py:345-367: `return self.keys[..., :offset, :], ...`) for a
// PAGED cache: token t's cached (already rotated) k and v rows -> the k / v columns of row t of a token-major qkv buffer
__global__ __launch_bounds__(256) void kv_gather_kernel(bf16_t* __restrict__ qkv, int ld, int T, int Hq, int Hkv, int D,
                                                        const int* __restrict__ kv_seq, const int* __restrict__ kv_slot,
                                                        const int* __restrict__ block_table, int max_pages,
                                                        const bf16_t* __restrict__ kpool, const bf16_t* __restrict__ vpool) {
  const int cpd = D >> 3, per_tok = 2 * Hkv * cpd;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * per_tok) return;
  const int tok = (int)(idx / per_tok);
  int it = (int)(idx % per_tok);
  const bool is_v = it >= Hkv * cpd;
  if (is_v) it -= Hkv * cpd;
  const int g = it / cpd, c = it % cpd;
  const int seq = kv_seq ? kv_seq[tok] : tok, slot = kv_slot[tok];
  const size_t page = (size_t)block_table[(size_t)seq * max_pages + (slot >> 6)];
  const int within = slot & 63;
  bf16_t* row = qkv + (size_t)tok * ld;
  if (!is_v) {
    const uint4 k = *reinterpret_cast<const uint4*>(kpool + (((page * Hkv + g) * (size_t)cpd + c) * 64 + within) * 8);
    *reinterpret_cast<uint4*>(row + (size_t)(Hq + g) * D + c * 8) = k;
  } else {
    const bf16_t* vb = vpool + ((page * Hkv + g) * (size_t)D + c * 8) * 64 + vlm_vslot(within);
    uint4 v;
    v.x = (uint32_t)vb[0 * 64] | ((uint32_t)vb[1 * 64] << 16);
    v.y = (uint32_t)vb[2 * 64] | ((uint32_t)vb[3 * 64] << 16);
    v.z = (uint32_t)vb[4 * 64] | ((uint32_t)vb[5 * 64] << 16);
    v.w = (uint32_t)vb[6 * 64] | ((uint32_t)vb[7 * 64] << 16);
    *reinterpret_cast<uint4*>(row + (size_t)(Hq + Hkv + g) * D + c * 8) = v;
  }
}

}  // namespace

extern "C" int vlm_kv_gather(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* kv_seq, const void* kv_slot,
                             const void* block_table, int max_pages, const void* kpool, const void* vpool, void* stream) {
  if (!qkv || !kv_slot || !block_table || !kpool || !vpool || T < 0 || Hq < 0 || Hkv <= 0 || max_pages <= 0) return VLM_ERR_ARG;
  if (D % 8 != 0 || ld % 8 != 0) return VLM_ERR_SHAPE;
  if (T == 0) return VLM_OK;
  const long total = (long)T * 2 * Hkv * (D / 8);
  hipLaunchKernelGGL(kv_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv,
                     ld, T, Hq, Hkv, D, (const int*)kv_seq, (const int*)kv_slot, (const int*)block_table, max_pages,
                     (const bf16_t*)kpool, (const bf16_t*)vpool);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_rope2d_vision(void* qkv, const void* cos_tab, const void* sin_tab, int N, int H, int D, int ld,
                                 void* stream) {
  if (!qkv || !cos_tab || !sin_tab || N < 0 || H <= 0 || D <= 0) return VLM_ERR_ARG;
  if (D % 16 != 0 || ld % 8 != 0) return VLM_ERR_SHAPE;
  if (N == 0) return VLM_OK;
  const long total = (long)N * 2 * H * (D / 16);
  hipLaunchKernelGGL(rope2d_vision_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (bf16_t*)qkv, (const float*)cos_tab, (const float*)sin_tab, N, H, D, ld);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

extern "C" int vlm_mrope_kvwrite(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* pos_t, const void* pos_h,
                                 const void* pos_w, const void* inv_freq, int sec0, int sec1, const void* kv_seq,
                                 const void* kv_slot, const void* block_table, int max_pages, void* kpool, void* vpool,
                                 void* stream) {
  return vlm_mrope_kvwrite_scaled(qkv, ld, T, Hq, Hkv, D, pos_t, pos_h, pos_w, inv_freq, sec0, sec1, kv_seq, kv_slot, block_table,
                              max_pages, kpool, vpool, 1.f, stream);
}

extern "C" int vlm_mrope_kvwrite_scaled(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* pos_t, const void* pos_h,
                                        const void* pos_w, const void* inv_freq, int sec0, int sec1, const void* kv_seq,
                                        const void* kv_slot, const void* block_table, int max_pages, void* kpool, void* vpool,
                                        float qk_scale, void* stream) {
  if (!qkv || !pos_t || !pos_h || !pos_w || !inv_freq || T < 0 || Hq <= 0 || Hkv <= 0) return VLM_ERR_ARG;
  if ((kpool != nullptr) != (vpool != nullptr)) return VLM_ERR_ARG;
  if (kpool && (!kv_slot || !block_table || max_pages <= 0)) return VLM_ERR_ARG;
  if (sec0 < 0) {      // the QK-norm form: inv_freq = fp32 [D/2 inv_freq | eps | D q_norm_w | D k_norm_w], interleaved selector
    if (qk_scale != 1.f) return VLM_ERR_ARG;
    const float* tab = (const float*)inv_freq;
    return vlm_mrope_qknorm_kvwrite(qkv, ld, T, Hq, Hkv, D, pos_t, pos_h, pos_w, tab, -sec0, sec1, 1, tab + D / 2 + 1,
                                    tab + D / 2 + 1 + D, -1.f, kv_seq, kv_slot, block_table, max_pages, kpool, vpool, stream);
  }
  if (D % 16 != 0 || ld % 8 != 0) return VLM_ERR_SHAPE;
  if (T == 0) return VLM_OK;
  const long total = (long)T * ((Hq + Hkv) * (D / 16) + Hkv * (D / 8));
  hipLaunchKernelGGL(mrope_kvwrite_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (bf16_t*)qkv, ld, T, Hq, Hkv, D, (const int*)pos_t, (const int*)pos_h, (const int*)pos_w,
                     (const float*)inv_freq, sec0, sec1, (const int*)kv_seq, (const int*)kv_slot,
                     (const int*)block_table, max_pages, (bf16_t*)kpool, (bf16_t*)vpool, qk_scale, 0);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

// decode form (library-internal, csrc/engine.hip's wide steps): row b = one decoded token at text position pos[b] (all three
// M-RoPE axes equal), written at slot[b] of block-table row b; long_from > 0: inv_freq = [2][D/2] and the call-wide regime
// is decided from the slots on the device, so a captured wide step crosses the limit without host help
int vlm_mrope_kvwrite_decode(void* qkv, int ld, int B, int Hq, int Hkv, int D, const void* pos, const void* inv_freq, int sec0,
                             int sec1, const void* slot, const void* block_table, int max_pages, void* kpool, void* vpool,
                             float qk_scale, int long_from, void* stream) {
  if (!qkv || !pos || !inv_freq || !slot || !kpool || !vpool || B <= 0 || B > 64 || Hq <= 0 || Hkv <= 0 || max_pages <= 0)
    return VLM_ERR_ARG;
  if (D % 16 != 0 || ld % 8 != 0) return VLM_ERR_SHAPE;
  const long total = (long)B * ((Hq + Hkv) * (D / 16) + Hkv * (D / 8));
  if (!block_table) {      // identity layout (the rows of a narrow decode step over a pool that has no table)
    hipLaunchKernelGGL(mrope_kvwrite_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (bf16_t*)qkv, ld, B, Hq, Hkv, D, (const int*)pos, (const int*)pos, (const int*)pos, (const float*)inv_freq,
                       sec0, sec1, (const int*)nullptr, (const int*)slot, (const int*)nullptr, max_pages, (bf16_t*)kpool,
                       (bf16_t*)vpool, qk_scale, long_from);
    VLM_CHECK_LAUNCH();
    return VLM_OK;
  }
  hipLaunchKernelGGL(mrope_kvwrite_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (bf16_t*)qkv, ld, B, Hq, Hkv, D, (const int*)pos, (const int*)pos, (const int*)pos, (const float*)inv_freq,
                     sec0, sec1, (const int*)nullptr, (const int*)slot, (const int*)block_table, max_pages, (bf16_t*)kpool,
                     (bf16_t*)vpool, qk_scale, long_from);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}

// eps < 0: the kernel reads eps from the float in front of q_norm_w (the op-level table of vlm_mrope_kvwrite_scaled)
int vlm_mrope_qknorm_kvwrite(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* pos_t, const void* pos_h, const void* pos_w,
                             const void* inv_freq, int sec0, int sec1, int interleaved, const void* q_norm_w, const void* k_norm_w,
                             float eps, const void* kv_seq, const void* kv_slot, const void* block_table, int max_pages, void* kpool,
                             void* vpool, void* stream) {
  if (!qkv || !pos_t || !pos_h || !pos_w || !inv_freq || !q_norm_w || !k_norm_w || T < 0 || Hq <= 0 || Hkv <= 0) return VLM_ERR_ARG;
  if ((kpool != nullptr) != (vpool != nullptr)) return VLM_ERR_ARG;
  if (kpool && (!kv_slot || max_pages <= 0)) return VLM_ERR_ARG;
  if (sec0 < 0 || sec1 < 0 || sec0 + sec1 > D / 2) return VLM_ERR_ARG;
  if (D != 128 || ld % 8 != 0) return VLM_ERR_SHAPE;
  if (T == 0) return VLM_OK;
  const int lim_h = interleaved ? 3 * sec1 : sec0, lim_w = interleaved ? 3 * (D / 2 - sec0 - sec1) : sec0 + sec1;
  const long total = (long)T * ((Hq + Hkv) * (D / 16) + Hkv * (D / 8));
  const dim3 grid((unsigned)((total + 255) / 256));
#define QKN_GO(IDENT, IL)                                                                                                          \
  hipLaunchKernelGGL((mrope_qknorm_kvwrite_kernel<IDENT, IL>), grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv, ld, T, Hq, Hkv, \
                     (const int*)pos_t, (const int*)pos_h, (const int*)pos_w, (const float*)inv_freq, lim_h, lim_w,                \
                     (const float*)q_norm_w, (const float*)k_norm_w, eps, (const int*)kv_seq, (const int*)kv_slot,                  \
                     (const int*)block_table, max_pages, (bf16_t*)kpool, (bf16_t*)vpool)
  const bool ident = kpool && !block_table;
  if (ident && interleaved) QKN_GO(true, true);
  else if (ident) QKN_GO(true, false);
  else if (interleaved) QKN_GO(false, true);
  else QKN_GO(false, false);
#undef QKN_GO
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
