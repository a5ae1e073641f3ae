// Causal varlen GQA attention of a prompt CHUNK over the uniform 8-bit KV cache on gfx950: the keys and values are read
// straight from the 8-bit paged pools through the block table - no gather, no bf16 copy of the prefix.
//
// Replaces quantized_scaled_dot_product_attention at L > 1 with the causal mask offset by the cache length (reference
// mlx_vlm/models/base.py:260-302 behind base.py:305-373, fed by QuantizedKVCache.update_and_fetch with an update of any
// length, models/cache.py:233-334): a chunk prefilled onto a cache that is already 8-bit - turn 2 of a conversation with
// kv_bits, generate_step(prompt_cache=...) - after the chunk's own tokens were quantised (vlm_kv_quantize_tokens).
//
// Arithmetic: the typed graph as the decode kernel states it (attn_decode.hip, attn_decode_pagesplit_q8_kernel) - bf16(scale),
// q * scale rounded to bf16, a score = fp32 sum over the two groups of scale_j * (q . n) + bias_j * sum(q) rounded to bf16
// ONCE, softmax in fp32 with the (unnormalised) probabilities rounded to bf16, P . V with p * scale_v as the fp16 MFMA operand
// and the bias term in fp32.  Bytes enter v_mfma_f32_16x16x32_f16 as the exact values 1024 + n (attn_q8.hpp).
//
// Mapping: one wave = 16 consecutive query rows of one head (the N dimension of both transposed products, so every softmax
// statistic is lane-local: row = lane & 15), four such waves per workgroup (64 rows; they walk the same pages, which the first
// to arrive pulls into L2 / the CU's cache for the others).  A wave walks its visible keys in units of 32 (half a page: the
// register footprint of the decode kernel's half-page form), every operand fragment ONE 8-byte load from the pools - the
// layouts were chosen for that - and no LDS, no barrier.  Workgroups with the most keys to walk (the last rows of a segment)
// are dispatched first.
#include "attn_pagesplit.hpp"
#include "attn_q8.hpp"
#include "internal.h"
#include "../../include/vlm_hip.h"

namespace {

constexpr int HD = VLM_HD, PAGE = VLM_PAGE;
constexpr int QWAVE = 16;     // query rows per wave
constexpr int QBLOCK = 64;    // query rows per workgroup

__global__ __launch_bounds__(256) void attn_prefill_q8_kernel(
    const bf16_t* __restrict__ q, bf16_t* __restrict__ out, const unsigned char* __restrict__ kpool8,
    const unsigned char* __restrict__ vpool8, const unsigned* __restrict__ ksb, const unsigned* __restrict__ vsb,
    const int* __restrict__ block_table, const int* __restrict__ seg_seq, const int* __restrict__ cu_q,
    const int* __restrict__ q_start, int ldq, int ldo, int max_pages, int nseg, int Hq, int Hkv, float scale) {
  // ---- locate (segment, query block): the heaviest block of a segment first ----
  int seg = 0, qb = 0, bid = blockIdx.x;
  for (; seg < nseg; ++seg) {
    const int nb = (cu_q[seg + 1] - cu_q[seg] + QBLOCK - 1) / QBLOCK;
    if (bid < nb) { qb = nb - 1 - bid; break; }
    bid -= nb;
  }
  if (seg >= nseg) return;
  const int head = blockIdx.y, g = head / (Hq / Hkv);
  const int row0 = cu_q[seg], n = cu_q[seg + 1] - row0, qs = q_start[seg];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, gq = lane >> 4;
  const int r0 = qb * QBLOCK + wave * QWAVE;
  if (r0 >= n) return;                                  // (wave-uniform; the kernel has no barrier)
  const int r = r0 + col, rc = min(r, n - 1);           // rows past the chunk's end repeat its last row and are not stored
  const int qpos = qs + rc;                             // absolute position = the last slot this row sees
  const int kv_end = qs + min(r0 + QWAVE, n);           // slots the wave walks: 0 .. its last row's position
  const int* trow = block_table + (size_t)seg_seq[seg] * max_pages;

  // Q fragments with the reference's typed q * scale, and the per-group sums of q the bias terms need
  f16x8_t qf[4];
  float sq[2] = {0.f, 0.f};
  {
    const bf16_t* qr = q + (size_t)(row0 + rc) * ldq + (size_t)head * HD + 8 * gq;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(qr + 32 * ds);
      u32x4_t sc;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned w = raw[j];
        const float a = rbf(bf_lo(w) * scale), c = rbf(bf_hi(w) * scale);      // the typed q * scale (bf16)
        sc[j] = pack_h2(a, c);                                                 // exact in fp16 (8 significant bits)
        sq[ds >> 1] += a + c;
      }
      qf[ds] = __builtin_bit_cast(f16x8_t, sc);
    }
    sq[0] = col4_sum(sq[0]);            // over the four 8-wide d chunks a row's lanes hold per 32-step
    sq[1] = col4_sum(sq[1]);
  }
  f32x4_t ot[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ot[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f, ob[2] = {0.f, 0.f};
  constexpr float LOG2E = 1.44269504088896340736f;

  for (int k0 = 0; k0 < kv_end; k0 += 32) {
    const size_t page = (size_t)trow[min(k0 >> 6, max_pages - 1)];
    const size_t ph = page * Hkv + g;
    const int hh = (k0 >> 5) & 1;                       // which half of the page
    const unsigned char* kp = kpool8 + ph * (size_t)(HD / 8) * PAGE * 8 + ((size_t)gq * PAGE + 32 * hh + col) * 8;
    const unsigned char* vp = vpool8 + ph * (size_t)HD * PAGE + (size_t)col * PAGE + 32 * hh + 8 * gq;
    const unsigned* ks = ksb + (ph * PAGE + 32 * hh + 4 * gq) * 2;
    const unsigned* vs = vsb + (ph * PAGE + 32 * hh + 4 * gq) * 2;
    u32x2_t kf[2][4], vf[8];
    u32x4_t kq[2][2], vq[2][2];           // (scale | bias) words of keys 16 t + 4 gq + r: [t][half]: r = 2 half, 2 half + 1 x 2 groups
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds)
        kf[t][ds] = *reinterpret_cast<const u32x2_t*>(kp + ((size_t)(4 * ds) * PAGE + 16 * t) * 8);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        kq[t][hf] = *reinterpret_cast<const u32x4_t*>(ks + (16 * t) * 2 + 4 * hf);
        vq[t][hf] = *reinterpret_cast<const u32x4_t*>(vs + (16 * t) * 2 + 4 * hf);
      }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) vf[dt] = *reinterpret_cast<const u32x2_t*>(vp + (size_t)(16 * dt) * PAGE);
    __builtin_amdgcn_sched_barrier(0);    // all loads of the unit in flight before the first MFMA

    // ---- S^T: per key tile two group accumulators, then the affine form per (key, group) ----
    float sc[2][4];
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
      a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_frag(kf[t][0]), qf[0], a0, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_frag(kf[t][1]), qf[1], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_frag(kf[t][2]), qf[2], a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_frag(kf[t][3]), qf[3], a1, 0, 0, 0);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const u32x4_t w4 = kq[t][rr >> 1];
        const unsigned w0 = (rr & 1) ? w4[2] : w4[0], w1 = (rr & 1) ? w4[3] : w4[1];     // groups 0 / 1 of key 16 t + 4 gq + rr
        const int key = k0 + 16 * t + 4 * gq + rr;
        // quantized_matmul: fp32 sum over the dequantised keys, one rounding to the query dtype
        // (a_j = q . (1024 + n): the constant leaves through the bias factor)
        const float sv = rbf(bf_lo(w0) * a0[rr] + (bf_hi(w0) - 1024.f * bf_lo(w0)) * sq[0] +
                             bf_lo(w1) * a1[rr] + (bf_hi(w1) - 1024.f * bf_lo(w1)) * sq[1]);
        sc[t][rr] = key <= qpos ? sv * LOG2E : -INFINITY;         // causal on absolute positions (a masked slot may hold NaN words)
        mt = fmaxf(mt, sc[t][rr]);
      }
    }
    mt = col4_max(mt);
    // (unit 0 holds slot 0, which every row sees: m_run is finite from the first unit on; a later unit may be wholly masked
    //  for the first rows of the wave - their m stays, their p are 0)
    if (__any(mt > m_run)) {
      const float m_new = fmaxf(m_run, mt);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
      ob[0] *= alpha;
      ob[1] *= alpha;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) ot[dt][rr] *= alpha;
      m_run = m_new;
    }
    float ls = 0.f, pbias[2] = {0.f, 0.f};
    u32x4_t pk[2];                                 // P'^T fragments [group]
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float pp[2][4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = k0 + 16 * t + 4 * gq + rr <= qpos;
        const float pr = ok ? rbf(__builtin_amdgcn_exp2f(sc[t][rr] - m_run)) : 0.f;     // the probabilities are a bf16 tensor in the reference
        ls += pr;
        const u32x4_t w4 = vq[t][rr >> 1];
        const unsigned w0 = (rr & 1) ? w4[2] : w4[0], w1 = (rr & 1) ? w4[3] : w4[1];
        // the V operands are 1024 + n as well: the constant leaves through the SAME fp16 value p * scale the MFMA takes, so
        // its rounding error multiplies n, not 1024 + n (see the decode kernel)
        pp[0][rr] = ok ? (float)(_Float16)(pr * bf_lo(w0)) : 0.f;
        pp[1][rr] = ok ? (float)(_Float16)(pr * bf_lo(w1)) : 0.f;
        pbias[0] += ok ? pr * bf_hi(w0) - 1024.f * pp[0][rr] : 0.f;
        pbias[1] += ok ? pr * bf_hi(w1) - 1024.f * pp[1][rr] : 0.f;
      }
      // k-slot 8 gq + j of the 32-key step <- tile 0 (j < 4) / tile 1 (j >= 4)
#pragma unroll
      for (int gI = 0; gI < 2; ++gI) {
        pk[gI][t * 2] = pack_h2(pp[gI][0], pp[gI][1]);
        pk[gI][t * 2 + 1] = pack_h2(pp[gI][2], pp[gI][3]);
      }
    }
    l_run += ls;
    ob[0] += pbias[0];
    ob[1] += pbias[1];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(q8_frag(vf[dt]), __builtin_bit_cast(f16x8_t, pk[dt >> 2]), ot[dt], 0, 0, 0);
  }

  // ---- the bias terms (one scalar per (row, group)), normalise, store: lane holds O^T[d = 16 dt + 4 gq + rr][row = col] ----
  ob[0] = col4_sum(ob[0]);
  ob[1] = col4_sum(ob[1]);
  l_run = col4_sum(l_run);
  if (r < n) {
    const float inv = 1.0f / l_run;
    bf16_t* orow = out + (size_t)(row0 + r) * ldo + (size_t)head * HD + 4 * gq;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const float b = ob[dt >> 2];
      uint2 o;
      o.x = pack_bf2((ot[dt][0] + b) * inv, (ot[dt][1] + b) * inv);
      o.y = pack_bf2((ot[dt][2] + b) * inv, (ot[dt][3] + b) * inv);
      *reinterpret_cast<uint2*>(orow + 16 * dt) = o;
    }
  }
}

}  // namespace

extern "C" int vlm_attn_prefill_paged_q8(const void* q, int ldq, void* out, int ldo, const void* kpool8, const void* vpool8,
                                         const void* ksb, const void* vsb, const void* block_table, int max_pages,
                                         const void* seg_seq, const void* cu_q, const void* q_start, int nseg, int total_qblocks,
                                         int Hq, int Hkv, int D, float scale, void* stream) {
  if (!q || !out || !kpool8 || !vpool8 || !block_table || !seg_seq || !cu_q || !q_start) return VLM_ERR_ARG;
  if ((ksb == nullptr) != (vsb == nullptr)) return VLM_ERR_ARG;      // both: the 8-bit pools; neither: the bf16 pools
  if (max_pages <= 0 || nseg <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 || Hq > 65535) return VLM_ERR_ARG;
  if (D != HD || ldq % 8 != 0 || ldo % 4 != 0) return VLM_ERR_SHAPE;
  if (total_qblocks <= 0) return VLM_OK;
  if (!ksb)      // the bf16 form (attn_prefill_paged.hip): kpool8 / vpool8 are the bf16 pools
    return vlm_attn_prefill_paged_bf16(q, ldq, out, ldo, kpool8, vpool8, block_table, max_pages, seg_seq, cu_q, q_start, nseg,
                                       total_qblocks, Hq, Hkv, scale, stream);
  hipLaunchKernelGGL(attn_prefill_q8_kernel, dim3(total_qblocks, Hq), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q,
                     (bf16_t*)out, (const unsigned char*)kpool8, (const unsigned char*)vpool8, (const unsigned*)ksb,
                     (const unsigned*)vsb, (const int*)block_table, (const int*)seg_seq, (const int*)cu_q, (const int*)q_start, ldq,
                     ldo, max_pages, nseg, Hq, Hkv, vlm_bf16_scale(scale));
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
