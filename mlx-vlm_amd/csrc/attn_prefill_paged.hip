// Causal varlen GQA attention of a prompt CHUNK over the bf16 paged KV cache on gfx950: the keys and values are read straight
// from the pools through the block table - no vlm_kv_gather, no full-length token-major copy of the prefix.  The bf16 twin of
// attn_prefill_q8.hip, reached through the same entry (vlm_attn_prefill_paged_q8 with ksb == vsb == NULL).
//
// It is the attention of a WARM admission of the batch generator's automatic prefix caching (mlx-vlm_amd/apc.py): the matched
// prefix was copied into the sequence's pages, the suffix's own K / V were written by vlm_mrope_kvwrite, and the suffix rows
// attend over [prefix | suffix] in place (reference mlx_vlm/models/base.py:366-373 under the causal mask offset by the cache
// length, fed by KVCache.update_and_fetch, models/cache.py:345-367).
//
// Arithmetic: that of the bf16 kernels at D = 128 (attn_pagesplit.hpp) - S^T = K . Q^T on v_mfma_f32_16x16x32_bf16 (bf16 inputs,
// exact products, fp32 sums), the scores scaled by scale * log2(e) in fp32, softmax in fp32, P fed to O^T += V^T . P^T as the
// hi + lo bf16 pair (vlm_pack_p_hilo: 16 mantissa bits of p), the row sum taken from the fp32 p, one rounding to bf16 at the
// store.  A warm admission is held to the same "hilo" bar as the cold prefill it replaces.
//
// Mapping (attn_prefill_q8.hip's): one wave = 16 consecutive query rows of one head (the N dimension of both transposed
// products, so every softmax statistic is lane-local: row = lane & 15), four such waves per workgroup (64 rows; they walk the
// same pages, which the first to arrive pulls into L2 for the others).  A wave walks its visible keys in units of 32 (half a
// page), every operand fragment ONE 16-byte load from the pool layouts (K [page][Hkv][D/8][64][8], V [page][Hkv][D][64 key
// slots in k-slot order]) - and no LDS, no barrier.  Workgroups with the most keys to walk (the last rows of a segment) are
// dispatched first.
//
// What never reaches a result: slots past a row's own position are masked by a select on the score (they may hold NaN), and
// the V words of slots past the wave's last row are zeroed before the MFMA (p = 0 there, but 0 * NaN is NaN); slots between a
// row's position and the wave's last row are the chunk's own tokens, which the caller has written.  Pages are named by the
// table only: min(k0 / 64, max_pages - 1) of the segment's row.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form -Rpass-analysis=kernel-resource-usage):
//   130 VGPRs, 0 AGPRs, 67 SGPRs, scratch 0 bytes / lane, no spills, LDS 0: 3 waves / SIMD (compiled, cross-compiler report).
//   Two registers over the 4-wave boundary: __launch_bounds__(256, 4) gives 128 VGPRs but spills one (8 bytes of scratch per
//   lane), so it is not taken.  A warm admission launches segments x heads workgroups of at most 4 waves (96 workgroups of 2 live
//   waves at 8 x 32 rows, 12 heads): under one wave per SIMD on 256 CUs, so occupancy does not bound it there; a form that issues
//   the K and the V loads in two batches (kf and vf never live together) is what many-segment launches would want.
#include "attn_pagesplit.hpp"
#include "internal.h"
#include "../../include/vlm_hip.h"

namespace {

constexpr int HD = VLM_HD, PAGE = VLM_PAGE;
constexpr int QWAVE = 16;     // query rows per wave
constexpr int QBLOCK = 64;    // query rows per workgroup

__global__ __launch_bounds__(256) void attn_prefill_paged_kernel(
    const bf16_t* __restrict__ q, bf16_t* __restrict__ out, const bf16_t* __restrict__ kpool, const bf16_t* __restrict__ vpool,
    const int* __restrict__ block_table, const int* __restrict__ seg_seq, const int* __restrict__ cu_q,
    const int* __restrict__ q_start, int ldq, int ldo, int max_pages, int nseg, int Hq, int Hkv, float scale_log2) {
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

  bf16x8_t qf[4];
  {
    const bf16_t* qr = q + (size_t)(row0 + rc) * ldq + (size_t)head * HD + 8 * gq;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) qf[ds] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(qr + 32 * ds));
  }
  f32x4_t ot[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ot[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  for (int k0 = 0; k0 < kv_end; k0 += 32) {
    const size_t page = (size_t)trow[min(k0 >> 6, max_pages - 1)];
    const size_t ph = page * Hkv + g;
    const int hh = (k0 >> 5) & 1;                       // which half of the page
    const bf16_t* kp = kpool + ph * (size_t)(HD / 8) * PAGE * 8 + ((size_t)gq * PAGE + 32 * hh + col) * 8;
    const bf16_t* vp = vpool + ph * (size_t)HD * PAGE + (size_t)col * PAGE + 32 * hh + 8 * gq;
    u32x4_t kf[2][4], vf[8];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds)
        kf[t][ds] = *reinterpret_cast<const u32x4_t*>(kp + ((size_t)(4 * ds) * PAGE + 16 * t) * 8);
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) vf[dt] = *reinterpret_cast<const u32x4_t*>(vp + (size_t)(16 * dt) * PAGE);
    __builtin_amdgcn_sched_barrier(0);    // all loads of the unit in flight before the first MFMA

    // ---- S^T[key 16 t + 4 gq + rr][row col] ----
    f32x4_t st[4];
    float mt = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < 4; ++ds)
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[t][ds]), qf[ds], a, 0, 0, 0);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int key = k0 + 16 * t + 4 * gq + rr;
        const float sv = key <= qpos ? a[rr] * scale_log2 : -INFINITY;      // causal on absolute positions (a masked slot may hold NaN)
        a[rr] = sv;
        mt = fmaxf(mt, sv);
      }
      st[t] = a;
    }
    mt = col4_max(mt);
    // (unit 0 holds slot 0, which every row sees: m_run is finite from the first unit on; a later unit may be wholly masked
    //  for the first rows of the wave - their m stays, their p are 0)
    if (__any(mt > m_run)) {
      const float m_new = fmaxf(m_run, mt);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) ot[dt][rr] *= alpha;
      m_run = m_new;
    }
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = k0 + 16 * t + 4 * gq + rr <= qpos;
        const float p = ok ? __builtin_amdgcn_exp2f(st[t][rr] - m_run) : 0.f;
        st[t][rr] = p;
        ls += p;
      }
    l_run += ls;
    st[2] = st[3] = f32x4_t{0.f, 0.f, 0.f, 0.f};      // the unit is half a page: only step 0 of the pair packing is used
    bf16x8_t phi[2], plo[2];
    vlm_pack_p_hilo(st, phi, plo);
    if (k0 + 32 > kv_end) {
      // the wave's last unit: V words of slots past its last row may hold anything (0 * NaN = NaN)
      const int ka = k0 + 4 * gq, kb = ka + 16;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        u32x4_t vv = vf[dt];
        vv[0] = (ka + 1 < kv_end) ? vv[0] : ((ka < kv_end) ? (vv[0] & 0xffffu) : 0u);
        vv[1] = (ka + 3 < kv_end) ? vv[1] : ((ka + 2 < kv_end) ? (vv[1] & 0xffffu) : 0u);
        vv[2] = (kb + 1 < kv_end) ? vv[2] : ((kb < kv_end) ? (vv[2] & 0xffffu) : 0u);
        vv[3] = (kb + 3 < kv_end) ? vv[3] : ((kb + 2 < kv_end) ? (vv[3] & 0xffffu) : 0u);
        vf[dt] = vv;
      }
    }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf[dt]), phi[0], ot[dt], 0, 0, 0);
      ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf[dt]), plo[0], ot[dt], 0, 0, 0);
    }
  }

  // ---- normalise, store: lane holds O^T[d = 16 dt + 4 gq + rr][row = col] ----
  l_run = col4_sum(l_run);
  if (r < n) {
    const float inv = 1.0f / l_run;
    bf16_t* orow = out + (size_t)(row0 + r) * ldo + (size_t)head * HD + 4 * gq;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      uint2 o;
      o.x = pack_bf2(ot[dt][0] * inv, ot[dt][1] * inv);
      o.y = pack_bf2(ot[dt][2] * inv, ot[dt][3] * inv);
      *reinterpret_cast<uint2*>(orow + 16 * dt) = o;
    }
  }
}

}  // namespace

// the bf16 form of vlm_attn_prefill_paged_q8 (attn_prefill_q8.hip checks the arguments both forms share)
int vlm_attn_prefill_paged_bf16(const void* q, int ldq, void* out, int ldo, const void* kpool, const void* vpool,
                                const void* block_table, int max_pages, const void* seg_seq, const void* cu_q,
                                const void* q_start, int nseg, int total_qblocks, int Hq, int Hkv, float scale, void* stream) {
  hipLaunchKernelGGL(attn_prefill_paged_kernel, dim3(total_qblocks, Hq), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q,
                     (bf16_t*)out, (const bf16_t*)kpool, (const bf16_t*)vpool, (const int*)block_table, (const int*)seg_seq,
                     (const int*)cu_q, (const int*)q_start, ldq, ldo, max_pages, nseg, Hq, Hkv,
                     scale * 1.44269504088896340736f);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
