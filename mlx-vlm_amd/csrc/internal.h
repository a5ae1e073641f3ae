// Library-internal entry points (hidden visibility: not part of the C ABI of include/vlm_hip.h).
// They are the forms of the exported operators that the decode engine (csrc/engine.hip) needs.
#pragma once
#include <stddef.h>

#define VLM_INTERNAL __attribute__((visibility("hidden")))

// decode form of vlm_mrope_kvwrite_scaled (csrc/rope.hip): SuScaledRoPE's per-call regime decided on the device
VLM_INTERNAL int vlm_mrope_kvwrite_decode(void* qkv, int ld, int B, int Hq, int Hkv, int D, const void* pos, const void* inv_freq,
                                          int sec0, int sec1, const void* slot, const void* block_table, int max_pages,
                                          void* kpool, void* vpool, float qk_scale, int long_from, void* stream);

// QK-norm form of both (csrc/rope.hip; Qwen3-VL, qwen3_vl/language.py:84-89): per q / k head RMSNorm(head_dim) with q_norm_w /
// k_norm_w (fp32 [D]: the checkpoint's weights widened) and eps, then the rotation and the KV write; D == 128 (VLM_ERR_SHAPE
// otherwise).  interleaved != 0: the interleaved selector over mrope_section (sec0, sec1, D / 2 - sec0 - sec1).  T token rows with
// positions pos_t / pos_h / pos_w (a decode step passes its pos three times and kv_seq == NULL); block_table == NULL with pools:
// the identity layout.  The exported vlm_mrope_kvwrite_scaled reaches it with a negative mrope_sec0.
VLM_INTERNAL int vlm_mrope_qknorm_kvwrite(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* pos_t, const void* pos_h,
                                          const void* pos_w, const void* inv_freq, int sec0, int sec1, int interleaved,
                                          const void* q_norm_w, const void* k_norm_w, float eps, const void* kv_seq,
                                          const void* kv_slot, const void* block_table, int max_pages, void* kpool, void* vpool,
                                          void* stream);

// bf16 form of vlm_attn_prefill_paged_q8 (csrc/attn_prefill_paged.hip): a prompt chunk attending over the bf16 pages; the
// arguments are checked by the exported entry (csrc/attn_prefill_q8.hip), which takes this form when ksb == vsb == NULL
VLM_INTERNAL int vlm_attn_prefill_paged_bf16(const void* q, int ldq, void* out, int ldo, const void* kpool, const void* vpool,
                                             const void* block_table, int max_pages, const void* seg_seq, const void* cu_q,
                                             const void* q_start, int nseg, int total_qblocks, int Hq, int Hkv, float scale,
                                             void* stream);

// one-tile form of vlm_attn_prefill (csrc/attn_window.hip): what the exported entry does with bit 3 of its flag word.  Segments of
// 1 .. 64 tokens, D == 80, Hq == Hkv, max_seg = the caller's declared longest segment (VLM_ERR_SHAPE otherwise, nothing enqueued)
VLM_INTERNAL int vlm_attn_window(const void* q, const void* k, const void* v, void* out, int q_stride, int k_stride, int v_stride,
                                 int o_stride, const void* cu_seqlens, int nseg, int max_seg, int Hq, int Hkv, int D, float scale,
                                 void* stream);

// ---- skinny-M decode GEMM on the matrix cores (csrc/gemv_mfma.hip): 3 <= M <= 16 batch rows
struct VlmRopeKv {
  const int* pos;            // [M] rope position (all three M-RoPE axes are equal for a decoded text token)
  const int* slot;           // [M] KV slot (= tokens already in the cache)
  const float* inv_freq;     // [D/2]
  const int* block_table;    // [M][max_pages] or nullptr (identity layout)
  int max_pages, Hq, Hkv, D;
  unsigned short* kpool;     // [page][Hkv][D/8][64][8]
  unsigned short* vpool;     // [page][Hkv][D][64 key slots]
  float qk_scale = 1.f;      // q and k times this, rounded to bf16, before the rotation (SuScaledRoPE, rope_utils.py:174-176)
  int long_from = 0;         // > 0: inv_freq = [2][D/2] (short, long); long for the whole step when any row's slot >= long_from
};
// split-K workspace of the bf16 GEMMs for kernels captured on another stream than the one that replays them (gemm_bf16.hip)
VLM_INTERNAL int vlm_gemm_splitk_share(void* from_stream, void* to_stream);
VLM_INTERNAL void vlm_gemm_splitk_unshare(void* to_stream);
VLM_INTERNAL size_t vlm_gemv_mfma_ws_bytes(void);
// -> 0 done, > 0 error, -1 shape not handled (take the v_dot2c kernels).  ws: zero-initialised workspace of
// vlm_gemv_mfma_ws_bytes() owned by the caller (one per engine: launches that share it must be stream-ordered), or nullptr
// (no K split across workgroups).  rk != nullptr: the qkv projection with M-RoPE + paged KV write.
VLM_INTERNAL int vlm_gemv_mfma_try(const void* x, const void* W, const void* bias, const void* res, const void* norm_w, void* y,
                                   int M, int N, int K, int ldx, int ldw, int ldy, int ldres, float eps, int epilogue,
                                   const VlmRopeKv* rk, void* ws, void* stream);
VLM_INTERNAL int vlm_gemv_mfma_try_w4(const void* x, const void* Wq, const void* Wsb, const void* bias, const void* res,
                                      const void* norm_w, void* y, int M, int N, int K, int ldx, int ldy, int ldres, float eps,
                                      int epilogue, const VlmRopeKv* rk, void* ws, void* stream);
// second form (csrc/gemv_mfma2.hip): activations in registers, two workgroups per CU, coalesced 4-bit loads; the RMSNorm
// prologue runs as one rows kernel into the workspace scratch at VLM_MFMA_WS_XN_OFFSET.  -1: shape not handled.
#define VLM_MFMA_WS_XN_OFFSET ((size_t)4096 * 256 * 4 + 8192 * 4)
#define VLM_MFMA_WS_XN_BYTES ((size_t)16 * 8192 * 2)
VLM_INTERNAL int vlm_gemv_mfma2_try_bf16(const void* x, const void* W, const void* Wsb, const void* bias, const void* res,
                                         const void* norm_w, void* y, int M, int N, int K, int ldx, int ldw, int ldy, int ldres,
                                         float eps, int epilogue, const VlmRopeKv* rk, void* ws, void* stream);
VLM_INTERNAL int vlm_gemv_mfma2_try_w4(const void* x, const void* W, const void* Wsb, const void* bias, const void* res,
                                       const void* norm_w, void* y, int M, int N, int K, int ldx, int ldw, int ldy, int ldres,
                                       float eps, int epilogue, const VlmRopeKv* rk, void* ws, void* stream);
// long-K form (csrc/gemv_mfma_longk.hip): bf16, no norm prologue, few row tiles; -1: shape not handled
VLM_INTERNAL int vlm_gemv_mfma_longk_try(const void* x, const void* W, const void* bias, const void* res, void* y, int M, int N,
                                         int K, int ldx, int ldw, int ldy, int ldres, int epilogue, void* stream);
VLM_INTERNAL void vlm_gemv_set_variant(int bits);   // A/B bits of the batch-1 launch shapes (process-wide; VLM_TUNE_GEMV_VARIANT)
VLM_INTERNAL void vlm_sample_set_variant(int bits); // ... its bits 13, 14: the forms of the greedy tail's two launches (sample.hip)
VLM_INTERNAL int vlm_gemv_attn_out_exact_ok(int K);   // its bit 12: vlm_gemv_attn_out_bf16 has an exact-split form at K = Hq * D
VLM_INTERNAL void vlm_attn_set_dsplit(int dz);     // its bits 8 / 9: the partial-only page-split attention over 2 / 4 workgroups per page
VLM_INTERNAL int vlm_gemv_bf16_ex(const void* x, const void* W, const void* bias, const void* res, const void* norm_w, void* y,
                                  int M, int N, int K, int ldx, int ldw, int ldy, int ldres, float eps, int epilogue, int mfma,
                                  void* ws, void* stream);
VLM_INTERNAL int vlm_gemv_qkv_rope_kvwrite_ex(const void* h, const void* norm_w, float eps, const void* Wqkv, const void* bqkv,
                                              void* qkv, int ldq, int M, int hidden, int Hq, int Hkv, int D, const void* pos,
                                              const void* slot, const void* inv_freq, const void* block_table, int max_pages,
                                              void* kpool, void* vpool, int mfma, void* ws, float qk_scale, int long_from,
                                              void* stream);
VLM_INTERNAL int vlm_gemv_w4_ex(const void* x, const void* Wq, const void* Wsb, const void* bias, const void* res, const void* norm_w,
                                void* y, int M, int N, int K, int ldx, int ldy, int ldres, float eps, int epilogue, int mfma, void* ws,
                                void* stream);
VLM_INTERNAL int vlm_gemv_w4_qkv_rope_kvwrite_ex(const void* h, const void* norm_w, float eps, const void* Wq, const void* Wsb,
                                                 const void* bqkv, void* qkv, int ldq, int M, int hidden, int Hq, int Hkv, int D,
                                                 const void* pos, const void* slot, const void* inv_freq, const void* block_table,
                                                 int max_pages, void* kpool, void* vpool, int mfma, void* ws, float qk_scale,
                                                 int long_from, void* stream);

// row-slice form of the skinny-M decode GEMM (csrc/gemv_mfma_rows.hip): x in the tiled layout [K / 8][16][8]; -1: shape not handled
VLM_INTERNAL int vlm_gemv_mfma_rows_ok(int M, int N, int K);      // 1: vlm_gemv_mfma_rows_try takes this projection
VLM_INTERNAL int vlm_gemv_mfma_rows_try(const void* xt, const void* W, const void* bias, const void* res, void* y, int M, int N, int K,
                                        int ldw, int ldy, int ldres, int epilogue, void* stream);

// ---- max_kv_size on the device (VLM_DECODE_WINDOW, include/vlm_hip.h): the window rule of a decode step's tail.
// M == 0: no window - ctx / pos are int32 [B] and both advance by one (the public entry points' behaviour).
// M > 0: ctx = [2][B] (n = entries held, w = write slot), pos = [2][B] (p = rope position, d = rope delta); host mirror:
// models/cache.py::window_step (tests/test_window_rule_cpu.py pins both to the reference's RotatingKVCache)
struct VlmWindow {
  int M, K, ring_pos;
  int host_ring;   // VLM_DECODE_HOST_RING: out_ring is pinned host memory (travels with the window: both are options of the tails)
};
// the tail's token-ring entry.  A host-visible ring gets a system-scope vector store: written through to the host at once, so
// the token is there when the step's completion is - no copy launch behind the step
__device__ __forceinline__ void vlm_ring_store(int* ring, size_t i, int v, const VlmWindow wn) {
  if (wn.host_ring) __hip_atomic_store(ring + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else ring[i] = v;
}
__device__ __forceinline__ void vlm_window_advance(int* ctx, int* pos, int B, int b, const VlmWindow wn) {
  if (wn.M <= 0) {
    ctx[b] += 1;
    pos[b] += 1;
    return;
  }
  const int n = ctx[b], w = ctx[B + b], p = pos[b], d = pos[B + b];
  ctx[b] = n + 1 < wn.M - 1 ? n + 1 : wn.M - 1;
  ctx[B + b] = w + 1 == wn.M ? wn.K : w + 1;
  const int r = p - d;                       // the ring's write index as the forward of this step read it
  pos[b] = wn.ring_pos ? (r >= wn.M ? wn.K : r) + 1 + d : p + 1;
}
/* embed.hip: vlm_decode_advance under the window rule */
VLM_INTERNAL int vlm_decode_advance_win(void* ctx, void* pos, const void* tok, void* out_ring, int ring_len, void* step, int B,
                                        VlmWindow wn, void* stream);
/* embed.hip: what vlm_scatter_image_rows does with n < 0 - dst[dst_rows[i]] = T(dst[dst_rows[i]] + src[i]), distinct rows */
VLM_INTERNAL int vlm_add_rows(const void* src, const void* dst_rows, void* dst, int n, int D, int ld_src, int ld_dst, void* stream);
/* sample.hip: vlm_sample_greedy_advance under the window rule */
VLM_INTERNAL int vlm_sample_greedy_advance_win(const void* logits, int ld, int B, int V, void* logprobs, int ldlp, void* tok,
                                               void* workspace, void* ctx, void* pos, void* out_ring, int ring_len, void* step,
                                               const void* embed, void* h, int D, int ldh, VlmWindow wn, void* stream);

/* top_logprobs.hip: the K best (index, log-prob) of every row in the reference's order (value descending, the higher index first
 * among equal values) - what vlm_sample_ex does when vlm_sampler_params.input_is_logprobs == 2 */
VLM_INTERNAL int vlm_top_logprobs(const void* lp, int ld, int B, int V, int K, void* idx, void* val, void* stream);

/* image_preprocess.hip: what vlm_cast_f32_bf16_pad does with ld_src == -1 (u8 image -> resized frame -> bf16 patch rows) */
struct vlm_image_patch_args;
VLM_INTERNAL int vlm_image_patches(const struct vlm_image_patch_args* a, void* dst, int rows, int cols, int ld_dst, void* stream);

/* quantize_w4.hip: what vlm_dequant_w4 does with n_table_rows == -1 (mx.quantize(group_size = 64, bits = 4) of a bf16 matrix
 * [n_rows][K], leading dimension ldw, into Wq [n_rows][K / 8] and Wsb [n_rows][K / 64]) */
VLM_INTERNAL int vlm_quantize_w4(const void* w, void* Wq, void* Wsb, int n_rows, int K, int ldw, void* stream);

VLM_INTERNAL int vlm_sample_last_launches(void);   /* sample.hip: kernels the last vlm_sample / vlm_sample_advance of this thread enqueued */

/* sample.hip: the sampled step's tail for the engine's captured step - vlm_sample (temperature > 0; top_p / min_p / top_k) with the
 * final pick, vlm_decode_advance (under the window rule when wn.M > 0) and the next step's embedding gather in ONE last launch */
VLM_INTERNAL int vlm_sample_advance(const void* logits, int ld, int B, int V, void* logprobs, void* scratch, int ldlp, void* tok,
                                    void* workspace, float temperature, float top_p, float min_p, int top_k, unsigned seed,
                                    void* ctx, void* pos, void* out_ring, int ring_len, void* step, const void* embed, void* h,
                                    int D, int ldh, VlmWindow wn, void* stream);

/* sample.hip: the ROW-TABLE sampler (VLM_SAMPLE_ROW_TABLE: every row's own line in `workspace`) as the tail of the engine's step.
 * ctx != NULL: the final pick also does vlm_decode_advance, the next step's embedding gather and every row's count += 1 (B <= 64,
 * no window); ctx == NULL: the pick and the counts alone */
VLM_INTERNAL int vlm_sample_rows_advance(const void* logits, int ld, int B, int V, void* logprobs, void* scratch, int ldlp, void* tok,
                                         void* workspace, void* ctx, void* pos, void* out_ring, int ring_len, void* step,
                                         const void* embed, void* h, int D, int ldh, VlmWindow wn, void* stream);

/* gemm_bf16.hip: what the reduce launch of a split-K GEMM does ON TOP of its epilogue (the wide decode steps of engine.hip): the
 * launch the caller would otherwise issue next on the reduced rows.  Bit-identical to the two-launch sequence. */
enum { VLM_TAIL_NONE = 0, VLM_TAIL_RMSNORM = 1, VLM_TAIL_ROPE_KV = 2 };
struct VlmGemmTail {
  int kind;
  /* VLM_TAIL_RMSNORM: xn[m] = norm_w * T(C[m] * rsqrt(mean(C[m]^2) + eps)) (vlm_rmsnorm_residual on the rows just written) */
  const void* norm_w;
  float eps;
  void* xn;
  int ldxn;
  /* VLM_TAIL_ROPE_KV: vlm_mrope_kvwrite_decode on the qkv rows just written (row b at text position pos[b], slot[b] of
   * block-table row b) */
  int Hq, Hkv, D;
  const int* pos;
  const float* inv_freq;
  const int* slot;
  const int* block_table;
  int max_pages;
  unsigned short* kpool;
  unsigned short* vpool;
  float qk_scale;
  int long_from;
};
VLM_INTERNAL int vlm_gemm_bf16_tail(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K,
                                    int lda, int ldw, int ldc, int ldres, int epilogue, const VlmGemmTail* tail, int* tail_done,
                                    void* stream);
VLM_INTERNAL int vlm_gemm_w4_tail(const void* A, const void* Wq, const void* Wsb, const void* bias, const void* res, void* C, int M,
                                  int N, int K, int lda, int ldc, int ldres, int epilogue, const VlmGemmTail* tail, int* tail_done,
                                  void* stream);
