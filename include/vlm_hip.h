/* vlm_hip.h - C ABI of libvlm_hip.so, the MI355X (gfx950) operator library that
 * replaces the MLX ops on mlx-vlm's generate hot path (Qwen2-VL first).
 *
 * The reference (Blaizzy/mlx-vlm v0.6.15, /root/reference) has NO FFI/plugin ABI
 * of its own: its model code calls straight into the `mlx` Python runtime.  The
 * drop-in boundary is therefore the set of MLX operators that path invokes
 * (SURVEY.md par. 8b); every entry point below names the reference call site it
 * replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked (host); the caller owns
 *     every buffer; bf16 tensors are raw 16-bit words; "ld*" / "*_stride" are
 *     leading dimensions in ELEMENTS
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     every function only enqueues work and returns
 *   - return value: 0 = VLM_OK; 1 = bad argument; 2 = unsupported shape;
 *     1000 + hipError_t = a HIP launch error.  No exceptions cross the ABI.
 *   - no global state; functions are re-entrant; one stream per engine thread
 *     (the reference's contract: one thread-local generation stream,
 *     mlx_vlm/generate/common.py:32)
 */
#ifndef VLM_HIP_H_
#define VLM_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* epilogue flags for vlm_gemm_bf16 / vlm_gemv_bf16 (rounded to bf16 at the same
 * points as the reference's typed graph: after bias, after activation, after
 * the residual add) */
#define VLM_EPI_NONE 0
#define VLM_EPI_BIAS 1       /* + bias[n]                           nn.Linear(bias=True) */
#define VLM_EPI_GELU_FAST 2  /* x*sigmoid(1.702x)                   vision.py:167        */
#define VLM_EPI_GELU_ERF 4   /* exact erf GELU                      vision.py:112        */
#define VLM_EPI_RESIDUAL 8   /* + res[m][n]                         vision.py:188-193, language.py:151-153 */
#define VLM_EPI_SWIGLU 16    /* W rows interleaved (gate_j, up_j): out[j] = silu(g)*u   mlp.py:6-14, activations.py:7-9 */
/* vlm_gemv_bf16_ws only, batched decode steps of 5..16 rows (ABI v8): the activations BETWEEN two projections in the tiled layout
 * t[K / 8][16][8] bf16 (k group, batch row, 8 consecutive k) instead of row-major [M][K] - what the matrix cores' B fragments read
 * as whole cache lines.  Y_TILED: y is written tiled (ldy ignored; y holds 16 * N_out elements, rows M..15 are not written);
 * X_TILED: x is read tiled (ldx ignored) - the row-slice form of the skinny decode GEMM (csrc/gemv_mfma_rows.hip), for projections
 * with at most 16 output rows per compute unit and K >= 4096, K % 128 == 0 (the SwiGLU MLP's down projection, mlp.py:6-14).
 * A shape the flagged kernel does not take is refused (return 2) and nothing is enqueued. */
#define VLM_EPI_X_TILED 64
#define VLM_EPI_Y_TILED 128
/* vlm_gemm_bf16 only, added within ABI v8 (bit 5 is taken inside the library): nn.GELU(approx="tanh"),
 * 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) on the bf16-rounded acc + bias, every elementary op rounded to bf16 as
 * the two GELU forms above (qwen3_vl/vision.py:169).  Every tile, staging and split-K form that takes VLM_EPI_GELU_FAST. */
#define VLM_EPI_GELU_TANH 256
/* vlm_gemm_bf16 only, added within ABI v8: layer scale, x = x + ls * f(x) (internvl_chat/vision.py:126-132).  Valid only as
 * VLM_EPI_BIAS | VLM_EPI_RESIDUAL | VLM_EPI_LAYERSCALE.  `bias` then points at bf16 [2][N], contiguous: row 0 the bias, row 1
 * the per-column scale ls.  C[m][n] = T(res[m][n] + T(T(acc + bias[n]) * ls[n])), T = one rounding to bf16 - the three
 * roundings of the reference's typed graph (Linear, multiply, add).  Every tile, staging and split-K form that takes
 * VLM_EPI_BIAS | VLM_EPI_RESIDUAL; res may be C.  vlm_encoder_forward takes the bit in act_epilogue (below). */
#define VLM_EPI_LAYERSCALE 512

int vlm_abi_version(void);

/* C[M,N] = epi(A[M,K] . W[N,K]^T), bf16 in / fp32 MFMA accumulate / bf16 out.
 * Replaces nn.Linear (mlx_vlm/models/qwen2_vl/vision.py:110-120,129-130,137,161,168-173;
 * language.py:52-55,76,120; models/mlp.py:9-14), embed_tokens.as_linear / lm_head
 * (language.py:514-517) and the Conv3d patch projection (vision.py:83-101).
 * K % 8 == 0, N % 8 == 0.  With VLM_EPI_SWIGLU, C is [M, N/2].
 * Added within ABI v8: VLM_EPI_BIAS | VLM_EPI_SWIGLU (the biased gate / up of qwen2_5_vl/vision.py:166-174) - bias [N]
 * interleaved like W's rows; g = bf16(x Wg^T + bg), u = bf16(x Wu^T + bu), one rounding each, then silu(g) * u. */
int vlm_gemm_bf16(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K,
                  int lda, int ldw, int ldc, int ldres, int epilogue, void* stream);

/* The qkv projection of the vision attention with apply_rotary_pos_emb_vision (vision.py:35-50,141-142) as its epilogue:
 * C = rope2d(A . W^T + bias) on the first rope_cols columns (the q and k heads, head_dim wide), plain bias on the rest.
 * W's q / k rows must be INTERLEAVED per head - row (h, d) of the checkpoint at h * head_dim + 2 d, row (h, d + hd/2) at
 * h * head_dim + 2 d + 1 (q.k is invariant under a common permutation of the head dimension) - so that a rotation pair
 * is two adjacent outputs.  cos_sin: fp32 [2][M][head_dim / 2]: cos rows then sin rows of VisionModel.rot_pos_emb
 * (vision.py:219-255).  Rounding as the reference: bf16(linear + bias), fp32 rotation, one rounding. */
int vlm_gemm_bf16_rope2d(const void* A, const void* W, const void* bias, const void* cos_sin, void* C, int M, int N, int K,
                         int lda, int ldw, int ldc, int head_dim, int rope_cols, void* stream);

/* The same GEMM over MLX affine 4-bit weights, dequantisation FUSED into the W-tile staging (nn.QuantizedLinear /
 * mx.quantized_matmul at L > 1, reference utils.py:918-967): Wq uint32 [N][K/8] (element k of a row in word k / 8, nibble
 * k % 8), Wsb uint32 [N][K/64] (scale bf16 | bias bf16 << 16 per 64-wide group), K % 64 == 0.  The LDS image of a W tile
 * is the one vlm_gemm_bf16 builds from vlm_dequant_w4's output, so C is bit-identical to dequantise-then-GEMM while the
 * weights move at 4.5 bits instead of being written and re-read at 16.  Epilogues: NONE, BIAS, RESIDUAL, BIAS | RESIDUAL,
 * SWIGLU. */
int vlm_gemm_w4(const void* A, const void* Wq, const void* Wsb, const void* bias, const void* res, void* C, int M, int N,
                int K, int lda, int ldc, int ldres, int epilogue, void* stream);

/* test / A-B knob for vlm_gemm_bf16 kernel selection: 0 = automatic (LDS-DMA staging when K % 64 == 0; the phased
 * 256x256 kernel from ~120 tiles up), 1 = 128x128 kernel with global -> VGPR -> LDS staging, 2 = 128x128 kernel with
 * LDS-DMA staging, 3 = 256x256 phased kernel whenever legal (K % 64 == 0, K >= 128, no SwiGLU), 4 = its 2-phase
 * variant, 5 = automatic with the 2-phase variant, 6 / 7 = as 3 with 256x192 / 256x256 tiles forced, 8 = as 2 (named
 * "no split-K"), 9 = 128 kernel family with split-K x4 forced, 10 = as 3 with the persistent tile loop.  Modes 1-8 are bit-identical to each other; split-K (automatic
 * for few tiles and K >= 2048, or mode 9) sums fp32 partials of K ranges and agrees to fp32 summation order.
 * 100 + 10 * splits + cfg (round 6, tile sweeps - scripts/r06/gemm_tiles.py): the plain kernels only, tile cfg 1 = 64 x 64,
 * 2 = 64 x 128, 3 = 128 x 128 (0 = the policy), split-K forced to `splits` K ranges (0 / 1 = never).
 * The automatic policy since round 6: up to 64 rows (wide decode steps, short prompts) 64 x 64 tiles - 32 x 64 up to 32 rows -
 * and split-K from K = 1024, because such a launch is a weight stream and wants workgroups (VLM_GEMM_SKINNY64=0 /
 * VLM_GEMM_SKINNY32=0 in the environment restore the policy of rounds 1-5 for A/B runs). */
int vlm_gemm_set_staging(int mode);

/* y[M,N] = epi(x[M,K] . W[N,K]^T) for the decode step, M in {1,2,4,8}; weight streaming.
 * norm_w != NULL fuses y = f(RMSNorm(x; norm_w, eps)) (language.py:130-133,149-153,200).
 * Same reference call sites as vlm_gemm_bf16 at L == 1.
 * Shapes: K % 8 == 0.  With norm_w: K <= 4096 and M * K * 2 <= 64 KiB of staged rows.  Without: K <= 3584 on the same
 * kernel, longer rows on the split-K kernel: NONE / BIAS / RESIDUAL up to K <= 20480 (<= 30720 for up to 4 rows - the 72B down
 * projection); SWIGLU, whose gate / up pairs need two weight rows per workgroup, up to K <= 20480 for 1 or 2 rows and
 * K <= 10240 for 4 or 8.  Anything else returns 2 and enqueues nothing.  A hidden size past 4096 (up to
 * 8192, Qwen2-VL-72B) runs vlm_rmsnorm_residual and then this call without norm_w: measured faster than a fused kernel. */
int vlm_gemv_bf16(const void* x, const void* W, const void* bias, const void* res, const void* norm_w, void* y, int M,
                  int N, int K, int ldx, int ldw, int ldy, int ldres, float eps, int epilogue, void* stream);

/* Decode-step fusions built on the same kernels (one decoder layer = 5 launches):
 * vlm_gemv_qkv_rope_kvwrite: qkv = RMSNorm(h) Wqkv^T + b (language.py:52-54,76,149), then M-RoPE on the q and k
 *   heads at pos[m] (rope_utils.py:567-651; a decoded text token has equal t/h/w positions, language.py:476-509)
 *   and KVCache.update_and_fetch (cache.py:345-367): rotated q -> qkv[m][0 : Hq*D], rotated k and v -> slot[m] of
 *   sequence m in the paged pools.  pos / slot int32 [M] on the device.  block_table == NULL selects the identity
 *   layout: row m owns pages [m * max_pages, (m + 1) * max_pages) of the pools as passed (no table load).
 * vlm_gemv_attn_out: h += merge(attention split partials) Wo^T (language.py:115-120,151): the split-K merge of
 *   vlm_attn_decode_paged is the GEMV prologue, the residual add its epilogue. */
/* hidden <= 4096, hidden % 8 == 0, D % 16 == 0, M in {1,2,4,8} with M * hidden * 2 <= 64 KiB (else 2, nothing enqueued: a wider
 * model runs vlm_rmsnorm_residual, vlm_gemv_bf16 with VLM_EPI_BIAS and the rotary + KV-write launch - the engine does) */
int vlm_gemv_qkv_rope_kvwrite(const void* h, const void* norm_w, float eps, const void* Wqkv, const void* bqkv,
                              void* qkv, int ldq, int M, int hidden, int Hq, int Hkv, int D, const void* pos,
                              const void* slot, const void* inv_freq, const void* block_table, int max_pages,
                              void* kpool, void* vpool, void* stream);

/* The same projections for a batched decode step of up to 16 rows: from 5 rows on (9 for the qkv form) the batch rows
 * become the N dimension of v_mfma_f32_16x16x32_bf16 (csrc/gemv_mfma.hip) - one weight stream for all rows instead of M dot
 * products per weight chunk.  `workspace` (vlm_gemv_workspace_bytes() bytes, ZERO-INITIALISED once, owned by the caller;
 * launches sharing it must be ordered by one stream) lets projections with few output rows and a long K (o_proj, down)
 * split K over workgroups: fp32 partial tiles + an arrival ticket per tile, summed in a fixed order (deterministic).
 * NULL = no split; shapes that then do not fit fall back to the kernels of vlm_gemv_bf16 (M in {1, 2, 4, 8}).
 * With norm_w these forms take K <= 8192 (K % 128 == 0; past one K segment the RMSNorm runs as one rows launch into the
 * workspace), and past K = 4096 the qkv form takes 8 rows as well as 9..16.  A projection of more than 4096 (row tile, K
 * segment) units - N / 16 tiles times ceil(K / 3072) - is refused (2): the engine cuts such an N into slices of W's rows. */
size_t vlm_gemv_workspace_bytes(void);
int vlm_gemv_bf16_ws(const void* x, const void* W, const void* bias, const void* res, const void* norm_w, void* y, int M, int N,
                     int K, int ldx, int ldw, int ldy, int ldres, float eps, int epilogue, void* workspace, void* stream);
int vlm_gemv_qkv_rope_kvwrite_ws(const void* h, const void* norm_w, float eps, const void* Wqkv, const void* bqkv, void* qkv, int ldq,
                                 int M, int hidden, int Hq, int Hkv, int D, const void* pos, const void* slot,
                                 const void* inv_freq, const void* block_table, int max_pages, void* kpool, void* vpool,
                                 void* workspace, void* stream);
int vlm_gemv_attn_out(const void* part_o, const void* part_ml, int nsplit, const void* Wo, void* h, int ldh, int M,
                      int N, int Hq, int D, void* stream);

/* MLX affine 4-bit weights (group 64): what load_model turns every Linear / Embedding of a 4-bit checkpoint into
 * (utils.py:918-967: nn.quantize with the `<path>.scales in weights` predicate -> nn.QuantizedLinear = mx.quantized_matmul(x,
 * weight, scales, biases, transpose=True, group_size=64, bits=4) (+ bias); nn.QuantizedEmbedding = mx.dequantize of the rows).
 * Engine layout (repacked once at load): Wq uint32 [N][K/8], MLX's own words (element k of a row in word k / 8, bits
 * 4 (k % 8) .. +3); Wsb uint32 [N][K/64] = scale bf16 (low half) | bias bf16 (high half) of each group.  K % 64 == 0.
 * vlm_gemv_w4 / vlm_gemv_w4_qkv_rope_kvwrite: the decode GEMVs of vlm_gemv_bf16 / vlm_gemv_qkv_rope_kvwrite with the
 *   dequantisation fused into the operand path (fp32 affine form per group, no weight is rounded); M in {1,2,4,8};
 *   K <= 30720 (K <= 4096 with norm_w; hidden <= 8192 for the qkv form) and M * K * 2 + 256 bytes of staged rows <= 160 KiB.
 * vlm_dequant_w4: rows of the matrix as bf16 (fp32 scale * q + bias, one rounding): rows == NULL -> rows 0..n_rows-1
 *   (prefill: materialised once per projection, then vlm_gemm_bf16), rows != NULL -> gather (QuantizedEmbedding lookup).
 *   n_table_rows == -1 is the QUANTISE direction, mx.quantize(w, group_size=64, bits=4) as `mlx_vlm.convert -q` runs it
 *   (quant_utils.py:98-104): `out` is then the bf16 SOURCE [n_rows][K] with leading dimension ldo (ldo >= K, ldo % 8 == 0,
 *   16-byte aligned), Wq [n_rows][K/8] and Wsb [n_rows][K/64] are WRITTEN (both contiguous) and `rows` must be NULL
 *   (VLM_ERR_ARG otherwise).  Per group, in fp32 with IEEE division and rint: scale = max((max - min) / 15, 1e-7), signed so
 *   that the edge of larger magnitude lands on an integer (edge = |min| > |max| ? min : max; q0 = rint(edge / scale);
 *   scale = edge / q0 if q0 != 0; bias = edge, or 0 when q0 == 0); q = clip(rint((w - bias) / scale), 0, 15); scale and bias
 *   are rounded to bf16 only when stored.  Non-finite weights are outside the contract (min / max skip a NaN). */
int vlm_gemv_w4(const void* x, const void* Wq, const void* Wsb, const void* bias, const void* res, const void* norm_w, void* y,
                int M, int N, int K, int ldx, int ldy, int ldres, float eps, int epilogue, void* stream);
int vlm_gemv_w4_qkv_rope_kvwrite(const void* h, const void* norm_w, float eps, const void* Wq, const void* Wsb, const void* bqkv,
                                 void* qkv, int ldq, int M, int hidden, int Hq, int Hkv, int D, const void* pos, const void* slot,
                                 const void* inv_freq, const void* block_table, int max_pages, void* kpool, void* vpool,
                                 void* stream);
/* batched decode rows (5..16; 9..16 for the qkv form) over 4-bit weights: the dequant-fused MFMA form of csrc/gemv_mfma.hip -
 * nibbles become bf16 128 + q in the A fragments, every 64-wide group enters the sum as scale * (D - 128 sum_x) + bias * sum_x in
 * fp32 (no weight is rounded); `workspace` as vlm_gemv_bf16_ws.  Other row counts: the kernels of vlm_gemv_w4. */
int vlm_gemv_w4_ws(const void* x, const void* Wq, const void* Wsb, const void* bias, const void* res, const void* norm_w, void* y,
                   int M, int N, int K, int ldx, int ldy, int ldres, float eps, int epilogue, void* workspace, void* stream);
int vlm_gemv_w4_qkv_rope_kvwrite_ws(const void* h, const void* norm_w, float eps, const void* Wq, const void* Wsb, const void* bqkv,
                                    void* qkv, int ldq, int M, int hidden, int Hq, int Hkv, int D, const void* pos, const void* slot,
                                    const void* inv_freq, const void* block_table, int max_pages, void* kpool, void* vpool,
                                    void* workspace, void* stream);
int vlm_dequant_w4(const void* Wq, const void* Wsb, const void* rows, void* out, int n_rows, int K, int ldo, int n_table_rows,
                   void* stream);

/* nn.LayerNorm(eps) -> mx.fast.layer_norm (vision.py:109,180-181). dim % 8 == 0, dim <= 8192 */
int vlm_layernorm(const void* x, const void* w, const void* b, void* y, int rows, int dim, float eps, void* stream);

/* nn.RMSNorm -> mx.fast.rms_norm (language.py:130-133,168) with the residual add of
 * language.py:151-153 fused: h = x + res (res may be NULL), y = rmsnorm(h) * w, h_out = h (may be NULL) */
int vlm_rmsnorm_residual(const void* x, const void* res, const void* w, void* y, void* h_out, int rows, int dim,
                         float eps, void* stream);

/* apply_rotary_pos_emb_vision (vision.py:35-50) in place on q and k of qkv [N][3][H][D];
 * cos_tab / sin_tab fp32 [N][D/2] (cos / sin of VisionModel.rot_pos_emb, vision.py:219-255) */
int vlm_rope2d_vision(void* qkv, const void* cos_tab, const void* sin_tab, int N, int H, int D, int ld, void* stream);

/* M-RoPE (MRoPERotaryEmbedding.apply_rotary, fused-kernel numerics: rope_utils.py:567-651,
 * 1243-1286, selector 519-526) applied in place to the q and k heads of
 * qkv [T][(Hq + 2 Hkv) * D], fused with KVCache.update_and_fetch (cache.py:345-367): the rotated
 * k and the v of token t are written to slot kv_slot[t] of sequence kv_seq[t] (NULL: seq = t) in
 * the paged pools (page = block_table[seq][slot / 64]).  pos_* int32 [T] (t, h, w axes; pass the
 * same pointer three times for text).  sec0 / sec1 = mrope_section[0..1].  kpool == NULL: rope only.
 * K pool [page][Hkv][D/8][64][8], V pool [page][Hkv][D][64 key slots] (bf16; slot order: see csrc/common.hpp
 * vlm_vslot - the k-slot order of the decode P.V MFMA). */
int vlm_mrope_kvwrite(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* pos_t, const void* pos_h,
                      const void* pos_w, const void* inv_freq, int sec0, int sec1, const void* kv_seq,
                      const void* kv_slot, const void* block_table, int max_pages, void* kpool, void* vpool,
                      void* stream);
/* the same with SuScaledRoPE's input scale (rope_utils.py:174-176, Phi-3.5 phi3_v.py:41-48): q and k are multiplied by
 * qk_scale and rounded to bf16 (the reference's typed `scale.astype(x.dtype) * x`) before the rotation; v is not scaled.
 * qk_scale = 1 is vlm_mrope_kvwrite bit for bit. */
/* sec0 < 0 (added within ABI v8): the QK-NORM form of Qwen3-VL (qwen3_vl/language.py:84-89, selector rope_utils.py:511-516).
 * mrope_section = (-sec0, sec1, D / 2 + sec0 - sec1) under the INTERLEAVED selector, and inv_freq points at ONE fp32 table
 * [D / 2 inv_freq | eps | D q_norm_w | D k_norm_w].  Per (row, q or k head): y = T(w * T(x * rsqrt(mean(x^2) + eps))) - the
 * roundings of vlm_rmsnorm_residual - then the fp32 rotation of y and one rounding; q back in place, rotated k and the
 * untouched v into the pools.  D == 128 (VLM_ERR_SHAPE otherwise), qk_scale == 1 (VLM_ERR_ARG otherwise). */
int vlm_mrope_kvwrite_scaled(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* pos_t, const void* pos_h,
                             const void* pos_w, const void* inv_freq, int sec0, int sec1, const void* kv_seq,
                             const void* kv_slot, const void* block_table, int max_pages, void* kpool, void* vpool,
                             float qk_scale, void* stream);

/* The fetch half of KVCache.update_and_fetch (cache.py:345-367 returns keys / values [..., :offset, :]) over the PAGED
 * pools: the cached (rotated) k and v of token t - slot kv_slot[t] of sequence kv_seq[t] (NULL: seq = t) - are copied
 * into the k / v columns of row t of a token-major qkv buffer [T][(Hq + 2 Hkv) * D] (the q columns are left alone).
 * Used when a prompt chunk is prefilled onto a non-empty cache (ar.py:426-472 chunked prefill, dispatch.py:861-882
 * prompt_cache continuation): the chunk attends to [cached tokens | its own]. */
int vlm_kv_gather(void* qkv, int ld, int T, int Hq, int Hkv, int D, const void* kv_seq, const void* kv_slot,
                  const void* block_table, int max_pages, const void* kpool, const void* vpool, void* stream);

/* mx.fast.scaled_dot_product_attention on the prefill path: varlen segments (cu_seqlens int32
 * [nseg+1]), mask=None (vision.py:148-158) or mask="causal" (base.py:214-228,366-373), GQA.
 * q/k/v/out are token-major with the given token strides; head h of token t at ptr + t*stride + h*D.
 * total_qblocks = sum_s ceil(len_s / 128) (host).  D in {64, 80, 128}.
 * causal: bit 0 = causal mask; bit 1 = hint "all segments have the same length" (enables an XCD-local
 * placement of the query blocks of one (segment, head); results are identical with or without it);
 * bit 2 = cu_seqlens is followed by q_start int32 [nseg]: rows of segment s before q_start[s] are KEYS ONLY (the
 * cached prefix of a prompt chunk appended to a non-empty cache, ar.py:426-472 / dispatch.py:861-882 - the causal
 * mask stays on absolute rows, i.e. offset by the cache length as base.py:366-373 builds it); their rows of `out`
 * are not written and total_qblocks = sum_s ceil((len_s - q_start_s) / 128).  Not with bit 1.
 * Added within ABI v8: bit 3 = the ONE-TILE form (csrc/attn_window.hip; the window blocks of the Qwen2.5-VL tower,
 * qwen2_5_vl/vision.py:149-163): every segment has 1..64 tokens, so its K and V are one tile and the softmax is a single exact
 * pass; two (segment, head) pairs per workgroup.  `total_qblocks` then carries the caller's DECLARED longest segment.
 * VLM_ERR_SHAPE with nothing enqueued when D != 80, Hq != Hkv or that maximum exceeds 64; not with bits 0 / 2 (VLM_ERR_ARG);
 * bit 1 is accepted and has no effect.  Of a segment longer than declared only the first 64 tokens are read and written. */
int vlm_attn_prefill(const void* q, const void* k, const void* v, void* out, int q_stride, int k_stride, int v_stride,
                     int o_stride, const void* cu_seqlens, int nseg, int total_qblocks, int Hq, int Hkv, int D,
                     float scale, int causal, void* stream);

/* the same op at L == 1 over the paged cache (base.py:366-373 from language.py:115-118).
 * q [B][Hq*D] (row stride ldq); kv_len int32 [B] (+ kv_len_add) keys per sequence;
 * part_o fp32 [B][Hq][nsplit][D], part_ml fp32 [B][Hq][nsplit][2] receive the per-split partials; out [B][Hq*D]
 * (bf16) gets the merged result, or pass out == NULL and merge in vlm_gemv_attn_out.  D == 128.
 * block_table == NULL: identity layout - sequence b owns pages [b * max_pages, (b + 1) * max_pages) of the pools as
 * passed, page numbers are computed instead of loaded (one dependent memory round trip less). */
int vlm_attn_decode_paged(const void* q, int ldq, const void* kpool, const void* vpool, const void* block_table,
                          int max_pages, const void* kv_len, int kv_len_add, int B, int Hq, int Hkv, int D,
                          float scale, int nsplit, void* part_o, void* part_ml, void* out, int ldo, void* stream);

/* The same op (base.py:366-373 at L == 1) in its page-split form, the one the decode engine uses for up to 64
 * (sequence, kv head) pairs: nsplit one-wave workgroups per (sequence, kv head), workgroup s walks pages s, s + nsplit,
 * ... - one 64-token page (32 KB of K + V) is the whole load of a compute unit, so a context is pulled through
 * min(pages, nsplit) CUs per kv head instead of one - and the LAST workgroup to arrive (one agent-scope ticket per
 * (sequence, kv head)) merges the partials and writes out [B][Hq*D] (bf16): one launch, no merge pass, no merge in the
 * o_proj prologue.  part_o fp32 [B*Hkv][nsplit][Hq/Hkv][D] and part_ml fp32 [B*Hkv][nsplit][Hq/Hkv][2] are scratch
 * (same sizes as vlm_attn_decode_paged's); tickets: uint32 [B*Hkv], ZERO before the first launch - every launch leaves
 * it zero again.  Launches that share part_o / part_ml / tickets must be stream-ordered. */
/* out == NULL: the partial-only form.  Nothing is merged and no ticket is taken (tickets may be NULL): every split s
 * of every head writes (m, l) - m in the log2 domain, (-inf, 0) for a split with no page - to part_ml fp32
 * [B][Hq][nsplit][2] and, when it has pages, its unnormalised O as fp32 to part_o [B][Hq][nsplit][D] (ABI v8; bf16 before -
 * a rounding point the reference's fused attention does not have); the launch ends at those (plain) stores and
 * vlm_gemv_attn_out_bf16 merges them in the o_proj prologue.
 * The pitch of part_ml (added within ABI v8, the partial-only form alone): nsplit may carry P << 16, P >= nsplit - part_ml is
 * then [B][Hq][P][2] and the pairs nsplit .. P - 1 of a head are never written.  With P even a head's pairs start on 16 bytes,
 * which is what the exact-split forms of vlm_gemv_attn_out_bf16 read; P = 0 (every caller before): P = nsplit.  part_o keeps
 * the pitch nsplit. */
int vlm_attn_decode_paged_split(const void* q, int ldq, const void* kpool, const void* vpool, const void* block_table,
                                int max_pages, const void* kv_len, int kv_len_add, int B, int Hq, int Hkv, int D,
                                float scale, int nsplit, void* part_o, void* part_ml, void* tickets, void* out, int ldo,
                                void* stream);

/* Uniform 8-bit KV cache: QuantizedKVCache (cache.py:233-334, mx.quantize bits = 8, group_size = 64 over the head
 * dimension), KVCache.to_quantized (cache.py:415-423) and quantized_scaled_dot_product_attention at L == 1
 * (base.py:260-302).  8-bit pools per layer, same pages / block table as the bf16 pools:
 *   kpool8 u8 [page][Hkv][D/8][64 keys][8], vpool8 u8 [page][Hkv][D][64 key slots] (the bf16 layouts with 1-byte elements),
 *   ksb / vsb uint32 [page][Hkv][64 keys][D/64]: (scale bf16 | bias bf16 << 16) of key k, group j at word k * (D/64) + j.
 * layer_stride: ELEMENTS between consecutive layers' pools, identical for the bf16 and the u8 pools (the sb pools advance
 * by layer_stride / (D/2) words).  D == 128.
 * vlm_kv_quantize_tokens: token i of the list (slot kv_slot[i] of sequence kv_seq[i]; kv_seq NULL: row i) is quantised from
 *   the bf16 pools into the 8-bit pools, all n_layers layers - to_quantized over a range of cached tokens.
 * vlm_attn_decode_paged_q8: the page-split decode attention (vlm_attn_decode_paged_split: same nsplit / part_o / part_ml /
 *   tickets / out conventions, out == NULL = partial-only form) over the 8-bit pools; quantize_new != 0: the step's new
 *   token (slot kv_len - 1, already written to the bf16 pools by the qkv epilogue) is quantised first -
 *   QuantizedKVCache.update_and_fetch - by the workgroup that owns its page.  In the merging form (out != NULL) a step of
 *   128 or more (row, kv head) pairs with nsplit <= 16 runs half-page units: part_o / part_ml must then hold 2 * nsplit
 *   splits per (row, head). */
int vlm_kv_quantize_tokens(const void* kpool, const void* vpool, void* kpool8, void* vpool8, void* ksb, void* vsb,
                           size_t layer_stride, int n_layers, const void* kv_seq, const void* kv_slot, int T,
                           const void* block_table, int max_pages, int Hkv, int D, void* stream);
int vlm_attn_decode_paged_q8(const void* q, int ldq, const void* kpool16, const void* vpool16, void* kpool8, void* vpool8,
                             void* ksb, void* vsb, const void* block_table, int max_pages, const void* kv_len,
                             int kv_len_add, int B, int Hq, int Hkv, int D, float scale, int nsplit, void* part_o,
                             void* part_ml, void* tickets, void* out, int ldo, int quantize_new, void* stream);

/* The same op at L > 1: a prompt CHUNK appended to a cache that is already 8-bit (QuantizedKVCache.update_and_fetch with an
 * update of any length, cache.py:233-334, then quantized_scaled_dot_product_attention under the causal mask offset by the
 * cache length, base.py:260-302 behind base.py:305-373).  Causal, varlen, GQA; keys and values are read straight from the
 * 8-bit pools (the layouts above) through the block table - no vlm_kv_gather, no bf16 copy of the prefix.
 * q / out: token-major bf16 rows of the chunk(s) only, head h of row t at ptr + t * ld + h * D; q is already rotated.
 * Segment s = query rows cu_q[s] .. cu_q[s + 1] - 1 (int32 [nseg + 1]) of the sequence in block-table row seg_seq[s]
 * (int32 [nseg]); its row r sits at absolute position q_start[s] + r (int32 [nseg]: tokens cached before the chunk) and sees
 * slots 0 .. q_start[s] + r.  All of those must be 8-bit at the launch: the caller quantises the chunk's own tokens first
 * (vlm_kv_quantize_tokens).  Later slots, stale bytes behind a trim and pages the table does not name never reach a result.
 * total_qblocks = sum_s ceil(rows_s / 64) (host).  D == 128; arithmetic as vlm_attn_decode_paged_q8 (bf16(scale), q * scale
 * and every score rounded to bf16, softmax in fp32, unnormalised probabilities rounded to bf16).
 * The bf16 form: ksb == NULL && vsb == NULL (both; one NULL alone is VLM_ERR_ARG).  kpool8 / vpool8 are then the BF16 pools
 * (K [page][Hkv][D/8][64][8], V [page][Hkv][D][64 key slots]) and nothing is quantised: the chunk's own K / V must be in the
 * pages (vlm_mrope_kvwrite).  Same segments, same masking; arithmetic of the bf16 kernels at D == 128 (fp32 scores and
 * softmax, P fed as the hi + lo bf16 pair).  It is the attention of a warm prefix-cache admission (mlx-vlm_amd/apc.py). */
int vlm_attn_prefill_paged_q8(const void* q, int ldq, void* out, int ldo, const void* kpool8, const void* vpool8,
                              const void* ksb, const void* vsb, const void* block_table, int max_pages, const void* seg_seq,
                              const void* cu_q, const void* q_start, int nseg, int total_qblocks, int Hq, int Hkv, int D,
                              float scale, void* stream);

/* h[0][0:N] += merge(partials of vlm_attn_decode_paged_split's partial-only form) Wo^T for ONE decode row
 * (language.py:115-120,151): every thread of the o_proj GEMV loads one 8-element chunk of all nsplit <= 16 fp32 partials
 * and their (m, l) ahead of its weight stream and merges them in registers (bf16 Wo: the name).  Hq * D <= 2048.
 * nsplit may carry the pitch P << 16 of part_ml as vlm_attn_decode_paged_split wrote it (0: P = nsplit, P <= 16); a P other
 * than nsplit needs the exact-split forms (VLM_TUNE_GEMV_VARIANT bit 12, P even, part_ml on 16 bytes) - VLM_ERR_SHAPE otherwise. */
int vlm_gemv_attn_out_bf16(const void* part_o, const void* part_ml, int nsplit, const void* Wo, void* h, int ldh, int N,
                           int Hq, int D, void* stream);

/* nn.Embedding (language.py:164,179): out[t] = table[ids[t]] */
int vlm_embed_gather(const void* ids, const void* table, void* out, int T, int D, int ldo, int vocab, void* stream);

/* Model.merge_input_ids_with_image_features (qwen2_vl.py:78-148): dst[dst_rows[i]] = src[i] */
/* n < 0 (added within ABI v8): the ADD form over -n rows, dst[dst_rows[i]] = T(dst[dst_rows[i]] + src[i]) - DeepStack's
 * h[visual rows] += deepstack_visual_embeds[layer] (qwen3_vl/language.py:231-283); the rows must be distinct */
int vlm_scatter_image_rows(const void* src, const void* dst_rows, void* dst, int n, int D, int ld_src, int ld_dst,
                           void* stream);

/* pixel_values.astype(bf16) (qwen2_vl.py:44-45) with zero padding of the row to ld_dst
 *
 * ld_src == -1 (added within ABI v8): image mode - the rows are not cast from fp32 but MADE on the device from a raw u8 RGB
 * image, i.e. the operation replaces the image processor's resize + rescale + normalise + patch shuffle
 * (mlx_vlm/models/qwen3_vl/processing_qwen3_vl.py:302-354) together with the cast.  `src` is then a HOST pointer to the
 * struct below; `dst` = bf16 [rows][ld_dst], `cols` = 3 * temporal * patch * patch (VLM_ERR_SHAPE otherwise), ld_dst >= cols,
 * ld_dst % 8 == 0, dst 16-byte aligned (VLM_ERR_ARG otherwise), and rows row_offset .. row_offset + (rh / patch) * (rw / patch) - 1 of dst are written, all ld_dst
 * columns of each, the ones from `cols` on as zeros; `rows` is what dst holds (VLM_ERR_ARG when the image does not fit).
 * Launches: [horizontal pass] [vertical pass] patchify.  A pass is Pillow's 8-bit resampler (ImagingResampleHorizontal_8bpc /
 * Vertical_8bpc of src/libImaging/Resample.c): out = clip8((2^21 + sum_i px[first + i] * coeffs[i]) >> 22), int32, arithmetic
 * shift; horizontal first, rounded to u8, then vertical.  Its tables come from the host (Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc): coeffs int32 [out][ksize], bounds int32 [out][2] = (first source index, taps <= ksize).  A NULL
 * coeffs pointer skips the pass, and the size along that axis must then be unchanged (VLM_ERR_SHAPE).  Source indices are
 * clamped into the image and tap counts into ksize: a bad table gives a wrong picture, not a fault.
 * patch == 0: the passes only - `frame` is the product; dst, rows, cols and ld_dst are ignored.
 * Bad arguments return 1 or 2 and enqueue nothing. */
typedef struct vlm_image_patch_args {
  const void* src;        /* u8 [height][width][3], rows src_stride BYTES apart (>= 3 * width) */
  int height, width;
  long long src_stride;
  int resized_height, resized_width; /* rh, rw: multiples of patch * merge unless patch == 0 */
  const void* coeffs_h;   /* horizontal pass, width -> rw: int32 [rw][ksize_h]; NULL = skipped */
  const void* bounds_h;   /* int32 [rw][2] */
  int ksize_h;
  const void* coeffs_v;   /* vertical pass, height -> rh: int32 [rh][ksize_v]; NULL = skipped */
  const void* bounds_v;   /* int32 [rh][2] */
  int ksize_v;
  void* tmp_h;            /* u8 [height][rw][3]: the horizontal result; needed when BOTH passes run */
  void* frame;            /* u8 [rh][rw][3]: the resized frame; needed when a pass runs */
  const void* lut;        /* bf16 [3][256]: rescale + normalise of (channel, byte) */
  int patch, merge, temporal; /* patch_size, spatial merge_size, temporal_patch_size (every temporal copy is written) */
  int row_offset;         /* first row of dst this image writes: several images of one call share one matrix */
} vlm_image_patch_args;
int vlm_cast_f32_bf16_pad(const void* src, void* dst, int rows, int cols, int ld_src, int ld_dst, void* stream);

/* decode-loop bookkeeping kept on the device (cache.py:362 offset += 1; language.py:476-509
 * pos = offset + rope_delta): ctx[b]++, pos[b]++, out_ring[step % ring_len][b] = tok[b], step++ */
int vlm_decode_advance(void* ctx, void* pos, const void* tok, void* out_ring, int ring_len, void* step, int B,
                       void* stream);

/* ar.py:368 logprobs = logits - logsumexp (bf16) -> logprobs [B][V] (may be NULL when greedy);
 * temperature == 0: argmax, lowest index on ties (sample_utils.py:63-64);
 * else top_p (289-318) -> min_p (266-286) -> top_k (169-175) -> categorical(logprobs/temp) (385-387)
 * by Gumbel-max with a counter-hash RNG keyed by (seed, *step_ptr, row, index).
 * scratch bf16 [B][ldlp] is required when temperature > 0.
 * workspace: vlm_sample_workspace_bytes(B) bytes, zero-filled ONCE at allocation and then owned by the sampler: an arrival
 * ticket, the per-block argmax partials, a 65 536-bin key histogram per row (every call leaves it all-zero again) and 128
 * control words per row for the top-p path that is split over several workgroups (crossing key, per-slice counts, the
 * populated key range - re-armed by the last launch of a call; the first call after the zero fill sees range [0, kmax],
 * takes the unwindowed route and gives the same row).  One workspace serves one stream at a time. */
size_t vlm_sample_workspace_bytes(int B);
int vlm_sample(const void* logits, int ld, int B, int V, void* logprobs, void* scratch, int ldlp, void* tok,
               void* workspace, float temperature, float top_p, float min_p, int top_k, unsigned seed,
               const void* step_ptr, void* stream);

/* The whole sampler surface of make_sampler (sample_utils.py:10-89), filters in its order: top_n_sigma (181-212) -> p_less
 * (215-236) -> typical_p (321-345) -> top_p (289-318) -> min_p with min_tokens_to_keep (239-286) -> xtc (348-376) -> top_k
 * (169-175) -> categorical(logprobs / temp) (385-387).  The python scalars arrive as doubles and are converted the way MLX's
 * weak typing converts them (double -> float32 -> the log-probs' dtype) before they meet the bf16 log-probs; every
 * elementary op of the typed graph rounds to bf16 (pinned by tests/golden/samplers_ref.npz).  A filter is off at the value
 * make_sampler treats as off: top_p outside (0, 1), min_p == 0, top_k <= 0, top_n_sigma == 0, p_less == 0, typical_p outside
 * (0, 1), xtc_probability == 0.  After the call `scratch` holds the filtered log-probs (-inf = removed) when at least one filter
 * is on; with none the draw reads the log-probs themselves.  Launches: logsumexp partials, log-probs, [filters: one workgroup
 * per row], the Gumbel-max partials (64 workgroups per row), the final pick.
 * typical_p needs sort_workspace (device, vlm_sample_sort_workspace_bytes(B, V)).  xtc: B == 1 only (the reference's minimum
 * runs over the whole array and its draw is one scalar per call) -> VLM_ERR_SHAPE otherwise; the draw is the counter hash at
 * (seed, *step_ptr, row, 0xFFFFFFFF); xtc_special_tokens = device int32 [n_xtc_special <= 256].
 *
 * input_is_logprobs == 2 (added within ABI v8): top_logprobs mode - nothing is sampled.  `logits` = bf16 log-prob rows [B][ld]
 * (ld >= V; what lies past V is never read, the rows are left untouched), top_k = K with 1 <= K <= min(64, V) (VLM_ERR_SHAPE
 * otherwise), `tok` = int32 [B][K] out, `logprobs` = bf16 [B][K] out: the K best entries of every row as the reference's batch
 * generator lists them (ar.py:1092-1122, argsort ascending, last K, reversed): value descending and, among equal values, the
 * HIGHER index first; +0.0 and -0.0 are equal values; the value written is the row's own bits at that index.  NaN is outside the
 * contract.  Every other field, `scratch`, `ldlp`, `workspace` and `step_ptr` are ignored (workspace may be NULL and is not
 * touched).  One launch, one workgroup per row. */
/* input_is_logprobs bit 2 = VLM_SAMPLE_ROW_TABLE (added within ABI v8; combinable with 1 = "log-probs in", which then holds for
 * every row): ROW-TABLE mode - every row is drawn with its OWN sampler.  Every scalar field of the block is then ignored (a
 * filter outside the three below switched on - typical_p, top_n_sigma, p_less, xtc_probability - is VLM_ERR_ARG), `step_ptr` is
 * ignored, `scratch` is required, and row b reads its LINE of eight 32-bit words from the workspace the caller already owns:
 *     word VLM_SAMPLE_ROW_LINE_WORD + b * VLM_SAMPLE_ROW_STRIDE_WORDS of the workspace (as uint32 [])
 *     = {temperature f32, top_p f32, min_p f32, top_k i32, seed u32, count u32, T(1 - top_p) f32, T(log(min_p)) f32}
 * - eight control words of the row's own workspace block that no other mode reads or writes, at the same place whatever the
 * call's B (a step over the first B' < B rows of a state finds the same words) and inside vlm_sample_workspace_bytes(B) as it
 * always was.  The last two words are the two scalar conversions of the scalar path made by whoever writes the line:
 * (float) of the double 1 - top_p, resp. of the double log(min_p), rounded to bf16 (nearest even) and stored as f32.
 * temperature == 0 - an all-zero line, what a workspace zero-filled by a caller that never heard of the mode holds - is a GREEDY
 * row: argmax of the row's log-probs, lowest index on ties, no filter, no noise.  Otherwise top_p -> min_p (min_tokens_to_keep
 * = 1) -> top_k -> categorical(logprobs / temperature), each filter off at the values that switch it off above (top_p outside
 * (0, 1), min_p == 0, top_k <= 0 or >= V), the draw keyed (seed, count, 0, index): the row index does not enter, so a request's
 * draws depend on its own line alone.  The call's last launch does count += 1 on every row; the host writes count = 0 when a
 * request takes the row.  Row b gives the token, the log-prob row and (a filter on) the filtered scratch row of the scalar call
 * on that row alone (B = 1) with the line's scalars, seed and *step_ptr = count, bit for bit (tests/test_row_sampler_gpu.py).
 * The launches depend on (B, V, leading dimensions, alignment) only, never on the lines: lse partials, [log-probs], then the split
 * chain (histogram, crossing, count, mask + draw) where V % 8 == 0, V >= 8192 and the rows are 16-byte aligned, else the
 * one-workgroup filter and the Gumbel partials, then the pick - a captured call replays over any table.  scratch is written for
 * every row (an unfiltered copy where the row has no filter). */
#define VLM_SAMPLE_ROW_TABLE 4
#define VLM_SAMPLE_ROW_STRIDE_WORDS 65920 /* 32-bit words from one row's workspace block to the next */
#define VLM_SAMPLE_ROW_LINE_WORD 65928    /* 32-bit word of the workspace where row 0's line starts (32-byte aligned) */
typedef struct vlm_sampler_params {
  double temperature, top_p, min_p;
  int min_tokens_to_keep, top_k;
  double top_n_sigma;
  int p_less;
  double typical_p, xtc_probability, xtc_threshold;
  const void* xtc_special_tokens;
  int n_xtc_special;
  void* sort_workspace;
  unsigned seed;
  int input_is_logprobs; /* temperature > 0: `logits` already holds log-probs (what the reference hands a sampler closure,
                            ar.py:368-379): no logsumexp pass, `logprobs` may be NULL.  2: top_logprobs mode, see above.
                            bit 2 (VLM_SAMPLE_ROW_TABLE, | 1 allowed): row-table mode, see above */
} vlm_sampler_params;
size_t vlm_sample_sort_workspace_bytes(int B, int V);
int vlm_sample_ex(const void* logits, int ld, int B, int V, void* logprobs, void* scratch, int ldlp, void* tok, void* workspace,
                  const vlm_sampler_params* p, const void* step_ptr, void* stream);

/* Logits processors of generate_step (make_logits_processors, sample_utils.py:92-146, applied at ar.py:360-364) as ONE
 * device pass over the logits row(s), in the reference's order: logit_bias (129-134) -> repetition penalty (390-422:
 * x < 0 ? x * p : x / p, once per distinct token of the last rep_ctx fed tokens) -> presence penalty (425-450: - p once
 * per distinct token) -> frequency penalty (453-475: - p per occurrence).  Every step rounds to bf16 as the reference's
 * typed graph does (python-float penalties are rounded to bf16 first).
 * The history of fed tokens (prompt + every token fed back) lives on the device so the step stays graph-replayable:
 * hist int32 [B][hist_cap] ring, hist_len int32 [B] tokens pushed so far.  push_tok != NULL: push_tok[b] is appended to
 * row b's history FIRST (the decode step feeds tok[b]; the reference appends y before the processors run).
 * A penalty of 0 / a context of 0 switches that processor off.  Contexts <= hist_cap <= 1024. */
typedef struct vlm_penalty_args {
  void* hist;
  void* hist_len;
  int hist_cap;
  float rep_penalty;
  int rep_ctx;
  float pres_penalty;
  int pres_ctx;
  float freq_penalty;
  int freq_ctx;
  const void* bias_idx; /* int32 [n_bias] (distinct) */
  const void* bias_val; /* fp32 [n_bias] */
  int n_bias;
  /* per-request processors of a continuous batch (BatchGenerator.insert(..., logits_processors=), ar.py:2584-2606):
   * row_params != NULL: fp32 [B][8] on the device = {rep_penalty, rep_ctx, pres_penalty, pres_ctx, freq_penalty, freq_ctx,
   * n_bias, W} of row b - the scalar fields above are then ignored - and row b's bias list sits at bias_idx / bias_val +
   * b * bias_stride.  The host rewrites the table as requests join and leave; a captured step keeps its arguments.
   * W (slot 7; 0 = none, what every caller passed before it had a meaning): row b carries a TOKEN BITMASK of W 32-bit words
   * (constrained decoding, reference structured.py:7-36), stored in the LAST W int32 of its bias_idx row: bias_idx +
   * b * bias_stride + (bias_stride - W); the caller keeps n_bias + W <= bias_stride.  Token t stays iff t < 32 * W and bit
   * (t & 31) of word (t >> 5) is set; every other logit of the row becomes bf16 -inf (0xFF80) - tokens past the mask
   * included: a tokenizer's vocabulary is usually shorter than the logits row.  Applied after the row's bias and penalties,
   * by a launch of its own over (vocabulary chunks, rows).  An all-zero mask leaves no token: the host refuses it. */
  const void* row_params;
  int bias_stride;
} vlm_penalty_args;
int vlm_apply_logit_penalties(void* logits, int ld, int B, int V, const void* push_tok, const vlm_penalty_args* p,
                              void* stream);

/* The greedy tail of a decode step in two launches instead of five: vlm_sample at temperature 0 (ar.py:368 logprobs,
 * sample_utils.py:63-64 argmax) + vlm_decode_advance (cache.py:362, language.py:476-509) + the NEXT step's
 * vlm_embed_gather (language.py:164,179): h[b] = embed[tok[b]] (row stride ldh).  workspace: vlm_sample_workspace_bytes,
 * zero-filled once at allocation (its first word is an arrival ticket the kernel re-arms). */
int vlm_sample_greedy_advance(const void* logits, int ld, int B, int V, void* logprobs, int ldlp, void* tok,
                              void* workspace, void* ctx, void* pos, void* out_ring, int ring_len, void* step,
                              const void* embed, void* h, int D, int ldh, void* stream);

/* ------------------------------------------------------------------------------------------
 * Model-level engine: the layer loops of Qwen2Model / VisionModel run natively so that a decode
 * step is ~150 back-to-back launches with no host code in between and can be captured in a
 * hipGraph (the reference keeps the loop in Python and relies on MLX's lazy graph + async_eval,
 * mlx_vlm/generate/ar.py:474-508).
 * ------------------------------------------------------------------------------------------ */
typedef struct vlm_llm_config {
  int hidden /* <= 8192; a multiple of 128 above 4096 (vlm_llm_create returns 2 otherwise, before anything is allocated) */,
      n_layers, inter, n_heads, n_kv_heads, head_dim, vocab;
  float rms_eps;
  int mrope_sec0, mrope_sec1; /* mrope_section[0], [1] */
  float attn_scale;           /* softmax scale of the attention; 0 = head_dim ** -0.5.  Set when the engine's head_dim is a
                                 zero-padded form of the model's (e.g. 64 -> 128, llava_bunny language.py:24-25) */
  float rope_qk_scale;        /* ABI v3.  SuScaledRoPE (rope_utils.py:96-189): q and k are multiplied by this and rounded to
                                 bf16 before the rotation, in the prefill pass and in every decode qkv epilogue; 0 = 1 = none */
  int rope_long_from;         /* ABI v4.  SuScaledRoPE's short / long factor regimes: > 0 = original_max_position_embeddings and
                                 vlm_llm_globals.inv_freq holds TWO tables [2][head_dim / 2] (short factors, then long).  A decode
                                 step picks the long table for every row when ANY row's cache offset >= this value - the
                                 reference's per-call rule position_end = max(offset) + 1 > original_max (rope_utils.py:168-172)
                                 evaluated inside the qkv epilogue, so captured steps cross the limit without host help and a
                                 continuous batch behaves as the reference's batched call; a prefill call names its regime in
                                 vlm_prefill_args.rope_long.  0 = one table */
} vlm_llm_config;

typedef struct vlm_llm_layer {
  const void *ln1_w, *wqkv, *bqkv, *wo, *ln2_w, *wgu /* interleaved gate/up rows */, *wdown;
  /* MLX affine 4-bit layers (vlm_gemv_w4): a non-NULL *_sb marks the matching w* as q words uint32 [N][K/8] with *_sb its
   * (scale | bias << 16) words uint32 [N][K/64]; NULL = bf16 weight as before.  Rows packed / interleaved the same way. */
  const void *wqkv_sb, *wo_sb, *wgu_sb, *wdown_sb;
  /* Added within ABI v8, APPENDED: read only by a handle in VLM_MODE_QWEN3 (set BEFORE vlm_llm_set_layer, which otherwise copies
   * the struct up to wdown_sb - a caller of the earlier form may keep passing it that long).  q_norm / k_norm of Qwen3's
   * attention (qwen3_vl/language.py:84-89): fp32 [head_dim] each, the checkpoint's weights widened (exact); bqkv is NULL there */
  const void *q_norm_w, *k_norm_w;
} vlm_llm_layer;

typedef struct vlm_llm_globals {
  const void *embed, *final_norm_w, *lm_head /* == embed when tied */, *inv_freq /* fp32 [head_dim/2] */;
  const void *embed_sb, *lm_head_sb; /* 4-bit embedding table / head (nn.QuantizedEmbedding, as_linear): see vlm_llm_layer */
} vlm_llm_globals;

typedef struct vlm_kv_pool {
  void *kpool, *vpool;      /* layer 0 base */
  size_t layer_stride;      /* elements between consecutive layers' pools */
  const void* block_table;  /* int32 [n_seq][max_pages]; NULL for decode over an identity-layout pool */
  int max_pages;
  /* ABI v4: the 8-bit pools of the uniform quantized KV cache (vlm_attn_decode_paged_q8), layer 0 base, NULL = none.
   * When set, every decode step attends over them (the qkv epilogue still writes the new token to the bf16 pools; the
   * attention launch quantises it). */
  void *kpool8, *vpool8, *ksb, *vsb;
  /* ABI v5: 1 = the LAST layer of a stack deeper than 2 keeps attending over the bf16 pools - the reference's policy for
   * BATCHED generation with kv_bits (models/cache.py:8-21 should_quantize_kv_layer, generate/ar.py:842-858); 0 = every
   * layer attends over the 8-bit pools (generate_step's maybe_quantize_kv_cache, generate/common.py:170-181). */
  int q8_skip_last;
} vlm_kv_pool;

/* max_kv_size (RotatingKVCache, models/cache.py:442-625; make_prompt_cache cache.py:45-70 builds it with keep = 4): entry i
 * moves the cached token of sequence seq[i] at slot src_slot[i] to slot dst_slot[i] in EVERY layer (bf16 pools).  The source
 * and destination SETS of one call must be disjoint.  The host keeps the ring (which slot holds which token); the engine's
 * rule stays "write at slot = entries held, attend over entries held + 1" (csrc/kv_rotate.hip).  int32 device arrays [T]. */
int vlm_kv_move_tokens(void* kpool, void* vpool, size_t layer_stride, int n_layers, const void* seq, const void* src_slot,
                       const void* dst_slot, int T, const void* block_table, int max_pages, int Hkv, int D, void* stream);

/* KVCache.update_and_fetch (models/cache.py:345-367; BatchKVCache.update_and_fetch cache.py:1002-1025 calls it per row): the S
 * tokens of `keys` / `values` - bf16 [Hkv][S][D] views, strides in ELEMENTS (multiples of 8 for the keys, whose rows are read
 * as 16-byte pieces; base 16-byte aligned) - become the cached tokens slot0 .. slot0 + S - 1 of sequence `seq` in ONE layer:
 * kpool_layer / vpool_layer = that layer's pools (vlm_kv_pool.kpool + layer * layer_stride elements).  block_table NULL =
 * identity layout (page = seq * max_pages + index).  The pages must already belong to the sequence. */
int vlm_kv_append_tokens(void* kpool_layer, void* vpool_layer, const void* keys, const void* values, int S, long k_head_stride,
                         long k_tok_stride, long v_head_stride, long v_tok_stride, int seq, int slot0, const void* block_table,
                         int max_pages, int Hkv, int D, void* stream);

/* prefill over T tokens (all sequences concatenated).  h [T][hidden] holds the input
 * embeddings and is the residual stream (overwritten).  Workspaces are caller-owned:
 * xn [T][hidden], qkv [T][(Hq+2Hkv)*D], attn [T][Hq*D], act [T][inter].
 * last_rows int32 [n_last]: rows of h whose logits are wanted (the reference computes all L rows
 * and keeps [:, -1], ar.py:358); logits [n_last][vocab]; xlast [n_last][hidden] workspace. */
typedef struct vlm_prefill_args {
  void* h;
  int T;
  const void *pos_t, *pos_h, *pos_w; /* int32 [T] */
  const void *kv_seq, *kv_slot;      /* int32 [T] */
  const void* cu_seqlens;            /* int32 [nseg+1] */
  int nseg, total_qblocks;
  void *xn, *qkv, *attn, *act;
  const void* last_rows;
  int n_last;
  void *xlast, *logits;
  int rope_long; /* models with rope_long_from > 0: 1 = this call uses the LONG frequency table (the caller applies
                    SuScaledRoPE's per-call rule: max cache offset + tokens of the call > original_max) */
  /* Added within ABI v8, APPENDED: read only by a handle in VLM_MODE_QWEN3 - a caller of the earlier form may keep passing the
   * struct up to rope_long.  DeepStack (qwen3_vl/language.py:231-283): after decoder layer i < n_ds, h[ds_rows[j]] +=
   * ds_embeds[i][j] (one typed bf16 add per element) for j < n_ds_rows.  ds_embeds bf16 [n_ds][n_ds_rows][hidden], ds_rows int32
   * [n_ds_rows], distinct rows of h (the image-token rows of THIS call: a chunked prefill passes the slice of its chunk).
   * ds_embeds == NULL or n_ds_rows == 0: none */
  const void *ds_embeds, *ds_rows;
  int n_ds, n_ds_rows;
} vlm_prefill_args;

/* one decode step for B sequences (B in {1,2,4,8}); every buffer is device resident so the
 * step can be replayed from a graph: tok int32 [B] (in: token to feed, out: sampled token),
 * pos / ctx int32 [B] (rope position / keys in cache, advanced by the step; int32 [2][B] under
 * VLM_DECODE_WINDOW, see the flag), step int32 [1]. */
typedef struct vlm_decode_args {
  int B;
  void *tok, *pos, *ctx, *step;
  void *h, *qkv, *attn, *act, *logits, *logprobs, *scratch;
  void *part_o, *part_ml, *sample_ws;
  void* out_ring; /* int32 [ring_len][B] sampled-token history (may be NULL) */
  int ring_len, nsplit;
  float temperature, top_p, min_p;
  int top_k;
  unsigned seed;
  int flags; /* VLM_DECODE_* */
  const vlm_penalty_args* penalties; /* NULL: none.  Applied to the step's logits before sampling; the fed token is
                                        pushed to the history first (vlm_apply_logit_penalties). (host pointer, copied) */
} vlm_decode_args;

/* vlm_decode_args.flags */
#define VLM_DECODE_FUSED_TAIL 1 /* the step does not start with the embedding gather - h already holds embed[tok] (the
                                   caller gathers it once after the prefill, vlm_embed_gather) and the sampler tail leaves
                                   the next step's h behind: vlm_sample_greedy_advance at temperature 0; with a temperature
                                   the sampler's last launch (final pick) also does vlm_decode_advance and the gather.
                                   bf16 embedding tables only.  The host must not rewrite tok between steps. */
#define VLM_DECODE_ACT16 2      /* `act` holds 16 x intermediate_size elements (not B x): a step of 5..16 rows over bf16 weights
                                   may then hand the SwiGLU output to the down projection in the tiled layout of
                                   VLM_EPI_Y_TILED / VLM_EPI_X_TILED (rows padded to the MFMA tile's 16).  ABI v8. */
#define VLM_DECODE_WINDOW 4     /* max_kv_size on the device (RotatingKVCache, models/cache.py:442-625): the rows' caches are rings
                                   of VLM_MODE_WINDOW_SIZE slots whose first VLM_MODE_WINDOW_KEEP are never overwritten.  ctx and
                                   pos then point at int32 [2][B]: ctx row 0 = n (entries held before the step's write), row 1 = w
                                   (the slot the step writes); pos row 0 = p (rope position of the step), row 1 = d (the row's
                                   rope delta).  The step writes K / V at slot w, attends over n + 1 entries (the rotation is
                                   baked into the keys: slot order does not matter) and its tail advances
                                     n' = min(n + 1, M - 1),  w' = w + 1 == M ? K : w + 1,
                                     p' = VLM_MODE_WINDOW_RING_POS ? (r >= M ? K : r) + 1 + d  with r = p - d  :  p + 1.
                                   B in {1, 2, 4, 8}, bf16 pools (8-bit pools: argument error), one rope table
                                   (vlm_llm_config.rope_long_from > 0: argument error - that epilogue reads ctx as the offset).
                                   A bit added within ABI v8: callers that pass [B] arrays never set it. */
#define VLM_DECODE_HOST_RING 8  /* out_ring is host-visible pinned memory (hipHostMalloc; the pointer as the device sees it): the
                                   step's tail writes its ring entry with a system-scope vector store, so the host reads slot
                                   step % ring_len once the step has completed (an event behind it) and no device-to-host copy is
                                   enqueued between two steps.  The host must have read a slot before the step ring_len later is
                                   enqueued.  Same tokens; part of the graph key like every flag.  A bit added within ABI v8. */
#define VLM_DECODE_SPLITS_SHIFT 4 /* bits 4, 5 (added within ABI v8): c = (flags >> 4) & 3.  c > 0: a ONE-row step whose page-split
                                   attention is merged in the o_proj prologue (VLM_TUNE_ATTN_MERGE) runs both launches over
                                   4 c splits instead of VLM_TUNE_ATTN_PAGESPLIT.  The caller promises ctx + 1 <= 256 c for
                                   every replay: each split then owns at most one page, as under 16 splits, and the step gives
                                   the same bytes (a longer context is still attended over in full - other bits).  Ignored by
                                   every other step (more rows, 8-bit pools, a window, VLM_TUNE_ATTN_MERGE 0). */
#define VLM_DECODE_SPLITS_MASK (3 << VLM_DECODE_SPLITS_SHIFT)
#define VLM_DECODE_NSPLITS_SHIFT 6 /* bits 6 .. 10 (added within ABI v8): S = (flags >> 6) & 31, 0 = not named.  S in 1 .. 16: the
                                   step of VLM_DECODE_SPLITS_SHIFT runs its attention and o_proj over EXACTLY S splits - the caller
                                   promises ctx + 1 <= 64 S for every replay, i.e. S = the pages of the longest context it will
                                   replay the step at.  Every split owns at most one page, a split whose page the context has
                                   not reached yet reports m = -inf and is dropped by the merge, and the live ones are added in
                                   the order of 16 splits: the same bytes.  The attention launch starts Hkv x S x 4 workgroups
                                   and none of them finds no page at the last replay; the o_proj prologue reads S (m, l, O)
                                   slots and none is dead (VLM_TUNE_GEMV_VARIANT bit 12: its exact forms; part_ml then has a
                                   per-head pitch of S rounded up to even, see vlm_attn_decode_paged_split).  Wins over the
                                   class of bits 4, 5 when both are set; S > 16 and every step that ignores the class ignore it.
                                   Part of the graph key like every flag: one captured step per count. */
#define VLM_DECODE_NSPLITS_MASK (31 << VLM_DECODE_NSPLITS_SHIFT)
#define VLM_DECODE_ROW_SAMPLER (1 << 11) /* bit 11 (added within ABI v8): the step's tail samples in ROW-TABLE mode (see
                                   VLM_SAMPLE_ROW_TABLE at vlm_sampler_params): row b draws with the line of row b in sample_ws, which
                                   the host rewrites as requests join and leave while the captured step keeps its arguments;
                                   temperature / top_p / min_p / top_k / seed of the args are ignored, `logprobs` and `scratch` are
                                   required.  With VLM_DECODE_FUSED_TAIL the sampler's last launch also does vlm_decode_advance and
                                   the next step's embedding gather (B <= 64), and bumps every row's count; without it the advance
                                   is a launch of its own.  Part of what a cached decode graph is keyed by (the flags are).
                                   Together with VLM_DECODE_WINDOW: an argument error, nothing is enqueued. */

int vlm_llm_create(const vlm_llm_config* cfg, void** handle);          /* (host) */
int vlm_llm_destroy(void* handle);
int vlm_llm_set_layer(void* handle, int layer, const vlm_llm_layer* w);
int vlm_llm_set_globals(void* handle, const vlm_llm_globals* g);
int vlm_llm_set_kv(void* handle, const vlm_kv_pool* kv);
int vlm_llm_prefill(void* handle, const vlm_prefill_args* a, void* stream);
int vlm_llm_decode_step(void* handle, const vlm_decode_args* a, void* stream);
/* embeddings -> logits only (no sampling, no advance): language_model(y, cache=...) at L == 1 */
int vlm_llm_decode_forward(void* handle, const vlm_decode_args* a, void* stream);
/* capture vlm_llm_decode_step into a hipGraph owned by the handle / replay it */
int vlm_llm_decode_graph_build(void* handle, const vlm_decode_args* a, void* stream);
int vlm_llm_decode_graph_launch(void* handle, void* stream);
/* number of kernel launches in one decode step (for reporting) */
int vlm_llm_decode_launches(void* handle);

/* Tuning of the captured decode step (no effect on results; measured defaults in DESIGN.md).  Changing a value drops
 * the cached graphs of the handle.
 * (keys 0..5 and 10 were the round-2 / round-3 experiments - weight prefetch on a side branch, the fused MLP launch,
 *  launch-skipping masks, translation warm-up - which lost to the five-launch layer; they left the library in ABI v5 and
 *  live on as sources under scripts/rejected/ with their measurements in profiles/) */
#define VLM_TUNE_MFMA_GEMV 6        /* 1 (default): decode steps of 3..16 rows run their projections on the matrix cores
                                       (csrc/gemv_mfma.hip); 0: the v_dot2c GEMVs (rows in {4, 8}) - A/B knob */
#define VLM_TUNE_ATTN_PAGESPLIT 7   /* decode attention of steps with at most 64 (row, kv head) pairs: N > 0 (default 16) = the
                                       page-split form (vlm_attn_decode_paged_split) with up to N workgroups per pair (32 when
                                       the caller asked for a split, i.e. a long context); 0 = the round-2 forms (one workgroup
                                       per pair, or split-K partials merged in the o_proj prologue) - A/B knob */
#define VLM_TUNE_GEMV_VARIANT 8     /* A/B knob of the batch-1 GEMV launch shapes (bit 0: down projection with 6 rows per
                                       workgroup = one workgroup per CU at N = 1536; bit 1: 3 rows;
                                       bit 2 (4): gate/up (RMSNorm prologue, SwiGLU, N >= 8192) with 2 rows per wave instead of 4
                                       - twice the workgroups, a gate / up pair stays in one wave;
                                       bit 3 (8): the head GEMV (RMSNorm prologue, no epilogue, N >= 8192) likewise;
                                       bit 4 (16): the o_proj that merges the page-split attention (vlm_gemv_attn_out_bf16,
                                       Hq * D <= 1536) with 4 rows per wave - half as many workgroups repeat the merge;
                                       bit 5 (32): RMSNorm-prologue GEMVs of ONE row: the three waves of a workgroup that do not
                                       store the normalised row fetch x / norm_w through a zero-extent buffer resource, i.e.
                                       generate no memory traffic for them;
                                       bits 8, 9 (256, 512): the knob's launches of the same step that are no GEMV - the
                                       partial-only page-split attention (vlm_attn_decode_paged_split with out == NULL, at most
                                       64 (row, kv head) pairs) splits the eight 16-row output tiles of a page over 2 (bit 8) or
                                       4 (bit 9; wins over bit 8) workgroups in grid z: each computes the scores and softmax
                                       statistics of its pages as the single workgroup does and loads V, multiplies and stores
                                       for its own tiles only; z = 0 stores (m, l).
                                       bit 11 (2048): vlm_gemv_attn_out_bf16 over at most 4 / 8 / 12 splits reads that many
                                       (m, l, O) slots ahead of its weights, not all 16 (dead slots are dropped by a select either
                                       way), and the Python layer asks for such launches: a one-row greedy step carries the
                                       context class of VLM_DECODE_SPLITS_SHIFT in its flags.
                                       bit 12 (4096): vlm_gemv_attn_out_bf16 at Hq * D <= 1536 (and bit 4 off) over S splits runs a
                                       prologue compiled for exactly S = 1 .. 16: S slots, no clamped address, and the (m, l) pairs
                                       of a head as ceil(S / 2) 16-byte loads where part_ml has an even per-head pitch (an odd one
                                       keeps the forms of bit 11); the Python layer names the page count of a one-row greedy
                                       step's context in VLM_DECODE_NSPLITS_SHIFT of its flags.
                                       bit 6 (64): the qkv launch of a ONE-row step at hidden <= 1536 and Hq * D <= 1536 takes (Hq, Hkv, D)
                                       and long_from from a preloaded argument slot and pos / slot / inv_freq by scalar loads:
                                       nothing is waited for ahead of its weight stream (more rows and wider heads keep their entry).
                                       bit 13 (8192): the log-sum-exp partials of the sampler (greedy tail and vlm_sample) load a
                                       thread's elements once and keep them in registers across the max and the sum pass
                                       (V <= 163,840; a longer row takes the two-pass loop) - same element-to-thread assignment, same
                                       order of every max and add.
                                       bit 14 (16384): the fused greedy tail (vlm_sample_greedy_advance) issues the logits loads of a
                                       thread's first two trips ahead of the loads of the partials, and with one row the block that
                                       takes the last row ticket is the last block: no second ticket level.
                                       A row's sum does not depend on the rows its wave owns, an output tile not on the
                                       workgroup that owns it, a merge not on slots that hold no page: every bit gives the same
                                       bytes.
                                       Measured (profiles/decode_slack_ab.txt, profiles/latency_launches_ab.txt,
                                       profiles/split_classes_ab.txt, profiles/split_exact_ab.txt, profiles/decode_tail_entry_ab.txt): bits 0, 2, 3, 9, 11, 12 win,
                                       bit 6 wins alone, bit 13 as part of the whole step - the Python layer sets 14925 - bit 14 gains nothing measurable, bit 4
                                       loses 1.7 %, bit 5 changes nothing, bit 8 gains half of bit 9; bits 7 and 10 are unused:
                                       the o_proj in three-wave workgroups (-0.7 %) and the greedy tail's log-sum-exp partials
                                       written by the head GEMV (-0.5 %) were measured on them and left the library) */
#define VLM_TUNE_ATTN_MERGE 9       /* where the page-split attention of a ONE-row step is merged: 1 (default) = in the o_proj
                                       GEMV's prologue (partial-only attention launch, vlm_gemv_attn_out_bf16; needs bf16 Wo,
                                       Hq * D <= 2048, <= 16 splits), 0 = by the attention launch's last-arriving workgroup */
/* Modes of the decode step: these keys DO change what a step computes (the sentence above holds for keys 6..9 only).  They
 * travel through vlm_llm_set_tuning / vlm_llm_get_tuning because the C ABI is frozen at v8; changing a value drops the cached
 * graphs of the handle as the tuning keys do.  Read by steps whose flags carry VLM_DECODE_WINDOW. */
#define VLM_MODE_WINDOW_SIZE 16     /* M = max_kv_size: slots of a row's ring; 0 (default) = no window (the flag is then refused).
                                       A window step needs M > keep + 1 */
#define VLM_MODE_WINDOW_KEEP 17     /* K = the first K slots (attention sinks) are never overwritten (make_prompt_cache: 4) */
#define VLM_MODE_WINDOW_RING_POS 18 /* 1: the rope position follows the ring's write index (the reference's Qwen2-VL reads
                                       cache._idx as its offset, qwen2_vl/language.py:426-431); 0 (default): it follows the tokens
                                       seen (cache.offset: the plain-rope families) */
#define VLM_MODE_QWEN3 19           /* 1: the Qwen3-VL language model (added within ABI v8; set right after vlm_llm_create, BEFORE
                                       vlm_llm_set_layer; head_dim == 128, one rope table, no rope_qk_scale - argument error
                                       otherwise).  Every q and k head goes through RMSNorm(head_dim) with vlm_llm_layer.q_norm_w /
                                       k_norm_w and rms_eps between the qkv projection and the rotation, and the rotation takes the
                                       INTERLEAVED selector over mrope_section (rope_utils.py:511-516: frequency f reads the h position
                                       when f % 3 == 1 and f < 3 sec1, the w position when f % 3 == 2 and f < 3 sec2, else t).  The qkv
                                       step of a decode layer is then TWO launches at every row count - the projection with its
                                       RMSNorm prologue, then the QK-norm form of the rotary + KV-write launch - and vlm_llm_prefill
                                       reads the DeepStack fields of vlm_prefill_args.  0 (default): everything as before */
int vlm_llm_set_tuning(void* handle, int key, int value);
int vlm_llm_get_tuning(void* handle, int key);

/* The encoder-layer loop of the SigLIP / CLIP vision towers (idefics2/vision.py:141-187, llava_bunny/vision.py:139-200,
 * phi3_v/vision.py:117-175: x = x + out_proj(attention(LN1(x))); x = x + fc2(act(fc1(LN2(x)))), biases everywhere, no
 * rope, no mask) as one native call: n_layers x [LayerNorm, qkv GEMM + bias, varlen flash attention, out GEMM + bias +
 * residual, LayerNorm, fc1 GEMM + bias + activation, fc2 GEMM + bias + residual] enqueued back to back.
 * x [N][E] residual stream (in / out); workspaces xn [N][E], qkv [N][3 H head_dim], attn [N][H head_dim], mlp [N][MH];
 * wqkv rows [q | k | v] of H * head_dim each (head_dim = the kernel's width: 64 / 80 / 128 - narrower heads zero-padded
 * by the caller, wo's columns likewise); act_epilogue VLM_EPI_GELU_FAST / VLM_EPI_GELU_ERF / VLM_EPI_GELU_TANH / 0; cu_seqlens int32
 * [nseg + 1], total_qblocks = sum ceil(len / 128); uniform_segments: vlm_attn_prefill's placement hint.
 * Added within ABI v8: act_epilogue | VLM_EPI_LAYERSCALE - the InternViT layer (internvl_chat/vision.py:126-132),
 * x = x + ls1 * out_proj(..); x = x + ls2 * fc2(..): bo and b2 then point at bf16 [2][E], the bias row followed by the
 * ls1 / ls2 row, and both GEMMs run VLM_EPI_BIAS | VLM_EPI_RESIDUAL | VLM_EPI_LAYERSCALE.  Without the bit nothing changes. */
typedef struct vlm_enc_layer {
  const void *ln1_w, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_w, *ln2_b, *w1, *b1, *w2, *b2;
} vlm_enc_layer;
int vlm_encoder_forward(const vlm_enc_layer* layers /* host array */, int n_layers, void* x, void* xn, void* qkv, void* attn,
                        void* mlp, int N, int E, int H, int head_dim, int MH, float ln_eps, int act_epilogue,
                        const void* cu_seqlens, int nseg, int total_qblocks, float scale, int uniform_segments, void* stream);

typedef struct vlm_vit_config {
  int depth, embed_dim, n_heads, mlp_hidden, patch_k /* padded K of the patch GEMM */, merge /* 2 */, out_dim;
  float ln_eps;
  int qk_interleaved; /* 1: the q / k rows of every wqkv / bqkv are interleaved per head (vlm_gemm_bf16_rope2d) and
                         cos_tab / sin_tab of vlm_vit_args are ONE table (sin_tab == cos_tab + N * head_dim / 2): the 2-D
                         rope runs in the qkv GEMM epilogue instead of a pass of its own.
                         Added within ABI v8: the field is a FLAG WORD.  Bit 0 keeps that meaning; bit 1
                         (VLM_VIT_FORM_QWEN2_5) selects the Qwen2.5-VL block form, bit 2 (VLM_VIT_FORM_QWEN3) the Qwen3-VL
                         form, see vlm_vit_forward below */
} vlm_vit_config;
#define VLM_VIT_QK_INTERLEAVED 1
#define VLM_VIT_FORM_QWEN2_5 2
#define VLM_VIT_FORM_QWEN3 4

typedef struct vlm_vit_block {
  const void *ln1_w, *ln1_b, *wqkv, *bqkv, *wproj, *bproj, *ln2_w, *ln2_b, *wfc1, *bfc1, *wfc2, *bfc2;
  /* Added within ABI v8, APPENDED: read only for a handle created with VLM_VIT_FORM_QWEN3 (vlm_vit_set_block copies the first
   * 12 pointers otherwise).  tap_w0 != NULL: a DeepStack tap follows this block - the post-shuffle PatchMerger of
   * deepstack_merger_list (qwen3_vl/vision.py:106-123): LayerNorm weights / bias [4E], Linear [4E][4E] + bias, Linear
   * [out_dim][4E] + bias.  The taps fill vlm_vit_args.tap_out in block order. */
  const void *tap_ln_w, *tap_ln_b, *tap_w0, *tap_b0, *tap_w2, *tap_b2;
} vlm_vit_block;

typedef struct vlm_vit_globals {
  const void *wpatch /* [embed_dim][patch_k] */, *ln_q_w, *ln_q_b, *wm0, *bm0, *wm2, *bm2;
  const void* bpatch; /* added within ABI v8, APPENDED, VLM_VIT_FORM_QWEN3 handles only: the patch Conv3d's bias, bf16 [embed_dim] */
} vlm_vit_globals;

/* VisionModel.__call__ (vision.py:257-290): patches bf16 [N][patch_k] -> out bf16 [N/merge^2][out_dim].
 * Workspaces: x [N][E], xn [N][E], qkv [N][3E], attn [N][E], mlp [N][mlp_hidden], mrg [N/4][4E].
 *
 * Added within ABI v8 - the Qwen2.5-VL form (VLM_VIT_FORM_QWEN2_5 | VLM_VIT_QK_INTERLEAVED in vlm_vit_config.qk_interleaved;
 * reference mlx_vlm/models/qwen2_5_vl/vision.py:177-193,326-393).  Per block: RMSNorm, qkv GEMM + bias with the 2-D rope in
 * its epilogue, attention over the window table (or over cu_seqlens for a block of fullatt_mask), proj GEMM + bias +
 * residual, RMSNorm, gate / up GEMM + bias + SwiGLU, down GEMM + bias + residual; merger RMSNorm -> [N/4][4E] -> Linear +
 * GELU(erf) -> Linear.  vlm_vit_block keeps its 12 pointers: ln1_b == ln2_b == NULL, wfc1 / bfc1 = the gate / up rows and
 * biases INTERLEAVED (gate_j, up_j) as VLM_EPI_SWIGLU wants them, [2 mlp_hidden][E] / [2 mlp_hidden], wfc2 / bfc2 = down
 * [E][mlp_hidden]; mlp_hidden = intermediate_size zero-padded to a multiple of 64 (a padded unit gives silu(0) * 0 = 0);
 * vlm_vit_globals.ln_q_b == NULL.  The rows are taken in WINDOW order: behind the patch GEMM the N / merge^2 merge units
 * are gathered by window_index (cos_tab / sin_tab are passed in that order already), behind the merger the rows are gathered
 * back by reverse_index - both on the device, inside the call.  Workspaces as above; head_dim % 16 == 0,
 * out_dim <= merge^2 * mlp_hidden (the un-permuted merger rows borrow the mlp workspace). */
typedef struct vlm_vit_args {
  const void* patches;
  int N;
  const void *cos_tab, *sin_tab; /* fp32 [N][head_dim/2] */
  const void* cu_seqlens;
  int nseg, total_qblocks;
  void *x, *xn, *qkv, *attn, *mlp, *mrg, *out;
  int uniform_segments;          /* 1: all segments have the same length (vlm_attn_prefill placement hint) */
  /* Added within ABI v8, APPENDED: read only for a handle created with VLM_VIT_FORM_QWEN2_5 - a caller of the first form may
   * keep passing the struct up to uniform_segments.  The window table of the tower's window blocks (vision.py:261-346),
   * int32 [win_nseg + 1] over the rows in WINDOW order, zero-length windows dropped; win_total_qblocks as total_qblocks;
   * win_max_seg = its longest segment; win_one_tile != 0: window blocks run the one-tile attention (vlm_attn_prefill bit 3;
   * needs win_max_seg <= 64 and head_dim 80), 0: the general kernel over the same table.  window_index / reverse_index int32
   * [N / merge^2]: row u of the window order is merge unit window_index[u] of the patch rows, and output row j is row
   * reverse_index[j] = argsort(window_index)[j] of the merger's.  fullatt_mask: bit i set = block i attends over cu_seqlens
   * (fullatt_block_indexes; depth <= 64). */
  const void* win_cu_seqlens;
  int win_nseg, win_total_qblocks, win_max_seg, win_one_tile;
  const void *window_index, *reverse_index;
  unsigned long long fullatt_mask;
  /* Added within ABI v8, APPENDED: read only for a handle created with VLM_VIT_FORM_QWEN3 | VLM_VIT_QK_INTERLEAVED (reference
   * mlx_vlm/models/qwen3_vl/vision.py:379-425).  That form is the FIRST form's block (LayerNorm, biased qkv with the 2-D rope
   * in the GEMM epilogue, attention over cu_seqlens, biased MLP) with: x = T(T(patches Wp^T + bpatch) + pos_rows) in front -
   * pos_rows bf16 [N][embed_dim] = fast_pos_embed_interpolate's rows, in the patch rows' merge-unit order (made by the caller);
   * VLM_EPI_GELU_TANH in the MLP; behind every block whose vlm_vit_block.tap_w0 is set, the post-shuffle merger of that block
   * into tap_out bf16 [n_taps][N / merge^2][out_dim] (n_taps = the number of such blocks, VLM_ERR_ARG otherwise); then the main
   * merger of the first form.  head_dim in {64, 80, 128}, merge^2 * embed_dim <= 8192 (VLM_ERR_SHAPE otherwise).  The window
   * fields above are not read. */
  const void* pos_rows;
  void* tap_out;
  int n_taps;
} vlm_vit_args;

int vlm_vit_create(const vlm_vit_config* cfg, void** handle);
int vlm_vit_destroy(void* handle);
int vlm_vit_set_block(void* handle, int i, const vlm_vit_block* w);
int vlm_vit_set_globals(void* handle, const vlm_vit_globals* g);
int vlm_vit_forward(void* handle, const vlm_vit_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VLM_HIP_H_ */
