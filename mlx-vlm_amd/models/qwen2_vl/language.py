"""Qwen2-VL language model on MI355X - host mirror of the reference's
mlx_vlm/models/qwen2_vl/language.py (LanguageModel: same call contract,
get_rope_index, rope-delta position rule) on top of the native engine
(csrc/engine.hip): prefill = MFMA GEMMs + causal flash attention + paged KV
write, decode = weight-streaming GEMV chain + paged split-K attention, both
enqueued by ONE native call per forward.

Differences from the reference that the contract allows:
  * `supports_logits_to_keep = True` (reference hook, generate/ar.py:340-341):
    with logits_to_keep=1 only the last row goes through the lm_head instead of
    all L rows (the reference computes all and slices [:, -1], ar.py:358).
  * `make_cache()` (reference hook, cache.py:57-58) returns per-layer views of
    one paged sequence instead of 28 independent contiguous KVCache objects.
  * position ids are built on the host from host-resident ids / grids and
    uploaded once; the reference does the same work with per-token Python
    loops and .item() syncs (language.py:242-382).
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from ... import _lib, ops
from ..._lib import check
from ..base import LanguageModelOutput, deepstack_window
from ..cache import PAGE, Arena, KVCache, KVPool, PagedSequence
from .config import ModelConfig, TextConfig


def _to_np(x):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def dense(x):
    """a 4-bit matrix materialised as bf16 for a GEMM (the prompt-chunk path); anything else as it is"""
    return ops.dequant_w4(x.wq, x.sb) if hasattr(x, "wq") else x


class DecodeState:
    """Device-resident state of a batch of B decoding sequences (what one graph replay reads/writes)."""

    def __init__(self, lm: "LanguageModel", B: int, nsplit: int = 32, ring_len: int = 64):
        t, dev = lm.args, lm.device
        D, hd, Hq, Hkv = t.hidden_size, lm.head_dim, t.num_attention_heads, t.num_key_value_heads
        bf, i32 = torch.bfloat16, torch.int32
        self.B, self.nsplit, self.ring_len = B, nsplit, ring_len   # nsplit: buffers sized for the max, see decode_begin
        A = lm.arena.alloc
        self.tok = A(B, i32, zero=True)
        # [2][B] each: row 0 is what every step reads (rope position / entries held); row 1 belongs to the window mode of a step
        # (_lib.DECODE_WINDOW: pos row 1 = rope delta, ctx row 1 = the slot the step writes) and is unused where nothing rotates
        self.pos2 = A((2, B), i32, zero=True)
        self.ctx2 = A((2, B), i32, zero=True)
        self.pos, self.ctx = self.pos2[0], self.ctx2[0]
        self.window = None          # (M, K, ring_pos) while the bound sequences decode on the device-resident window
        self.step = A(1, i32, zero=True)
        self.h = A((B, D), bf)
        self.qkv = A((B, (Hq + 2 * Hkv) * hd), bf)
        self.attn = A((B, Hq * hd), bf)
        # (16 rows even for a narrower state: a 5..16-row step hands the SwiGLU output to the down projection in the MFMA tile's
        #  layout [inter / 8][16][8] - vlm_decode_args.flags VLM_DECODE_ACT16, csrc/gemv_mfma_rows.hip)
        self.act = A((max(B, 16), t.intermediate_size), bf)
        self.part_ml = A((B, Hq, nsplit, 2), torch.float32)
        self.out_ring = A((ring_len, B), i32, zero=True)
        self.host_ring = None       # pinned twin of out_ring, allocated when a step first runs with _lib.DECODE_HOST_RING
        # rows at pitch VL = vocab rounded up to 8 (the engine's pitch: 16-byte aligned rows for any vocabulary, e.g. 32003)
        VL = (t.vocab_size + 7) & ~7
        self.logits = torch.empty(B, VL, dtype=bf, device=dev)[:, : t.vocab_size]
        self.logprobs = torch.empty(B, VL, dtype=bf, device=dev)[:, : t.vocab_size]
        self.scratch = torch.empty(B, VL, dtype=bf, device=dev)[:, : t.vocab_size]
        self.part_o = torch.empty(B, Hq, nsplit, hd, dtype=torch.float32, device=dev)
        self.sample_ws = ops.sample_workspace(B, dev)
        # history of fed tokens for the logits processors (penalties): ring per row + count
        from ...sample_utils import HIST_CAP
        self.hist = A((B, HIST_CAP), i32, zero=True)
        self.hist_len = A(B, i32, zero=True)
        self._pen = None            # (key, PenaltyArgs, device bias tensors) kept alive while a graph may use them
        self.graph_key = None

    MAX_ROW_BIAS = 64           # logit_bias entries per request in the per-row form

    @staticmethod
    def mask_words_of(vocab: int) -> int:
        """32-bit words of a token bitmask over `vocab` logits"""
        return (int(vocab) + 31) // 32

    @property
    def mask_words(self) -> int:
        return self.mask_words_of(self.logits.shape[1])

    @property
    def bias_stride(self) -> int:
        """entries of one row of the bias tables: the bias list in front, the row's token bitmask at the END (vlm_penalty_args)"""
        return self.MAX_ROW_BIAS + self.mask_words

    def row_penalty_tables(self):
        """Device tables of the per-request processors of a continuous batch (vlm_penalty_args.row_params): fp32 [B, 8]
        parameters and [B, MAX_ROW_BIAS + ceil(vocab / 32)] bias lists - wide enough for a full token bitmask behind the bias
        entries from the start, so that a captured step never sees the pointers move - allocated on first use, all zero =
        every row passes through."""
        if getattr(self, "row_params", None) is None:
            dev = self.hist.device
            self.row_params = torch.zeros(self.B, 8, dtype=torch.float32, device=dev)
            self.row_bias_idx = torch.zeros(self.B, self.bias_stride, dtype=torch.int32, device=dev)
            self.row_bias_val = torch.zeros(self.B, self.bias_stride, dtype=torch.float32, device=dev)
            self._pen_rows = _lib.PenaltyArgs(self.hist.data_ptr(), self.hist_len.data_ptr(), self.hist.shape[1], 0.0, 0, 0.0, 0,
                                              0.0, 0, self.row_bias_idx.data_ptr(), self.row_bias_val.data_ptr(), 0,
                                              self.row_params.data_ptr(), self.bias_stride)
        return self._pen_rows

    @classmethod
    def pack_row_penalties(cls, specs, hist_cap: int, mask_words: int = 0, masks=None):
        """specs: one sample_utils.LogitsProcessors (or None) per row -> host arrays (params f32 [n, 8], bias_idx i32
        [n, S], bias_val f32 [n, S]; S = MAX_ROW_BIAS + mask_words) in the layout of vlm_penalty_args.row_params.
        masks: per row None or the int32 words of its token bitmask (at most mask_words of them): they go to the end of the
        row's bias_idx entries and their count into slot 7."""
        n = len(specs)
        S = cls.MAX_ROW_BIAS + int(mask_words)
        params = np.zeros((n, 8), dtype=np.float32)
        bidx = np.zeros((n, S), dtype=np.int32)
        bval = np.zeros((n, S), dtype=np.float32)
        for r, sp in enumerate(specs):
            if not sp:
                continue
            bias = sp.logit_bias or {}
            if len(bias) > cls.MAX_ROW_BIAS:
                raise NotImplementedError(f"more than {cls.MAX_ROW_BIAS} logit_bias entries per request in a continuous batch")
            params[r, :6] = (sp.repetition_penalty, min(sp.repetition_context_size, hist_cap), sp.presence_penalty,
                             min(sp.presence_context_size, hist_cap), sp.frequency_penalty, min(sp.frequency_context_size, hist_cap))
            params[r, 6] = len(bias)
            bidx[r, :len(bias)] = list(bias.keys())
            bval[r, :len(bias)] = list(bias.values())
        for r, words in enumerate(masks or ()):
            if words is None:
                continue
            from ...structured import mask_words_of

            w = mask_words_of(words, mask_words)
            if len(w):
                params[r, 7] = len(w)
                bidx[r, S - len(w):] = w
        return params, bidx, bval

    def penalty_args(self, spec):
        """_lib.PenaltyArgs over this state's history for a sample_utils.LogitsProcessors spec (cached per spec);
        spec == "rows": the per-row tables of a continuous batch (row_penalty_tables)."""
        if isinstance(spec, str) and spec == "rows":
            return self.row_penalty_tables()
        if not spec:
            return None
        if self._pen is None or self._pen[0] != spec.key():
            bias = spec.logit_bias or {}
            idx = _lib.h2d(np.asarray(list(bias.keys()), dtype=np.int32), self.hist.device) if bias else None
            val = _lib.h2d(np.asarray(list(bias.values()), dtype=np.float32), self.hist.device) if bias else None
            pa = _lib.PenaltyArgs(self.hist.data_ptr(), self.hist_len.data_ptr(), self.hist.shape[1],
                                  float(spec.repetition_penalty), int(spec.repetition_context_size),
                                  float(spec.presence_penalty), int(spec.presence_context_size),
                                  float(spec.frequency_penalty), int(spec.frequency_context_size),
                                  idx.data_ptr() if idx is not None else None, val.data_ptr() if val is not None else None,
                                  len(bias))
            self._pen = (spec.key(), pa, idx, val)
        return self._pen[1]

    def set_history(self, rows_tokens):
        """rows_tokens[b] = the tokens fed so far for row b (the prompt): the last HIST_CAP of them go into the ring"""
        cap = self.hist.shape[1]
        host = np.zeros((len(rows_tokens), cap), dtype=np.int32)
        lens = np.zeros(len(rows_tokens), dtype=np.int32)
        for b, t in enumerate(rows_tokens):
            t = np.asarray(t, dtype=np.int64).reshape(-1)[-cap:]
            host[b, :len(t)] = t
            lens[b] = len(t)
        self.hist[:len(rows_tokens)].copy_(_lib.h2d(host, self.hist.device))
        self.hist_len[:len(rows_tokens)].copy_(_lib.h2d(lens, self.hist.device))

    def args(self, temperature=0.0, top_p=1.0, min_p=0.0, top_k=0, seed=0, with_logprobs=True, B=None, flags=0,
             penalties=None):
        """B < self.B: the step runs over the first B rows (every buffer is row-major, a prefix is a valid state).
        flags: _lib.DECODE_FUSED_TAIL = the step starts from h == embed[tok] and leaves the next step's h behind."""
        p = lambda t: t.data_ptr()  # noqa: E731
        ring = self.out_ring
        if int(flags) & _lib.DECODE_HOST_RING:
            if self.host_ring is None:
                self.host_ring = torch.zeros(self.ring_len, self.B, dtype=torch.int32).pin_memory()
            ring = self.host_ring
        return _lib.DecodeArgs(self.B if B is None else int(B), p(self.tok), p(self.pos), p(self.ctx), p(self.step), p(self.h), p(self.qkv),
                               p(self.attn), p(self.act), p(self.logits),
                               p(self.logprobs) if (with_logprobs or temperature > 0) else None, p(self.scratch),
                               p(self.part_o), p(self.part_ml), p(self.sample_ws), p(ring), self.ring_len,
                               self.nsplit, float(temperature), float(top_p), float(min_p), int(top_k),
                               int(seed) & 0xFFFFFFFF, int(flags) | _lib.DECODE_ACT16,       # (self.act holds 16 rows)
                               C.pointer(pa) if (pa := self.penalty_args(penalties)) is not None else None)


class LanguageModel:
    # rows of one decode step (decode_step_rows): up to 16 on the GEMV family (v_dot2c: 1 / 2 / 4 / 8, skinny-M MFMA: 5..16), 17..64 as
    # WIDE steps on the prefill GEMMs (needs the caller's block table; not for two-table RoPE models: phi3_v sets 16)
    MAX_DECODE_ROWS = 64

    # widest residual stream the engine runs (vlm_llm_create: Qwen2-VL-72B's 8192; multiples of 128 past 4096)
    MAX_HIDDEN = 8192

    supports_logits_to_keep = True

    def __init__(self, args: TextConfig, config: ModelConfig, device="cuda", kv_pool_tokens: int = 32768,
                 max_seqs: int = 64, kv_layout: str = "auto"):
        if args.hidden_size > self.MAX_HIDDEN or (args.hidden_size > 4096 and args.hidden_size % 128):
            raise NotImplementedError(f"hidden_size = {args.hidden_size}: the engine is built for hidden sizes up to {self.MAX_HIDDEN} "
                                      "(multiples of 128 above 4096)")
        self.args = args
        self.config = config
        self.model_type = args.model_type
        self.device = device
        self._rope_deltas = None
        self._position_ids = None
        self._handle = None
        self._w: Dict[str, torch.Tensor] = {}
        self._kv_pool_tokens, self._max_seqs = kv_pool_tokens, max_seqs
        self._kv_layout = os.environ.get("VLM_KV_LAYOUT", kv_layout)   # env: A/B knob for measurements
        self.pool: Optional[KVPool] = None
        self._decode_states: Dict[int, DecodeState] = {}
        sec = list((args.rope_scaling or {}).get("mrope_section", [16, 24, 24]))
        self.mrope_section = sec

    # ------------------------------------------------------------------ properties (reference language.py:520-530)
    @property
    def layers(self):
        return list(range(self.args.num_hidden_layers))

    @property
    def head_dim(self):
        """An explicit `args.head_dim` wins (a model whose heads are zero-padded to a width the kernels have)."""
        return getattr(self.args, "head_dim", None) or self.args.hidden_size // self.args.num_attention_heads

    @property
    def n_kv_heads(self):
        return self.args.num_key_value_heads

    # ------------------------------------------------------------------ weights
    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: names relative to `language_model.` (`model.layers.i....`, `model.embed_tokens.weight`, `lm_head.weight`).
        Packs q/k/v into one [Hq*D + 2*Hkv*D, hidden] matrix and interleaves gate/up rows (g0,u0,g1,u1,...) so the
        SwiGLU product is an epilogue of one GEMM/GEMV."""
        t, dev = self.args, self.device
        L = _lib.lib()
        bf = torch.bfloat16

        from .. import quantized as Qz

        def g(name):
            return W[name].to(device=dev, dtype=bf)

        def lin(path):
            """a projection weight: bf16 tensor, or QuantW when the checkpoint holds `<path>.scales` (utils.py:961)"""
            if isinstance(W.get(path + ".weight"), Qz.QuantW):      # already packed by a model-specific loader (phi3_v)
                return W[path + ".weight"].to(dev)
            if Qz.has_scales(W, path):
                return Qz.take(W, path).to(dev)
            return g(path + ".weight")

        # small tensors (norm weights, biases, rope table, decode state, block table) live in ONE arena
        small_bytes = t.num_hidden_layers * (2 * t.hidden_size + (t.num_attention_heads + 2 * t.num_key_value_heads) * self.head_dim) * 2
        self.arena = Arena(small_bytes + (8 << 20), device=dev)
        # ... and the big matrices live in ONE allocation too, in the order a decode step streams them, so the
        # driver can map the region with large page fragments (A/B knob: VLM_WEIGHT_ARENA=0 -> separate tensors)
        qkv_rows = (t.num_attention_heads + 2 * t.num_key_value_heads) * self.head_dim
        per_layer = (qkv_rows + t.num_attention_heads * self.head_dim + 3 * t.intermediate_size) * t.hidden_size * 2
        n_big = t.num_hidden_layers * per_layer + (1 if t.tie_word_embeddings else 2) * (t.vocab_size + 8) * t.hidden_size * 2
        use_wa = os.environ.get("VLM_WEIGHT_ARENA", "1") != "0" and not any(k.endswith(".scales") or isinstance(v, Qz.QuantW) for k, v in W.items())
        self.warena = Arena(n_big + (4 * t.num_hidden_layers + 4) * 4096, device=dev, zero=False) if use_wa else None

        def big(x):
            if isinstance(x, Qz.QuantW):
                return x                       # 4-bit matrices keep their own (small) allocations
            x = x.contiguous()
            if self.warena is None:
                return x
            out = self.warena.alloc(x.shape, x.dtype, align=4096)
            out.copy_(x)
            return out

        cfg = _lib.LlmConfig(t.hidden_size, t.num_hidden_layers, t.intermediate_size, t.num_attention_heads,
                             t.num_key_value_heads, self.head_dim, t.vocab_size, float(t.rms_norm_eps),
                             int(self.mrope_section[0]), int(self.mrope_section[1]),
                             float(getattr(t, "attn_scale", 0.0) or 0.0), float(getattr(t, "rope_qk_scale", 0.0) or 0.0),
                             int(getattr(self, "rope_long_from", 0) or 0))
        h = C.c_void_p()
        check(L.vlm_llm_create(C.byref(cfg), C.byref(h)), "llm_create")
        self._handle = h
        self.apply_tuning()
        self._set_engine_modes()           # (before the first vlm_llm_set_layer: a mode decides what the engine reads of a layer)
        for i in range(t.num_hidden_layers):
            p = f"model.layers.{i}."
            qkv_parts = [lin(p + "self_attn.q_proj"), lin(p + "self_attn.k_proj"), lin(p + "self_attn.v_proj")]
            if any(isinstance(x, Qz.QuantW) for x in qkv_parts):
                if not all(isinstance(x, Qz.QuantW) for x in qkv_parts):
                    raise NotImplementedError("q / k / v projections of one layer must be all quantized or all bf16")
                wqkv = Qz.cat_rows(qkv_parts)
            else:
                wqkv = big(torch.cat(qkv_parts, dim=0))
            bqkv = torch.cat([g(p + "self_attn.q_proj.bias"), g(p + "self_attn.k_proj.bias"),
                              g(p + "self_attn.v_proj.bias")], dim=0).contiguous() if self.QKV_BIAS else None
            gate, up = lin(p + "mlp.gate_proj"), lin(p + "mlp.up_proj")
            wo = big(lin(p + "self_attn.o_proj"))
            if isinstance(gate, Qz.QuantW) != isinstance(up, Qz.QuantW):
                raise NotImplementedError("gate / up projections of one layer must be both quantized or both bf16")
            wgu = Qz.interleave_rows(gate, up) if isinstance(gate, Qz.QuantW) else \
                big(torch.stack([gate, up], dim=1).reshape(2 * t.intermediate_size, t.hidden_size))
            del gate, up
            bqkv = self.arena.put(bqkv) if bqkv is not None else None
            ws = dict(ln1=self.arena.put(g(p + "input_layernorm.weight")), wqkv=wqkv, bqkv=bqkv, wo=wo,
                      ln2=self.arena.put(g(p + "post_attention_layernorm.weight")), wgu=wgu,
                      wdown=big(lin(p + "mlp.down_proj")))
            for k, v in ws.items():
                self._w[f"{i}.{k}"] = v

            def wp(x):
                return x.wq.data_ptr() if isinstance(x, Qz.QuantW) else x.data_ptr()

            def sp(x):
                return x.sb.data_ptr() if isinstance(x, Qz.QuantW) else None

            lay = _lib.LlmLayer(ws["ln1"].data_ptr(), wp(wqkv), bqkv.data_ptr() if bqkv is not None else None, wp(ws["wo"]),
                                ws["ln2"].data_ptr(), wp(wgu), wp(ws["wdown"]), sp(wqkv), sp(ws["wo"]), sp(wgu), sp(ws["wdown"]),
                                *self._layer_extra(i, p, W))
            check(L.vlm_llm_set_layer(h, i, C.byref(lay)), "llm_set_layer")
        def pad_rows8(x):
            """the head (and a tied embedding) gets zero rows up to a multiple of 8: the prefill logits GEMM runs over them"""
            n = (-x.shape[0]) % 8
            if n == 0:
                return x
            if isinstance(x, Qz.QuantW):
                return Qz.QuantW(torch.cat([x.wq, torch.zeros(n, x.wq.shape[1], dtype=x.wq.dtype, device=x.wq.device)]).contiguous(),
                                 torch.cat([x.sb, torch.zeros(n, x.sb.shape[1], dtype=x.sb.dtype, device=x.sb.device)]).contiguous())
            return torch.cat([x, torch.zeros(n, x.shape[1], dtype=x.dtype, device=x.device)])

        embed = big(pad_rows8(lin("model.embed_tokens")) if t.tie_word_embeddings else lin("model.embed_tokens"))
        head = embed if t.tie_word_embeddings else big(pad_rows8(lin("lm_head")))
        self.quantized = any(isinstance(v, Qz.QuantW) for v in self._w.values()) or isinstance(embed, Qz.QuantW) \
            or isinstance(head, Qz.QuantW)
        norm = self.arena.put(g("model.norm.weight"))
        hd = self.head_dim
        # compute_inv_freq (reference rope_utils.py:1042-1043), fp32 on the host
        # `args.rope_dim` < head_dim: only the first rope_dim / 2 pairs rotate (the rest get angle 0 = identity)
        rd = getattr(t, "rope_dim", None) or hd
        inv = torch.zeros(hd // 2, dtype=torch.float32)
        inv[: rd // 2] = 1.0 / (t.rope_theta ** (torch.arange(0, rd, 2).to(torch.float32) / rd))
        if getattr(t, "inv_freq", None) is not None:      # a model's own table (SuScaledRoPE: 1 / (factor * theta ** (2 i / d)))
            own = torch.as_tensor(t.inv_freq, dtype=torch.float32).reshape(-1)
            inv.zero_()
            inv[: own.numel()] = own
        if getattr(t, "inv_freq_long", None) is not None:   # second table behind the first (vlm_llm_config.rope_long_from)
            own = torch.as_tensor(t.inv_freq_long, dtype=torch.float32).reshape(-1)
            inv = torch.cat([inv, torch.zeros(hd // 2, dtype=torch.float32)])
            inv[hd // 2: hd // 2 + own.numel()] = own
        inv_freq = self.arena.put(inv.to(dev))
        self._w.update(embed=embed, head=head, norm=norm, inv_freq=inv_freq)
        isq = lambda x: isinstance(x, Qz.QuantW)    # noqa: E731
        gl = _lib.LlmGlobals(embed.wq.data_ptr() if isq(embed) else embed.data_ptr(), norm.data_ptr(),
                             head.wq.data_ptr() if isq(head) else head.data_ptr(), inv_freq.data_ptr(),
                             embed.sb.data_ptr() if isq(embed) else None, head.sb.data_ptr() if isq(head) else None)
        check(L.vlm_llm_set_globals(h, C.byref(gl)), "llm_set_globals")
        self._init_pool()

    # decode-step tuning (results are identical under every setting up to bf16 ties; defaults from the measurements in
    # DESIGN.md, environment overrides VLM_DECODE_<NAME> for A/B runs).  gemv_variant 14925 = 6669 | 64 | 8192; 6669 = bits 0, 2, 3, 9, 11, 12 of
    # VLM_TUNE_GEMV_VARIANT: down projection at 6 rows per workgroup, gate/up and head at 2 rows per wave
    # (profiles/decode_slack_ab.txt), the partial-only attention of a one-row step over 4 workgroups per page
    # (profiles/latency_launches_ab.txt), attention + o_proj of a one-row greedy step over as many splits as its context
    # has pages, in classes of 4 (profiles/split_classes_ab.txt) and, up to 1024 tokens, over exactly that many
    # (profiles/split_exact_ab.txt).  | 64 | 8192 = bits 6 and 13 (profiles/decode_tail_entry_ab.txt): the one-row qkv launch
    # that waits for no scalar load ahead of its weights (clears the bar alone) and the log-sum-exp partials in one pass
    # over memory; with them host_ring (tokens through a pinned ring, no copy kernel per step) is on: each of the two is
    # under the bar alone and positive in every series, and the step as a whole clears the bar against the parent with
    # them (+12.6 / +13.9 tok/s).  Bit 14 (the tail's early loads and one ticket level) and skip_logprobs
    # (generate_step(return_logprobs=False) hands its greedy steps no log-prob pointer, so the tail stores no 300 KB row
    # nobody reads) were not positive in both series alone: off, behind their switches
    TUNING_DEFAULTS = {"fused_tail": 1, "mfma_gemv": 1, "attn_pagesplit": 16, "gemv_variant": 6669 | 64 | 8192, "attn_merge": 1,
                       "host_ring": 1, "skip_logprobs": 0}

    QKV_BIAS = True             # q / k / v projections carry a bias (Qwen2); a family without one (Qwen3) hands the engine NULL

    def _set_engine_modes(self):
        """vlm_llm_set_tuning mode keys of the family, set between vlm_llm_create and the first vlm_llm_set_layer"""

    def _layer_extra(self, i, prefix, W):
        """the fields a family appends to vlm_llm_layer (read by the engine in that family's mode only)"""
        return ()

    def apply_tuning(self, **over):
        L = _lib.lib()
        t = dict(self.TUNING_DEFAULTS)
        for k in t:
            env = os.environ.get("VLM_DECODE_" + k.upper())
            if env is not None:
                t[k] = int(env, 0)
        t.update(over)
        self.tuning = t
        for key, name in ((_lib.TUNE_MFMA_GEMV, "mfma_gemv"), (_lib.TUNE_ATTN_PAGESPLIT, "attn_pagesplit"),
                          (_lib.TUNE_GEMV_VARIANT, "gemv_variant"), (_lib.TUNE_ATTN_MERGE, "attn_merge")):
            check(L.vlm_llm_set_tuning(self._handle, key, int(t[name])), "llm_set_tuning")
        for st in getattr(self, "_decode_states", {}).values():
            st.graph_key = None          # the engine dropped its captured steps

    def _init_pool(self):
        t = self.args
        self.pool = KVPool(t.num_hidden_layers, t.num_key_value_heads, self.head_dim, self._kv_pool_tokens,
                           self._max_seqs, max_pages_per_seq=min(512, (self._kv_pool_tokens + PAGE - 1) // PAGE),
                           device=self.device, arena=self.arena, layout=self._kv_layout)
        kv = _lib.KvPool(self.pool.kpool.data_ptr(), self.pool.vpool.data_ptr(), self.pool.layer_stride,
                         self.pool.block_table.data_ptr(), self.pool.max_pages)
        check(_lib.lib().vlm_llm_set_kv(self._handle, C.byref(kv)), "llm_set_kv")

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().vlm_llm_destroy(self._handle)
        except Exception:
            pass

    @property
    def embed_tokens_weight(self):
        return self._w["embed"]

    def embed_tokens(self, input_ids) -> torch.Tensor:
        """nn.Embedding (reference language.py:164,179).  input_ids [B, L] -> [B, L, D]"""
        ids = _lib.h2d(np.asarray(_to_np(input_ids), dtype=np.int32), self.device)
        B, Lq = ids.shape
        e = self._w["embed"]
        if hasattr(e, "wq"):          # nn.QuantizedEmbedding: dequantize of the looked-up rows
            out = ops.dequant_w4(e.wq, e.sb, rows=ids.reshape(-1).contiguous())
        else:
            out = ops.embed_gather(ids.reshape(-1), e)
        return out.view(B, Lq, -1)

    # ------------------------------------------------------------------ cache
    def make_cache(self) -> List[KVCache]:
        seq = PagedSequence(self.pool)
        return [KVCache(seq, i) for i in range(self.args.num_hidden_layers)]

    def make_cache_batch(self, n: int) -> List[List[KVCache]]:
        """n caches on consecutive block-table rows (what a decode batch needs)."""
        rows = self.pool.new_seqs(n)
        return [[KVCache(s, i) for i in range(self.args.num_hidden_layers)]
                for s in (PagedSequence(self.pool, r) for r in rows)]

    # ------------------------------------------------------------------ get_rope_index (reference language.py:216-402)
    def get_rope_index(self, input_ids, image_grid_thw=None, video_grid_thw=None, attention_mask=None):
        cfg = self.config
        input_ids = _to_np(input_ids)
        image_grid_thw, video_grid_thw = _to_np(image_grid_thw), _to_np(video_grid_thw)
        attention_mask = _to_np(attention_mask)
        B, L = input_ids.shape
        ms = cfg.vision_config.spatial_merge_size
        img_id, vid_id, vstart = cfg.image_token_id, cfg.video_token_id, cfg.vision_start_token_id
        if image_grid_thw is not None or video_grid_thw is not None:
            if attention_mask is None:
                attention_mask = np.ones_like(input_ids)
            position_ids = np.ones((3, B, L), dtype=np.int64)
            deltas = []
            ii = vi = 0
            for i in range(B):
                row_mask = attention_mask[i]
                toks = input_ids[i][row_mask == 1]
                tl = toks.tolist()
                starts = np.nonzero(toks[:-1] == vstart)[0]
                vision_tokens = toks[starts + 1]
                image_nums = int((vision_tokens == img_id).sum())
                video_nums = int((vision_tokens == vid_id).sum())
                chunks: List[np.ndarray] = []
                st, cur_max = 0, -1
                ri, rv = image_nums, video_nums
                for _ in range(image_nums + video_nums):
                    ed_image = tl.index(img_id, st) if (img_id in tl and ri > 0) else len(tl) + 1
                    ed_video = tl.index(vid_id, st) if (vid_id in tl and rv > 0) else len(tl) + 1
                    if ed_image < ed_video:
                        t_, h_, w_ = [int(x) for x in image_grid_thw[ii]]
                        ii += 1
                        ri -= 1
                        ed = ed_image
                    else:
                        t_, h_, w_ = [int(x) for x in video_grid_thw[vi]]
                        vi += 1
                        rv -= 1
                        ed = ed_video
                    gt, gh, gw = t_, h_ // ms, w_ // ms
                    text_len = ed - st
                    st_idx = cur_max + 1
                    chunks.append(np.broadcast_to(np.arange(text_len)[None], (3, text_len)) + st_idx)
                    tix = np.broadcast_to(np.arange(gt)[:, None], (gt, gh * gw)).reshape(-1)
                    hix = np.broadcast_to(np.arange(gh)[None, :, None], (gt, gh, gw)).reshape(-1)
                    wix = np.broadcast_to(np.arange(gw)[None, None, :], (gt, gh, gw)).reshape(-1)
                    vis = np.stack([tix, hix, wix]) + text_len + st_idx
                    chunks.append(vis)
                    cur_max = int(vis.max())   # == llm_pos_ids_list[-1].max() in the reference
                    st = ed + gt * gh * gw
                if st < len(tl):
                    st_idx = cur_max + 1
                    text_len = len(tl) - st
                    chunks.append(np.broadcast_to(np.arange(text_len)[None], (3, text_len)) + st_idx)
                if not chunks:
                    deltas.append(0)
                    continue
                llm_positions = np.concatenate(chunks, axis=1).reshape(3, -1)
                position_ids[:, i, row_mask == 1] = llm_positions
                deltas.append(int(llm_positions.max()) + 1 - len(tl))
            return position_ids, np.array(deltas, dtype=np.int64).reshape(-1, 1)
        if attention_mask is not None:
            am = attention_mask.astype(np.int64)
            position_ids = np.cumsum(am, axis=-1) - 1
            position_ids = np.where(am == 0, 1, position_ids)
            deltas = position_ids.max(axis=-1, keepdims=True) + 1 - am.shape[-1]
            return position_ids, deltas
        position_ids = np.broadcast_to(np.arange(L)[None], (B, L)).astype(np.int64)
        return position_ids, np.zeros((B, 1), dtype=np.int64)

    # ------------------------------------------------------------------ prefill over concatenated sequences
    def prefill(self, inputs_embeds: torch.Tensor, position_ids: np.ndarray, caches: List[List[KVCache]],
                lengths: List[int], logits_rows: str = "last", reserve_extra: int = 0, paged_attn: bool = False,
                deepstack=None) -> torch.Tensor:
        """inputs_embeds [T, D] (sequences concatenated, lengths[i] tokens each); position_ids int [3, T];
        caches[i] = the layer views of sequence i (appended after their current offset).
        paged_attn: chunks onto NON-EMPTY bf16 caches attend straight over the pages (ops.attn_prefill_paged) instead of over a
        gathered copy - the warm admission of the batch generator's prefix cache; every other caller leaves it False.
        deepstack (a family with DEEPSTACK only): (embeds bf16 [n_layers_ds, n_rows, D], rows int [n_rows]) - after decoder layer
        i < n_layers_ds the rows `rows` of the T rows of THIS call get embeds[i] added (reference qwen3_vl/language.py:231-283).
        -> logits [n_seq, V] (logits_rows == "last") or [T, V] ("all")."""
        t, dev = self.args, self.device
        T, D = inputs_embeds.shape
        hd, Hq, Hkv = self.head_dim, t.num_attention_heads, t.num_key_value_heads
        seqs = [c[0]._seq for c in caches]
        if any(s.offset != 0 for s in seqs):
            return self._prefill_onto_cache(inputs_embeds, position_ids, caches, lengths, logits_rows, reserve_extra,
                                            paged_attn=paged_attn, deepstack=deepstack)
        ds = self._deepstack_device(deepstack, T)
        cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        kv_seq = np.concatenate([np.full(n, s.seq, dtype=np.int32) for n, s in zip(lengths, seqs)])
        kv_slot = np.concatenate([np.arange(n, dtype=np.int32) for n in lengths])
        for n, s in zip(lengths, seqs):
            if s.rotating and n > s.max_size and self.ROTATING_PROMPT_WINDOW_MASK:
                # the reference's Phi-3.5-V hands cache[0] to create_attention_mask (phi3_v.py:163): for a first prompt longer
                # than max_kv_size RotatingKVCache.make_mask returns a causal mask WINDOWED to max_size (cache.py:586-596);
                # Qwen2-VL and Bunny pass the cache list and attend causally.  The windowed prefill is not built
                raise NotImplementedError(f"max_kv_size={s.max_size} with a prompt of {n} tokens: this family's reference prefills "
                                          "such a prompt under a sliding-window mask (RotatingKVCache.make_mask); only prompts "
                                          "up to max_kv_size are built for it")
            # (a rotating window never holds more than max(prompt, max_size) + 1 entries: max_kv_size bounds the reservation)
            s.reserve(max(n, s.max_size) + 1 if s.rotating else n + reserve_extra)
        kv = self._kv_struct(0)   # prefill addresses block-table rows by absolute sequence id
        check(_lib.lib().vlm_llm_set_kv(self._handle, C.byref(kv)), "llm_set_kv")
        nqb = int(sum((n + 127) // 128 for n in lengths))
        pos = np.ascontiguousarray(position_ids, dtype=np.int32)
        i32 = torch.int32
        pos_d = _lib.h2d(pos, dev)
        meta = _lib.h2d(np.concatenate([kv_seq, kv_slot, cu]), dev)
        kv_seq_d, kv_slot_d, cu_d = meta[:T], meta[T:2 * T], meta[2 * T:]
        if logits_rows == "last":
            rows = (cu[1:] - 1).astype(np.int32)
        else:
            rows = np.arange(T, dtype=np.int32)
        rows_d = _lib.h2d(rows, dev)
        bf = torch.bfloat16
        h = inputs_embeds.contiguous()
        xn = torch.empty(T, D, dtype=bf, device=dev)
        qkv = torch.empty(T, (Hq + 2 * Hkv) * hd, dtype=bf, device=dev)
        attn = torch.empty(T, Hq * hd, dtype=bf, device=dev)
        act = torch.empty(T, t.intermediate_size, dtype=bf, device=dev)
        xlast = torch.empty(len(rows), D, dtype=bf, device=dev)
        logits = torch.empty(len(rows), (t.vocab_size + 7) & ~7, dtype=bf, device=dev)[:, : t.vocab_size]      # pitch: see DecodeState
        a = _lib.PrefillArgs(h.data_ptr(), T, pos_d[0].data_ptr(), pos_d[1].data_ptr(), pos_d[2].data_ptr(),
                             kv_seq_d.data_ptr(), kv_slot_d.data_ptr(), cu_d.data_ptr(), len(lengths), nqb,
                             xn.data_ptr(), qkv.data_ptr(), attn.data_ptr(), act.data_ptr(), rows_d.data_ptr(),
                             len(rows), xlast.data_ptr(), logits.data_ptr(), int(bool(getattr(self, "_prefill_rope_long", False))),
                             *((ds[0].data_ptr(), ds[1].data_ptr(), ds[0].shape[0], ds[0].shape[1]) if ds is not None else ()))
        check(_lib.lib().vlm_llm_prefill(self._handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "llm_prefill")
        for n, s in zip(lengths, seqs):
            s.offset += n
            s.note_prefill(n)
        self._keep = (h, xn, qkv, attn, act, xlast, pos_d, meta, rows_d, ds)  # keep alive until the stream has run
        return logits

    DEEPSTACK = False           # does the engine mode of this family read vlm_prefill_args' DeepStack fields (Qwen3-VL)?

    def _deepstack_device(self, deepstack, T):
        """(embeds, rows) of a prefill call -> (contiguous bf16 [n, R, D] device tensor, int32 [R] device rows), or None"""
        if deepstack is None:
            return None
        if not self.DEEPSTACK:
            raise NotImplementedError(f"{type(self).__module__}: DeepStack embeddings are a Qwen3-VL input")
        embeds, rows = deepstack
        rows = np.asarray(_to_np(rows), dtype=np.int64).reshape(-1)
        if embeds is None or rows.size == 0 or len(embeds) == 0:
            return None
        embeds = embeds if isinstance(embeds, torch.Tensor) else torch.stack(list(embeds))
        if embeds.dim() != 3 or embeds.shape[1] != rows.size or embeds.shape[2] != self.args.hidden_size:
            raise ValueError(f"deepstack embeds {tuple(embeds.shape)} do not match {rows.size} rows of width {self.args.hidden_size}")
        if embeds.shape[0] > self.args.num_hidden_layers or rows.min() < 0 or rows.max() >= T or np.unique(rows).size != rows.size:
            raise ValueError("deepstack rows must be distinct rows of the call, the embeds at most one set per decoder layer")
        return (embeds.to(device=self.device, dtype=torch.bfloat16).contiguous(), _lib.h2d(rows.astype(np.int32), self.device))

    def _rope_kvwrite(self, i, qkv, pos_d, inv_tab, new_seq_d, new_slot_d, bt, kp, vp):
        """rotary embedding of layer i's q / k rows in place + their K / V into the pages (the prompt-chunk layer loop)"""
        t, sec = self.args, self.mrope_section
        ops.mrope_kvwrite_(qkv, t.num_attention_heads, t.num_key_value_heads, self.head_dim, pos_d[0], pos_d[1], pos_d[2], inv_tab,
                           int(sec[0]), int(sec[1]), kv_seq=new_seq_d, kv_slot=new_slot_d, block_table=bt, kpool=kp, vpool=vp,
                           qk_scale=getattr(t, "rope_qk_scale", None))

    def _layer_weights(self, i):
        """layer i's weights by the names of self._w; of a 4-bit model only THIS layer's matrices are dequantised"""
        if not self.quantized:
            return self._w
        return {k: dense(v) for k, v in self._w.items() if k.startswith(f"{i}.")}

    def _prefill_onto_cache(self, inputs_embeds, position_ids, caches, lengths, logits_rows, reserve_extra, paged_attn=False,
                            deepstack=None):
        """A prompt chunk appended to a NON-EMPTY cache: chunked prefill (reference ar.py:426-472), `prompt_cache=` continuation
        across calls, i.e. multi-turn (dispatch.py:861-882, common.py:243-263), a chunk onto a QuantizedKVCache (an update of any
        length, then quantized_scaled_dot_product_attention: cache.py:233-334, base.py:260-302) and the warm admission of the
        prefix cache (batch.py: the admission path of every warm request, not a rare one).  The chunk's queries attend to
        [cached tokens | the chunk] under the causal mask offset by the cache length (cache.py:345-367, base.py:366-373).
        The layer loop runs here over the C-ABI operators: per layer the chunk's K / V go into the pages (mrope_kvwrite_), then
        the chunk's rows attend by ONE of five routes, decided once:

          route      taken for                          the chunk's rows attend
          paged      paged_attn=True, any length        over the bf16 pages in place (attn_prefill_paged; bf16, 128-wide heads)
          q8_decode  an 8-bit cache, a short chunk      as decode rows over the 8-bit pages (attn_decode_paged_q8)
          q8_paged   an 8-bit cache, a longer chunk     over the 8-bit pages in place (attn_prefill_paged_q8)
          decode     a bf16 cache, a short chunk        as decode rows over the pages (attn_decode_paged)
          gather     everything else                    over a full-length copy [prefix | chunk] (kv_gather_ + attn_prefill)

        A short chunk: up to 64 new tokens in all (VLM_ONTO_CACHE_DECODE_ATTN=0: none is).  The 8-bit routes first turn the
        layer's new tokens 8-bit (kv_quantize_tokens); only `gather` builds anything of the full length."""
        if any(c[0]._seq.rotating for c in caches):
            raise NotImplementedError("max_kv_size: a multi-token update of a non-empty rotating cache (the reference first trims "
                                      "the window to max_size - 1 + S, cache.py:486-505) is not built; only the first prompt")
        t, dev, pool = self.args, self.device, self.pool
        hd, Hq, Hkv = self.head_dim, t.num_attention_heads, t.num_key_value_heads
        seqs = [c[0]._seq for c in caches]
        # A mix of 8-bit and bf16 sequences is refused as in decode_run
        if len({bool(s.q8) for s in seqs}) > 1:
            raise RuntimeError("a prompt chunk cannot mix sequences with and without a quantized KV cache")
        q8 = bool(seqs[0].q8)
        if q8 and any(getattr(s, "q8_batch_policy", False) for s in seqs):
            raise NotImplementedError("a prompt chunk onto a sequence quantised under the BATCH policy (the last layer of a deep "
                                      "stack stays bf16, models/cache.py:8-21): only its decode steps are built")
        offs = [int(s.offset) for s in seqs]
        for n, s in zip(lengths, seqs):
            s.reserve(s.offset + n + reserve_extra)
        T, S = int(sum(lengths)), len(seqs)
        short = T <= 64 and os.environ.get("VLM_ONTO_CACHE_DECODE_ATTN") != "0"
        if paged_attn:
            if q8 or hd != 128:
                raise NotImplementedError("paged_attn: the paged prefill attention is built for bf16 caches with 128-wide heads")
            route = "paged"
        elif q8:
            route = "q8_decode" if short else "q8_paged"
        else:
            route = "decode" if short else "gather"

        # every route: where the chunk's K / V go (new_seq, new_slot) and the segments of the launch, in ONE upload
        bt = pool.block_table
        seg_seq = np.asarray([s.seq for s in seqs], dtype=np.int32)
        new_slot = np.concatenate([o + np.arange(n, dtype=np.int32) for o, n in zip(offs, lengths)])
        cu_new = np.concatenate([[0], np.cumsum(lengths)])
        pos_d = _lib.h2d(np.ascontiguousarray(position_ids, dtype=np.int32), dev)
        meta = _lib.h2d(np.concatenate([np.repeat(seg_seq, lengths), new_slot, cu_new, seg_seq, offs]).astype(np.int32), dev)
        new_seq_d, new_slot_d, cu_new_d, seg_seq_d, q_start_d = meta.split([T, T, S + 1, S, S])
        scale = float(getattr(t, "attn_scale", 0.0) or 0.0) or hd ** -0.5

        def pools8(i, kp, vp):
            """QuantizedKVCache.update_and_fetch: layer i's new rows become 8-bit -> its 8-bit pools"""
            p8 = pool.kpool8[i], pool.vpool8[i], pool.ksb[i], pool.vsb[i]
            ops.kv_quantize_tokens(kp, vp, *p8, new_seq_d, new_slot_d, bt, Hkv, hd)
            return p8

        if route == "paged":
            nqb = int(sum((n + ops.PAGED_PREFILL_QBLOCK - 1) // ops.PAGED_PREFILL_QBLOCK for n in lengths))

            def attend(i, qkv, kp, vp):
                return ops.attn_prefill_paged(qkv, kp, vp, bt, seg_seq_d, cu_new_d, q_start_d, nqb, Hq, Hkv, hd, scale)
        elif route == "q8_paged":
            nqb8 = int(sum((n + ops.Q8_PREFILL_QBLOCK - 1) // ops.Q8_PREFILL_QBLOCK for n in lengths))

            def attend(i, qkv, kp, vp):
                return ops.attn_prefill_paged_q8(qkv, *pools8(i, kp, vp), bt, seg_seq_d, cu_new_d, q_start_d, nqb8, Hq, Hkv, hd, scale)
        elif route in ("decode", "q8_decode"):
            # every new token is a decode row over its sequence's pages with kv_len = cache length + its index + 1 (its K / V
            # are in the pages by then) - no gather of the prefix, and the keys are split over workgroups as in a decode step
            # (one 64-row query block per head walking 16k keys took ~0.4 ms per layer; profiles/r06_long_prompt_prefill.txt.
            # 8-bit: one wave of vlm_attn_prefill_paged_q8 walks all the keys of its 16 rows, the decode rows split them: 46
            # against 156 us at 32 rows onto 4096 tokens, profiles/q8_prefill_attn.txt)
            bt_rows = bt[new_seq_d.long()].contiguous()
            row_len_d = new_slot_d + 1
            longest = max(o + n for o, n in zip(offs, lengths))
            dec_nsplit = 1 if longest <= 2048 else max(2, min(32, (longest + 16 * PAGE - 1) // (16 * PAGE)))

            if q8:
                def attend(i, qkv, kp, vp):
                    return ops.attn_decode_paged_q8(qkv, kp, vp, *pools8(i, kp, vp), bt_rows, row_len_d, 0, Hq, Hkv, hd, scale,
                                                    dec_nsplit, quantize_new=False)
            else:
                def attend(i, qkv, kp, vp):
                    return ops.attn_decode_paged(qkv, kp, vp, bt_rows, row_len_d, 0, Hq, Hkv, hd, scale, dec_nsplit)
        else:
            # gather: per layer the cached k / v rows are fetched back into a token-major buffer of per sequence [prefix | chunk]
            # rows and the varlen causal attention runs with each segment's query rows starting at its cache length (q_start:
            # the prefix rows are keys only)
            tot = [o + n for o, n in zip(offs, lengths)]
            cu_full = np.concatenate([[0], np.cumsum(tot)])
            Tf, QKV = int(cu_full[-1]), (Hq + 2 * Hkv) * hd
            new_rows_d = _lib.h2d(np.concatenate([np.arange(cu_full[i] + offs[i], cu_full[i + 1]) for i in range(S)]).astype(np.int64),
                                  dev)
            full_slot = np.concatenate([np.arange(n, dtype=np.int32) for n in tot])
            seq_d, slot_d, cu_d = _lib.h2d(np.concatenate([np.repeat(seg_seq, tot), full_slot, cu_full]).astype(np.int32),
                                           dev).split([Tf, Tf, S + 1])
            nqb, q_start = int(sum((n + 127) // 128 for n in lengths)), q_start_d      # query blocks: the chunk rows only
            if os.environ.get("VLM_ONTO_CACHE_QSTART") == "0":     # A/B knob: the form of rounds 3-5 (the prefix rows carry zero queries)
                nqb, q_start = int(sum((n + 127) // 128 for n in tot)), None
            new_full = torch.empty if q_start is not None else torch.zeros      # (q_start: the q columns of the prefix rows are never read)

            def attend(i, qkv, kp, vp):
                full = new_full(Tf, QKV, dtype=torch.bfloat16, device=dev)
                full[new_rows_d] = qkv
                if Tf > T:
                    # ONE gather over every row of the buffer, straight into it: the chunk's rows re-read from the pages what
                    # mrope_kvwrite_ just stored there (the same bits) - no prefix buffer, no second copy of Tf rows
                    ops.kv_gather_(full, Hq, Hkv, hd, slot_d, bt, kp, vp, kv_seq=seq_d)
                attn = ops.attn_prefill(full, full[:, Hq * hd:], full[:, (Hq + Hkv) * hd:], cu_d, nqb, Hq, Hkv, hd, scale, True,
                                        q_start=q_start)
                return attn[new_rows_d].contiguous()

        h = inputs_embeds.contiguous().clone()
        ds = self._deepstack_device(deepstack, T)
        inv_tab = self._w["inv_freq"][hd // 2:] if getattr(self, "_prefill_rope_long", False) else self._w["inv_freq"]   # SuScaledRoPE regime of this call
        for i in range(t.num_hidden_layers):
            w = self._layer_weights(i)
            kp, vp = pool.kpool[i], pool.vpool[i]          # this layer's K / V pools (flat views)
            xn = ops.rmsnorm(h, w[f"{i}.ln1"], t.rms_norm_eps)
            bqkv = w[f"{i}.bqkv"]
            qkv = ops.gemm(xn, w[f"{i}.wqkv"], bias=bqkv, epilogue=ops.EPI_BIAS if bqkv is not None else ops.EPI_NONE)
            self._rope_kvwrite(i, qkv, pos_d, inv_tab, new_seq_d, new_slot_d, bt, kp, vp)
            h = ops.gemm(attend(i, qkv, kp, vp), w[f"{i}.wo"], res=h, epilogue=ops.EPI_RESIDUAL)
            xn = ops.rmsnorm(h, w[f"{i}.ln2"], t.rms_norm_eps)
            act = ops.gemm(xn, w[f"{i}.wgu"], epilogue=ops.EPI_SWIGLU)
            h = ops.gemm(act, w[f"{i}.wdown"], res=h, epilogue=ops.EPI_RESIDUAL)
            if ds is not None and i < ds[0].shape[0]:
                ops.add_rows_(ds[0][i], ds[1], h)          # DeepStack: the chunk's image rows (reference language.py:231-283)
        rows = (cu_new[1:] - 1) if logits_rows == "last" else np.arange(T)
        xl = ops.rmsnorm(h[_lib.h2d(rows.astype(np.int64), dev)].contiguous(), self._w["norm"], t.rms_norm_eps)
        logits = ops.gemm(xl, dense(self._w["head"]))[:, : t.vocab_size]      # (the head is dequantised once, here)
        for n, s in zip(lengths, seqs):
            s.offset += n
        return logits

    # ------------------------------------------------------------------ fused_greedy_decode (reference hook)
    def supports_fused_greedy_logits_processors(self, processors) -> bool:
        """reference ar.py:1023-1031: Python logits processors cannot run inside the captured step"""
        return False

    def fused_greedy_decode(self, inputs, cache=None, **kwargs):
        """The reference's plug point for a native greedy decode step (generate/ar.py:1015-1042: GenerationBatch calls
        `language_model.fused_greedy_decode(inputs[:, None], cache=prompt_cache, **fwd_kwargs)` and falls back to the
        module call when it returns None): feed one token per row, run the whole step on the device - layers, lm_head,
        log-softmax, argmax, cache / position advance - and return the sampled token ids [B] without a host round trip.
        Returns None (= fall back) for anything the captured step does not cover."""
        if cache is None or kwargs.get("logits_processors"):
            return None
        ids = _to_np(inputs).reshape(-1)
        B = int(ids.size)
        caches = [cache] if isinstance(cache[0], KVCache) else cache
        if B not in (1, 2, 4, 8) or len(caches) != B or any(c[0].offset == 0 for c in caches):
            return None
        if any(c[0]._seq.rotating for c in caches):       # max_kv_size: the host makes room before every step (the module call)
            return None
        deltas = self._rope_deltas if self._rope_deltas is not None else np.zeros((B, 1), dtype=np.int64)
        deltas = np.broadcast_to(np.asarray(deltas).reshape(-1, 1), (B, 1)) if np.asarray(deltas).size == 1 else np.asarray(deltas)
        try:
            st = self.decode_begin(caches, ids, deltas[:B], max_new_tokens=1)
        except RuntimeError:          # rows not on consecutive block-table rows: let the caller use the module call
            return None
        self.decode_run(st, 1, dict(temperature=0.0, top_p=1.0, min_p=0.0, top_k=0, seed=0))
        return st.tok[:B].clone()

    # ------------------------------------------------------------------ decode
    def decode_state(self, B: int) -> DecodeState:
        st = self._decode_states.get(B)
        if st is None:
            st = DecodeState(self, B)
            self._decode_states[B] = st
        return st

    # max_kv_size: the family's rule for the rope offset of a decode step over a RotatingKVCache.  The reference's Qwen2-VL reads
    # `cache[0]._idx` - the ring's WRITE INDEX - where the cache has one (qwen2_vl/language.py:426-431), so after the first wrap
    # a token's rope position is its ring index; the plain-rope families read `cache.offset` (llava_bunny/language.py:65-66,
    # idefics2/language.py:54-55, phi3_v/phi3_v.py:82-83)
    ROTATING_POS_FROM_RING = True
    # does the family's reference prefill a prompt longer than max_kv_size under the rotating cache's WINDOWED mask (it passes
    # cache[0] to create_attention_mask: phi3_v.py:163) instead of the plain causal one (cache list: Qwen2-VL, Bunny)?
    ROTATING_PROMPT_WINDOW_MASK = False

    def _rotate_windows(self, seqs) -> np.ndarray:
        """Before a one-token step over sequences with max_kv_size: read each one's rope offset (BEFORE the ring wraps, as the
        reference's forward does), then make room as RotatingKVCache._update_in_place would (cache.py:507-547) - the moves of
        PagedSequence.rotate_plan in one vlm_kv_move_tokens launch.  -> rope offsets int32 [B]"""
        if any(s.q8 for s in seqs if s.rotating):
            raise NotImplementedError("RotatingKVCache Quantization NYI")          # (the reference's own words, cache.py:583-584)
        rope_pos = np.array([(s.rope_offset if self.ROTATING_POS_FROM_RING else s.offset) for s in seqs], dtype=np.int32)
        rows, src, dst = [], [], []
        for s in seqs:
            plan = s.rotate_plan()
            if plan:
                rows += [s.seq] * len(plan[0])
                src += list(plan[0])
                dst += list(plan[1])
        if rows:
            pool = self.pool
            dev = _lib.h2d(np.array([rows, src, dst], dtype=np.int32), self.device)
            check(_lib.lib().vlm_kv_move_tokens(pool.kpool.data_ptr(), pool.vpool.data_ptr(), pool.layer_stride, pool.n_layers,
                                                dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(rows),
                                                pool.block_table.data_ptr(), pool.max_pages, pool.n_kv_heads, pool.head_dim,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "kv_move_tokens")
            self._keep_rot = dev
        return rope_pos

    def supports_window_decode(self) -> bool:
        """can a decode step of this model run in window mode (_lib.DECODE_WINDOW)?  Not with two rope tables: that qkv epilogue
        derives the long-factor regime from the rows' cache offsets, which the window's slot no longer is (Phi-3.5-vision)"""
        return not int(getattr(self, "rope_long_from", 0) or 0)

    def _window_begin(self, seqs):
        """Rows with max_kv_size enter (or continue on) the device-resident window: at most ONE vlm_kv_move_tokens call for the
        rows whose first prompt was longer than the window (models/cache.py::window_start).  -> (M, K, ring_pos)"""
        if not all(s.rotating for s in seqs) or len({(s.max_size, s.keep) for s in seqs}) != 1:
            raise NotImplementedError("max_kv_size: the rows of one decode step share one window (max_kv_size, keep)")
        if any(s.q8 for s in seqs):
            raise NotImplementedError("RotatingKVCache Quantization NYI")          # (the reference's own words, cache.py:583-584)
        if not self.supports_window_decode() or len(seqs) not in (1, 2, 4, 8):
            raise NotImplementedError("max_kv_size: the captured window step is built for 1 / 2 / 4 / 8 rows of a one-table rope "
                                      "model; this one runs through the module call, one step at a time")
        if any(s.ring is not None for s in seqs):
            raise NotImplementedError("max_kv_size: the captured step writes at the ring slot of the device-resident window; a "
                                      "window that already wrapped through module calls (LanguageModel.__call__) stays on them")
        rows, src, dst = [], [], []
        for s in seqs:
            a, d = s.window_enter()
            rows += [s.seq] * len(a)
            src += a
            dst += d
        if rows:
            pool = self.pool
            dev = _lib.h2d(np.array([rows, src, dst], dtype=np.int32), self.device)
            check(_lib.lib().vlm_kv_move_tokens(pool.kpool.data_ptr(), pool.vpool.data_ptr(), pool.layer_stride, pool.n_layers,
                                                dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(rows),
                                                pool.block_table.data_ptr(), pool.max_pages, pool.n_kv_heads, pool.head_dim,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "kv_move_tokens")
            self._keep_rot = dev
        return (seqs[0].max_size, seqs[0].keep, int(bool(self.ROTATING_POS_FROM_RING)))

    def _set_window_mode(self, window):
        """the handle's mode values of a window step (vlm_llm_set_tuning keys 16..18); a change drops the engine's graphs"""
        if getattr(self, "_window_mode", (0, 0, 0)) != tuple(window):
            for k, v in zip((_lib.MODE_WINDOW_SIZE, _lib.MODE_WINDOW_KEEP, _lib.MODE_WINDOW_RING_POS), window):
                check(_lib.lib().vlm_llm_set_tuning(self._handle, k, int(v)), "llm_set_tuning")
            self._window_mode = tuple(window)
            for st in self._decode_states.values():
                st.graph_key = None

    def decode_begin(self, caches: List[List[KVCache]], first_tokens, rope_deltas, max_new_tokens: int, rope_pos=None) -> DecodeState:
        """Bind B sequences (B in {1,2,4,8}) to the device decode state: tok = first sampled tokens,
        ctx = cache offsets, pos = offset + rope_delta (reference language.py:476-509)."""
        B = len(caches)
        st = self.decode_state(B)
        seqs = [c[0]._seq for c in caches]
        for s in seqs:
            s.reserve(s.offset + max_new_tokens + 1)
        # max_kv_size without `rope_pos` (the caller did not make room on the host): the rows go to - or continue on - the
        # device-resident window, where a decode step advances the ring itself
        st.window = self._window_begin(seqs) if rope_pos is None and any(s.rotating for s in seqs) else None
        # attention decomposition for this generation: up to 2048 tokens one workgroup per (sequence, kv head)
        # walks the pages itself (nsplit = 1, no merge pass); beyond that, split-K with one workgroup per
        # page-stride (<= 32 splits) merged in the o_proj prologue
        max_total = max(s.kv_entries for s in seqs) + max_new_tokens + 1
        if st.window is not None:            # (a window never holds more than max_kv_size entries)
            max_total = min(max_total, st.window[0])
        st.nsplit = 1 if max_total <= 2048 else max(2, min(32, (max_total + 16 * PAGE - 1) // (16 * PAGE)))
        if os.environ.get("VLM_DECODE_NSPLIT"):     # A/B knob for measurements
            st.nsplit = max(1, min(32, int(os.environ["VLM_DECODE_NSPLIT"])))
        # the engine indexes block-table rows by batch row: sequences must sit in rows 0..B-1 of a view
        rows = [s.seq for s in seqs]
        if rows != list(range(rows[0], rows[0] + B)):
            raise RuntimeError("decode batch needs consecutive KV sequence slots")
        st.seq_row0 = rows[0]
        # (a rotating window: entries held, not tokens seen; the rope offset is the family's - `rope_pos` when the caller read it
        # before the window wrapped, LanguageModel.__call__)
        ctx = np.array([s.kv_entries for s in seqs], dtype=np.int32)
        if rope_pos is not None:
            base = np.asarray(rope_pos, dtype=np.int32)
        elif st.window is not None and st.window[2]:
            base = np.array([s.ring_idx for s in seqs], dtype=np.int32)
        else:
            base = np.array([s.offset for s in seqs], dtype=np.int32)
        delta = np.asarray(rope_deltas, dtype=np.int64).reshape(-1).astype(np.int32)
        pos = base + delta
        slot = np.array([s.win_w for s in seqs], dtype=np.int32) if st.window is not None else ctx
        host = np.concatenate([pos, delta, ctx, slot, np.zeros(1, np.int32)])
        dev = _lib.h2d(host, self.device)
        st.pos2.view(-1).copy_(dev[:2 * B]); st.ctx2.view(-1).copy_(dev[2 * B:4 * B]); st.step.copy_(dev[4 * B:])
        if isinstance(first_tokens, torch.Tensor):
            st.tok.copy_(first_tokens.reshape(-1).to(torch.int32))
        else:
            st.tok.copy_(_lib.h2d(np.asarray(first_tokens, dtype=np.int32).reshape(-1), self.device))
        st.seqs = seqs
        # a fused-tail step starts from h == embed[tok] (vlm_decode_args.flags); every later h is left behind by the
        # previous step's sampler tail
        if not hasattr(self._w["embed"], "wq"):
            ops.embed_gather(st.tok[:B], self._w["embed"], out=st.h[:B])
        return st

    # ------------------------------------------------------------------ uniform 8-bit KV cache
    def quantize_kv(self, seqs, bits: int = 8, group_size: int = 64):
        """KVCache.to_quantized (reference cache.py:415-423) for whole sequences: every cached token of `seqs` (all layers) is
        quantised from the bf16 pools into the 8-bit pools (mx.quantize, group 64, 8 bits); from then on their decode steps
        attend over the 8-bit pools and quantise each new token (QuantizedKVCache.update_and_fetch, cache.py:233-334)."""
        if int(bits) != 8 or int(group_size) != 64:
            raise NotImplementedError(f"quantized KV cache: kv_bits = 8 with kv_group_size = 64 is built (asked: {bits} / {group_size})")
        seqs = [s for s in seqs if not s.q8]
        if not seqs:
            return
        pool = self.pool.ensure_q8()
        rows = np.concatenate([np.full(s.offset, s.seq, dtype=np.int32) for s in seqs]) if seqs else np.zeros(0, np.int32)
        slots = np.concatenate([np.arange(s.offset, dtype=np.int32) for s in seqs])
        if rows.size:
            dev = _lib.h2d(np.stack([rows, slots]), self.device)
            check(_lib.lib().vlm_kv_quantize_tokens(pool.kpool.data_ptr(), pool.vpool.data_ptr(), pool.kpool8.data_ptr(),
                                                    pool.vpool8.data_ptr(), pool.ksb.data_ptr(), pool.vsb.data_ptr(),
                                                    pool.layer_stride, pool.n_layers, dev[0].data_ptr(), dev[1].data_ptr(),
                                                    int(rows.size), pool.block_table.data_ptr(), pool.max_pages, pool.n_kv_heads,
                                                    pool.head_dim, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "kv_quantize_tokens")
            self._keep_q8 = dev
        for s in seqs:
            s.q8 = True

    def _kv_struct(self, row0: int, decode: bool = False, q8: bool = False):
        """The pool as the engine sees it for batch rows row0, row0+1, ...  Decode over an identity-layout pool:
        no block table (NULL) and pool pointers advanced to row0's region - the kernels compute
        page = row * max_pages + index instead of loading it."""
        pool = self.pool
        if decode and pool.identity:
            elems = row0 * pool.max_pages * pool.n_kv_heads * PAGE * pool.head_dim
            off = elems * pool.kpool.element_size()
            q = (pool.kpool8.data_ptr() + elems, pool.vpool8.data_ptr() + elems, pool.ksb.data_ptr() + elems // 64 * 4,
                 pool.vsb.data_ptr() + elems // 64 * 4) if q8 else (None, None, None, None)
            return _lib.KvPool(pool.kpool.data_ptr() + off, pool.vpool.data_ptr() + off, pool.layer_stride, None,
                               pool.max_pages, *q)
        bt = pool.block_table[row0:]
        q = (pool.kpool8.data_ptr(), pool.vpool8.data_ptr(), pool.ksb.data_ptr(), pool.vsb.data_ptr()) if q8 else (None,) * 4
        return _lib.KvPool(pool.kpool.data_ptr(), pool.vpool.data_ptr(), pool.layer_stride, bt.data_ptr(), pool.max_pages, *q)

    def decode_run(self, st: DecodeState, n_steps: int, sampler_args: dict, use_graph: bool = True, penalties=None,
                   host_ring: bool = False, with_logprobs: bool = True):
        """Enqueue n_steps decode steps (graph replays when use_graph).  penalties: sample_utils.LogitsProcessors, or "rows":
        the state's per-row tables (row_penalty_tables - what a token bitmask travels in).  host_ring: the steps write their
        tokens into st.host_ring (pinned; slot = sampling step % ring_len) instead of st.out_ring - the caller reads them
        there behind an event and enqueues no copy of st.tok.  with_logprobs=False: a greedy step without penalties leaves
        st.logprobs alone (the tail gets no log-prob pointer and stores no row); sampled steps and steps with penalties
        write the row whatever is asked."""
        L = _lib.lib()
        if st.window is None and any(s.rotating for s in st.seqs):
            raise NotImplementedError("max_kv_size: the captured step writes at slot = tokens seen; a rotating window runs "
                                      "through the module call (LanguageModel.__call__), one step at a time")
        if st.window is not None:
            if any(s.win_w is None for s in st.seqs):
                raise RuntimeError("decode_run: the state's rows left the device-resident window (decode_begin binds them)")
            self._set_window_mode(st.window)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        q8 = self._seqs_q8(st.seqs)
        kv = self._kv_struct(st.seq_row0, decode=True, q8=q8)
        check(L.vlm_llm_set_kv(self._handle, C.byref(kv)), "llm_set_kv")
        # the fused tails (greedy: vlm_sample_greedy_advance; with a temperature: the sampler's last launch also advances and
        # gathers) read bf16 embedding rows
        fused = bool(self.tuning.get("fused_tail")) and not hasattr(self._w["embed"], "wq")
        flags = ((_lib.DECODE_FUSED_TAIL if fused else 0) | (_lib.DECODE_WINDOW if st.window is not None else 0) |
                 (_lib.DECODE_HOST_RING if host_ring else 0))
        # a one-row greedy step at a short context (gemv_variant bit 11): attention and o_proj over 4 / 8 / 12 splits instead of
        # 16 - the smallest class whose splits still own at most one page each at the LAST step enqueued here (64 S >= ctx + 1;
        # the host knows the context: every step advances it by one), so the bytes are those of 16.  Beyond 768 tokens, in a
        # window and over the 8-bit pools nothing changes.  The class is part of the engine's graph key: one captured step each.
        if (st.B == 1 and fused and st.window is None and not q8 and st.nsplit == 1 and (int(self.tuning["gemv_variant"]) & 2048)
                and float(sampler_args.get("temperature", 0.0)) == 0.0):
            split_class = (st.seqs[0].kv_entries + n_steps + 255) // 256
            if split_class <= 3:
                flags |= split_class << _lib.DECODE_SPLITS_SHIFT
        # ... or over exactly as many splits as that context has pages (gemv_variant bit 12, up to 1024 tokens; the engine lets
        # the count win over the class): no attention workgroup without a page, no dead slot ahead of the o_proj's weights.  A
        # run of steps that crosses a page boundary takes the count of its last step - the page the first ones do not reach
        # yet reports m = -inf and is dropped.  One captured step per count, cached in the engine across requests.
        if (st.B == 1 and fused and st.window is None and not q8 and st.nsplit == 1 and (int(self.tuning["gemv_variant"]) & 4096)
                and float(sampler_args.get("temperature", 0.0)) == 0.0):
            n_pages = (st.seqs[0].kv_entries + n_steps + 63) // 64
            if n_pages <= 16:
                flags |= n_pages << _lib.DECODE_NSPLITS_SHIFT
        with_logprobs = bool(with_logprobs) or penalties is not None
        args = st.args(flags=flags, penalties=penalties, with_logprobs=with_logprobs, **sampler_args)
        if os.environ.get("VLM_NO_GRAPH"):           # diagnostics: every launch of the step visible to the HIP runtime's log
            use_graph = False
        if use_graph:
            key = (st.seq_row0, st.nsplit, fused, bool(host_ring), with_logprobs, q8, st.window,
                   flags & (_lib.DECODE_SPLITS_MASK | _lib.DECODE_NSPLITS_MASK),
                   penalties if isinstance(penalties, str) else penalties.key() if penalties else None,
                   tuple(sorted(sampler_args.items())))
            if st.graph_key != key or getattr(self, "_graph_owner", None) is not st:
                check(L.vlm_llm_decode_graph_build(self._handle, C.byref(args), stream), "decode_graph_build")
                st.graph_key = key
                self._graph_owner = st
            for _ in range(n_steps):
                check(L.vlm_llm_decode_graph_launch(self._handle, stream), "decode_graph_launch")
        else:
            for _ in range(n_steps):
                check(L.vlm_llm_decode_step(self._handle, C.byref(args), stream), "decode_step")
        for s in st.seqs:
            s.offset += n_steps
            if st.window is not None:       # the device advanced (n, w, p) itself; the host's mirror follows from the rule alone
                s.window_advance(n_steps)

    @staticmethod
    def _seqs_q8(seqs) -> bool:
        flags = {bool(getattr(s, "q8", False)) for s in seqs}
        if len(flags) > 1:
            raise RuntimeError("a decode step cannot mix sequences with and without a quantized KV cache")
        return bool(flags) and flags.pop()

    def decode_step_rows(self, st: DecodeState, B: int, block_table: torch.Tensor, sampler_args: dict,
                         use_graph: bool = True, with_logprobs: bool = True, row_penalties: bool = False, q8: bool = False,
                         row_sampler: bool = False):
        """One decode step over rows 0..B-1 of `st` (B in {1, 2, 4, 8}), addressing the KV pool through the caller's own
        `block_table` (int32 [>= B, max_pages]).  A continuous batch keeps such a table so that a sequence changes
        batch row by copying one table row - no KV bytes move (the reference's `filter`/`extend` copy the caches,
        cache.py:1100-1201).  Graphs are cached per (B, nsplit, table, sampler) inside the engine.
        row_sampler: the tail draws every row with its own line of st.sample_ws (ops.sample_row_table; _lib.DECODE_ROW_SAMPLER) -
        `sampler_args` are then not read by the step."""
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pool = self.pool
        q = (pool.kpool8.data_ptr(), pool.vpool8.data_ptr(), pool.ksb.data_ptr(), pool.vsb.data_ptr()) if q8 else (None,) * 4
        # the BATCH policy of the reference (models/cache.py:8-21, generate/ar.py:842-858): with kv_bits the last layer of a
        # stack deeper than 2 keeps its unquantised cache (vlm_kv_pool.q8_skip_last; the bf16 pools hold every token anyway)
        kv = _lib.KvPool(pool.kpool.data_ptr(), pool.vpool.data_ptr(), pool.layer_stride, block_table.data_ptr(),
                         pool.max_pages, *q, 1 if q8 else 0)
        check(L.vlm_llm_set_kv(self._handle, C.byref(kv)), "llm_set_kv")
        # row_penalties: the step applies every row's own logits processors (device tables of the state) before sampling
        if row_sampler:
            args = st.args(B=B, with_logprobs=True, penalties="rows" if row_penalties else None, flags=_lib.DECODE_ROW_SAMPLER)
        else:
            args = st.args(B=B, with_logprobs=with_logprobs, penalties="rows" if row_penalties else None, **sampler_args)
        if use_graph:
            key = ("rows", B, st.nsplit, block_table.data_ptr(), with_logprobs, bool(row_penalties), bool(q8),
                   "row_sampler" if row_sampler else tuple(sorted(sampler_args.items())))
            if st.graph_key != key or getattr(self, "_graph_owner", None) is not st:
                check(L.vlm_llm_decode_graph_build(self._handle, C.byref(args), stream), "decode_graph_build")
                st.graph_key = key
                self._graph_owner = st
            check(L.vlm_llm_decode_graph_launch(self._handle, stream), "decode_graph_launch")
        else:
            check(L.vlm_llm_decode_step(self._handle, C.byref(args), stream), "decode_step")

    def decode_forward_rows(self, st: DecodeState, B: int, block_table: torch.Tensor, q8: bool = False):
        """The forward half of decode_step_rows, eager: logits of rows 0..B-1 land in st.logits; nothing is sampled, nothing
        advanced (vlm_llm_decode_forward).  The caller finishes the step with its own processors / sampler and
        decode_advance_rows - the route for Python callables, which cannot live inside a captured step."""
        L = _lib.lib()
        pool = self.pool
        q = (pool.kpool8.data_ptr(), pool.vpool8.data_ptr(), pool.ksb.data_ptr(), pool.vsb.data_ptr()) if q8 else (None,) * 4
        kv = _lib.KvPool(pool.kpool.data_ptr(), pool.vpool.data_ptr(), pool.layer_stride, block_table.data_ptr(),
                         pool.max_pages, *q, 1 if q8 else 0)
        check(L.vlm_llm_set_kv(self._handle, C.byref(kv)), "llm_set_kv")
        args = st.args(B=B)
        check(L.vlm_llm_decode_forward(self._handle, C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "decode_forward")

    def decode_advance_rows(self, st: DecodeState, B: int):
        """ctx += 1, pos += 1, token ring, sampling step counter of rows 0..B-1 (vlm_decode_advance): the tail of an eager step"""
        check(_lib.lib().vlm_decode_advance(st.ctx.data_ptr(), st.pos.data_ptr(), st.tok.data_ptr(), st.out_ring.data_ptr(),
                                            st.ring_len, st.step.data_ptr(), int(B),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "decode_advance")

    # ------------------------------------------------------------------ module contract (reference language.py:404-518)
    def __call__(self, inputs, inputs_embeds=None, mask=None, cache=None, **kwargs):
        position_ids = kwargs.pop("position_ids", None)
        pixel_values = kwargs.pop("pixel_values", None)
        image_grid_thw = kwargs.pop("image_grid_thw", None)
        video_grid_thw = kwargs.pop("video_grid_thw", None)
        rope_deltas_kw = kwargs.pop("rope_deltas", None)
        logits_to_keep = kwargs.pop("logits_to_keep", None)
        # DeepStack (Qwen3-VL; every other family's InputEmbeddingsFeatures carries None): full-prompt mask + per-layer embeds
        visual_pos_masks = kwargs.pop("visual_pos_masks", None)
        deepstack_visual_embeds = kwargs.pop("deepstack_visual_embeds", None)
        if pixel_values is not None:
            self._rope_deltas = None
            self._position_ids = None
        if rope_deltas_kw is not None:
            self._rope_deltas = _to_np(rope_deltas_kw)
        ids = _to_np(inputs)
        if ids.ndim == 1:
            ids = ids[None]
        B, Lq = ids.shape
        if cache is None:
            cache = self.make_cache()
            if B != 1:
                raise NotImplementedError("cache=None is only supported for B == 1")
        caches = [cache] if isinstance(cache[0], KVCache) else cache
        cache_offset = caches[0][0].offset

        # decode widths of the engine: 1 / 2 / 4 / 8 rows on the v_dot2c GEMVs, 9..16 rows on the skinny-M MFMA GEMM, 17..64 as
        # WIDE steps on the prefill GEMMs (these walk the pool's block table in either layout)
        if Lq == 1 and cache_offset > 0 and inputs_embeds is None and (B in (1, 2, 4, 8) or 9 <= B <= self.MAX_DECODE_ROWS):
            # decode: pos = cache offset + rope delta (language.py:476-509); logits only
            deltas = self._rope_deltas if self._rope_deltas is not None else np.zeros((B, 1), dtype=np.int64)
            deltas = np.broadcast_to(np.asarray(deltas).reshape(-1, 1), (B, 1)) if np.asarray(deltas).size == 1 else deltas
            rope_pos = None
            rot = [c[0]._seq for c in caches if c[0]._seq.rotating]
            # rows already on the device-resident window (a captured run came first) continue there: ONE window step through
            # vlm_llm_decode_forward from the host's mirror - one arrangement per sequence.  The others keep the host-planned ring
            on_device = any(s.win_w is not None for s in rot)
            saved = [(s, s.held, None if s.ring is None else list(s.ring), s.ring_idx, s.win_w) for s in rot]
            try:
                if rot and not on_device:
                    rope_pos = self._rotate_windows([c[0]._seq for c in caches])
                st = self.decode_begin(caches, ids.reshape(-1), deltas[:B], max_new_tokens=1, rope_pos=rope_pos)
                kv = self._kv_struct(st.seq_row0, decode=B <= 16, q8=self._seqs_q8(st.seqs))
                check(_lib.lib().vlm_llm_set_kv(self._handle, C.byref(kv)), "llm_set_kv")
                if st.window is not None:
                    self._set_window_mode(st.window)
                args = st.args(flags=_lib.DECODE_WINDOW if st.window is not None else 0)
                check(_lib.lib().vlm_llm_decode_forward(self._handle, C.byref(args),
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "decode_forward")
            except Exception:
                # the step did not get enqueued (slot rows, pool exhaustion, ...): the ring goes back to what it was, so a retry
                # plans the SAME move again (newest entry -> the slot of the token that leaves: idempotent on the pool)
                for s, held, ring, ring_idx, win_w in saved:
                    s.held, s.ring, s.ring_idx, s.win_w = held, ring, ring_idx, win_w
                raise
            for s in st.seqs:
                s.offset += 1
                if st.window is not None:
                    s.window_advance(1)
                else:
                    s.note_decode_step()
            return LanguageModelOutput(logits=st.logits.clone().view(B, 1, -1))

        # prefill path
        if position_ids is None:
            if self._position_ids is not None and cache_offset > 0:
                p = self._position_ids
                position_ids = p[..., cache_offset:cache_offset + Lq]
            else:
                position_ids, rope_deltas = self.get_rope_index(ids, image_grid_thw, video_grid_thw, _to_np(mask))
                self._rope_deltas = rope_deltas
                self._position_ids = position_ids
        pos = _to_np(position_ids)
        if pos.ndim == 2:
            pos = np.broadcast_to(pos[None], (3,) + pos.shape)
        if pos.shape[-1] > Lq:
            pos = pos[..., cache_offset:cache_offset + Lq]
        if inputs_embeds is None:
            inputs_embeds = self.embed_tokens(ids)
        emb = inputs_embeds.reshape(B * Lq, -1)
        pos_flat = pos.reshape(3, B * Lq)
        more = {}
        if deepstack_visual_embeds is not None:
            ds = deepstack_window(visual_pos_masks, deepstack_visual_embeds, cache_offset, Lq)
            if ds is not None:
                more["deepstack"] = ds
        logits = self.prefill(emb, pos_flat, caches, [Lq] * B, logits_rows="last" if logits_to_keep == 1 else "all", **more)
        if logits_to_keep == 1:
            return LanguageModelOutput(logits=logits.view(B, 1, -1))
        return LanguageModelOutput(logits=logits.view(B, Lq, -1))
