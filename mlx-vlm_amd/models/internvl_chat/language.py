"""Language models of InternVL3 (Qwen2.5) and InternVL3.5 (Qwen3) on the decode / prefill engine - host mirror of the reference's
`mlx_vlm/models/internvl_chat/language.py` (Attention 17-90: q / k / v bias XOR per-head QK-norm, nn.RoPE rotate-half at the
cache offset; Qwen2VLDecoderLayer 93-116; Qwen2Model 119-155; LanguageModel 158-193).

Both forms are decoders the engine already runs; nothing here is a new kernel:

  * `attention_bias = True` (Qwen2.5): the plain-RoPE engine class of models/llava_bunny - biased q / k / v, heads narrower than
    128 (Qwen2.5-0.5B: 64) spread into 128-wide slots;
  * `attention_bias = False` (Qwen3; the reference switches the QK-norm on exactly then, language.py:40-43): the engine's
    VLM_MODE_QWEN3 through models/qwen3_vl's class - bias-free projections, RMSNorm(head_dim) on every q / k head, head_dim 128.

The reference's nn.RoPE is 1-D.  The engine rotates with M-RoPE; with the same position on all three axes every frequency sees
that position whichever axis its selector picks - the chunked selector of the Qwen2 form and the interleaved one of the Qwen3 form
alike - so positions are arange(L) on all axes and the rope delta is 0 (tests/test_internvl_cpu.py shows it on the restatement).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from ..llava_bunny.language import LanguageModel as _PlainRopeEngine
from ..qwen3_vl.language import LanguageModel as _Qwen3Engine
from .config import ModelConfig, TextConfig

SUPPORTED_TEXT_MODELS = ("qwen2", "qwen3")


def _plain_positions(input_ids):
    ids = np.asarray(input_ids)
    B, L = ids.shape
    pos = np.broadcast_to(np.arange(L, dtype=np.int64)[None, None], (3, B, L)).copy()
    return pos, np.zeros((B, 1), dtype=np.int64)


class Qwen2LanguageModel(_PlainRopeEngine):
    """InternVL3: Qwen2.5 decoder (biased q / k / v, no QK-norm)"""

    def __init__(self, args: TextConfig, config: ModelConfig, device="cuda", **engine_kwargs):
        if getattr(args, "head_dim", None) not in (None, args.hidden_size // args.num_attention_heads):
            raise NotImplementedError("a Qwen2-form language model with head_dim != hidden_size / num_attention_heads")
        super().__init__(args, config, device=device, **engine_kwargs)

    def load_weights(self, W):
        if self.real_head_dim != 128 and any(k.endswith("self_attn.q_proj.scales") for k in W):
            raise NotImplementedError(f"MLX 4-bit attention projections with head_dim {self.real_head_dim}: the spread into 128-wide "
                                      "slots is built for bf16 weights (the 2B / 8B / 14B decoders have 128-wide heads)")
        return super().load_weights(W)


class Qwen3LanguageModel(_Qwen3Engine):
    """InternVL3.5: Qwen3 decoder (no bias, QK-norm, explicit head_dim) on VLM_MODE_QWEN3"""
    DEEPSTACK = False
    ROTATING_POS_FROM_RING = False     # rope offset of a decode step over a rotating cache = cache.offset (the reference's own read)

    def __init__(self, args: TextConfig, config: ModelConfig, device="cuda", **engine_kwargs):
        if args.rope_traditional:
            raise NotImplementedError("rope_traditional (interleaved pairs) is outside the built path")
        hd = getattr(args, "head_dim", None) or args.hidden_size // args.num_attention_heads
        self.text_config = args
        eng = SimpleNamespace(model_type=args.model_type, hidden_size=args.hidden_size, num_hidden_layers=args.num_hidden_layers,
                              intermediate_size=args.intermediate_size, num_attention_heads=args.num_attention_heads,
                              num_key_value_heads=args.num_key_value_heads, rms_norm_eps=args.rms_norm_eps,
                              vocab_size=args.vocab_size, rope_theta=args.rope_theta, rope_scaling=None,
                              tie_word_embeddings=args.tie_word_embeddings, head_dim=hd, attention_bias=False)
        super().__init__(eng, config, device=device, **engine_kwargs)

    def get_rope_index(self, input_ids, image_grid_thw=None, video_grid_thw=None, attention_mask=None):
        return _plain_positions(input_ids)

    def sanitize(self, weights):
        return {k: v for k, v in weights.items() if "self_attn.rotary_emb.inv_freq" not in k}


def LanguageModel(args: TextConfig, config: ModelConfig, device="cuda", **engine_kwargs):
    """The engine class for `text_config.model_type`: qwen2 (attention bias) or qwen3 (QK-norm).  Everything else the family has
    been shipped with (internlm2 / internlm3, gpt-oss, the MoE decoders) is refused here, at load."""
    mt = str(args.model_type).lower()
    if mt not in SUPPORTED_TEXT_MODELS:
        raise NotImplementedError(f"internvl_chat with a {args.model_type} language model: qwen2 (InternVL3) and qwen3 "
                                  "(InternVL3.5 dense) are built")
    bias = bool(getattr(args, "attention_bias", True))
    if bias != (mt == "qwen2"):
        raise NotImplementedError(f"text_config.model_type {mt} with attention_bias = {bias}: the reference runs the QK-norm "
                                  "exactly when there is no bias; qwen2 with bias and qwen3 without are built")
    cls = Qwen2LanguageModel if mt == "qwen2" else Qwen3LanguageModel
    return cls(args, config, device=device, **engine_kwargs)


__all__ = ["LanguageModel", "Qwen2LanguageModel", "Qwen3LanguageModel", "SUPPORTED_TEXT_MODELS"]
