"""Qwen2.5-VL configuration objects for the drop-in module contract: field NAMES and DEFAULTS of the reference's
`mlx_vlm/models/qwen2_5_vl/config.py:8-90` (HF layout: text parameters at the root of `config.json`, `vision_config`
nested), generated from field tables like models/qwen2_vl/config.py.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

from ..qwen2_vl.config import _REQUIRED, _build, _check_text

_FULLATT = object()         # default marker: a fresh [7, 15, 23, 31] per object (a dataclass default_factory)

_VISION: Tuple[Tuple[str, Any, Any], ...] = (
    ("model_type", str, "qwen2_5_vl"), ("depth", int, 32), ("hidden_size", int, 1280), ("intermediate_size", int, 3420),
    ("out_hidden_size", int, 1536), ("num_heads", int, 16), ("image_size", int, 384), ("patch_size", int, 14),
    ("vocab_size", int, 32000), ("mlp_ratio", float, 4.0), ("in_channels", int, 3), ("layer_norm_eps", float, 1e-6),
    ("spatial_patch_size", int, 14), ("spatial_merge_size", int, 2), ("tokens_per_second", int, 2),
    ("temporal_patch_size", int, 2), ("window_size", int, 112), ("fullatt_block_indexes", List[int], _FULLATT),
)
_TEXT: Tuple[Tuple[str, Any, Any], ...] = (
    ("model_type", str, _REQUIRED), ("hidden_size", int, _REQUIRED), ("num_hidden_layers", int, _REQUIRED),
    ("intermediate_size", int, _REQUIRED), ("num_attention_heads", int, _REQUIRED), ("rms_norm_eps", float, _REQUIRED),
    ("vocab_size", int, _REQUIRED), ("num_key_value_heads", Optional[int], None),
    ("max_position_embeddings", Optional[int], 128000), ("rope_theta", float, 1000000.0),
    ("rope_traditional", bool, False), ("rope_scaling", Optional[Dict[str, Any]], None),
    ("tie_word_embeddings", bool, True),
)
_MODEL: Tuple[Tuple[str, Any, Any], ...] = (
    ("text_config", Any, _REQUIRED), ("vision_config", Any, _REQUIRED), ("model_type", str, _REQUIRED),
    ("ignore_index", int, -100), ("image_token_id", int, 151655), ("video_token_id", int, 151656),
    ("vision_start_token_id", int, 151652), ("vision_end_token_id", int, 151653), ("vision_token_id", int, 151654),
    ("vision_feature_select_strategy", str, "default"), ("vision_feature_layer", int, -2), ("vocab_size", int, 32000),
    ("eos_token_id", Optional[List[int]], None),
)


def _vision_fields():
    """every vision field has a default; `_FULLATT` stands for a list made per object"""
    from dataclasses import field, make_dataclass

    from ..base import BaseModelConfig

    specs = [(n, t, field(default_factory=lambda: [7, 15, 23, 31])) if d is _FULLATT else (n, t, field(default=d))
             for n, t, d in _VISION]
    cls = make_dataclass("VisionConfig", specs, bases=(BaseModelConfig,))
    cls.__module__ = __name__
    return cls


VisionConfig = _vision_fields()
TextConfig = _build("TextConfig", _TEXT, {"__post_init__": _check_text})
TextConfig.__module__ = __name__


def _model_from_dict(cls, params):
    """HF Qwen2.5-VL `config.json`: every root-level key except `vision_config` describes the language model
    (reference config.py:76-90)."""
    known = {n for n, _, _ in _MODEL}
    raw = dict(params)
    text = raw.get("text_config")
    if not text or not isinstance(text, (dict, TextConfig)):
        text = {k: v for k, v in raw.items() if k != "vision_config"}
    raw["text_config"] = text
    cfg = cls(**{k: v for k, v in raw.items() if k in known})
    if isinstance(cfg.text_config, dict):
        cfg.text_config = TextConfig.from_dict(cfg.text_config)
    if isinstance(cfg.vision_config, dict):
        cfg.vision_config = VisionConfig.from_dict(cfg.vision_config)
    return cfg


ModelConfig = _build("ModelConfig", _MODEL, {"from_dict": classmethod(_model_from_dict)})
ModelConfig.__module__ = __name__

__all__ = ["ModelConfig", "TextConfig", "VisionConfig"]
