"""Qwen3-VL configuration objects for the drop-in module contract: field NAMES and DEFAULTS of the reference's
`mlx_vlm/models/qwen3_vl/config.py:30-127` (HF layout: `text_config` and `vision_config` both nested), generated from field
tables like models/qwen2_vl/config.py.
"""
from __future__ import annotations

import inspect
from dataclasses import field, make_dataclass
from typing import Any, Dict, List, Optional, Tuple

from ..base import BaseModelConfig
from ..qwen2_vl.config import _REQUIRED, _build

_LIST = object()            # default marker: a fresh list per object (a dataclass default_factory)
_ROPE = object()            # ... a fresh {"type": "default", "mrope_section": [24, 20, 20]}

_VISION: Tuple[Tuple[str, Any, Any], ...] = (
    ("model_type", str, "qwen3_vl"), ("depth", int, 32), ("hidden_size", int, 1280), ("intermediate_size", int, 3420),
    ("out_hidden_size", int, 1536), ("num_heads", int, 16), ("image_size", int, 384), ("patch_size", int, 14),
    ("vocab_size", int, 32000), ("mlp_ratio", float, 4.0), ("in_channels", int, 3), ("layer_norm_eps", float, 1e-6),
    ("spatial_patch_size", int, 14), ("spatial_merge_size", int, 2), ("tokens_per_second", int, 2),
    ("temporal_patch_size", int, 2), ("num_position_embeddings", int, 2304), ("window_size", int, 112),
    ("fullatt_block_indexes", List[int], _LIST), ("deepstack_visual_indexes", List[int], _LIST),
)
_TEXT: Tuple[Tuple[str, Any, Any], ...] = (
    ("model_type", str, _REQUIRED), ("num_hidden_layers", int, _REQUIRED), ("hidden_size", int, _REQUIRED),
    ("intermediate_size", int, _REQUIRED), ("num_attention_heads", int, _REQUIRED), ("rms_norm_eps", float, _REQUIRED),
    ("vocab_size", int, _REQUIRED), ("num_key_value_heads", Optional[int], _REQUIRED), ("head_dim", int, _REQUIRED),
    ("rope_theta", float, _REQUIRED), ("max_position_embeddings", int, _REQUIRED), ("norm_topk_prob", bool, True),
    ("rope_scaling", Optional[Dict[str, Any]], _ROPE), ("tie_word_embeddings", bool, False), ("attention_bias", bool, False),
    ("hidden_act", str, "silu"), ("use_final_norm", bool, True),
)
_MODEL: Tuple[Tuple[str, Any, Any], ...] = (
    ("text_config", Any, _REQUIRED), ("vision_config", Any, _REQUIRED), ("model_type", str, _REQUIRED),
    ("ignore_index", int, -100), ("image_token_id", int, 151655), ("video_token_id", int, 151656),
    ("image_token_index", Optional[int], None), ("video_token_index", Optional[int], None),
    ("vision_start_token_id", int, 151652), ("vision_end_token_id", int, 151653), ("vision_token_id", int, 151654),
    ("vision_feature_select_strategy", str, "default"), ("vision_feature_layer", int, -2), ("vocab_size", int, 32000),
    ("eos_token_id", Optional[List[int]], None), ("skip_vision", bool, False),
)


def _table_class(name, table, namespace=None):
    """_build with per-object defaults for the list / dict fields"""
    specs = []
    for n, t, d in table:
        if d is _REQUIRED:
            specs.append((n, t))
        elif d is _LIST:
            specs.append((n, t, field(default_factory=list)))
        elif d is _ROPE:
            specs.append((n, t, field(default_factory=lambda: {"type": "default", "mrope_section": [24, 20, 20]})))
        else:
            specs.append((n, t, field(default=d)))
    cls = make_dataclass(name, specs, bases=(BaseModelConfig,), namespace=namespace or {})
    cls.__module__ = __name__
    return cls


def _check_text(self):
    """reference config.py:76-90: GQA default, `rope_type` accepted for `type`, the M-RoPE description"""
    if self.num_key_value_heads is None:
        self.num_key_value_heads = self.num_attention_heads
    rs = self.rope_scaling
    if rs:
        if "type" not in rs and "rope_type" in rs:
            rs["type"] = rs.pop("rope_type")
        missing = {"mrope_section", "type"} - set(rs)
        if missing:
            raise ValueError(f"rope_scaling must contain keys {{'mrope_section', 'type'}} (missing {sorted(missing)})")
        if rs["type"] not in ("mrope", "default"):
            raise ValueError("rope_scaling type must be 'mrope' or 'default'")


def _check_model(self):
    if self.image_token_index is None:
        self.image_token_index = self.image_token_id
    if self.video_token_index is None:
        self.video_token_index = self.video_token_id


VisionConfig = _table_class("VisionConfig", _VISION)
TextConfig = _table_class("TextConfig", _TEXT, {"__post_init__": _check_text})


def _deserialize(cls, params, require_all_fields=False):
    """reference config.py:8-27: a dict becomes the class, restricted to its fields; a text_config that lacks a required field
    stays a dict (the reference's behaviour: construction of the language model then fails on it)"""
    if not isinstance(params, dict):
        return params
    sig = inspect.signature(cls).parameters
    if require_all_fields and not all(n in params for n, p in sig.items() if p.default is inspect.Parameter.empty):
        return params
    return cls(**{k: v for k, v in params.items() if k in sig})


def _model_from_dict(cls, params):
    params = dict(params)
    params["vision_config"] = _deserialize(VisionConfig, params.get("vision_config"))
    params["text_config"] = _deserialize(TextConfig, params.get("text_config"), require_all_fields=True)
    return cls(**{k: v for k, v in params.items() if k in inspect.signature(cls).parameters})


ModelConfig = _table_class("ModelConfig", _MODEL, {"from_dict": classmethod(_model_from_dict), "__post_init__": _check_model})

__all__ = ["ModelConfig", "TextConfig", "VisionConfig"]
