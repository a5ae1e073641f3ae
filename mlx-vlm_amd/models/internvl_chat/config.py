"""InternVL3 / InternVL3.5 (`internvl_chat`) configuration objects: field names, defaults and `from_dict` behaviour of the
reference's `mlx_vlm/models/internvl_chat/config.py:7-90` (HF layout: `llm_config` is not read there - the converted checkpoints
carry `text_config` and `vision_config`; `image_size` / `patch_size` given as a list take their first entry).  Generated from
field tables like models/llava_bunny/config.py."""
from __future__ import annotations

import inspect
from dataclasses import field, make_dataclass
from typing import Any, Dict, List, Optional, Union

from ..base import BaseModelConfig

_REQ = object()

_VISION = (
    ("model_type", str, _REQ), ("hidden_size", int, 1024), ("num_attention_heads", int, 16), ("patch_size", int, 14),
    ("num_hidden_layers", int, 24), ("intermediate_size", int, 4096), ("image_size", int, 448), ("num_channels", int, 3),
    ("layer_norm_eps", float, 1e-6), ("drop_path_rate", float, 0.1), ("qkv_bias", bool, True),
    ("qk_normalization", bool, False), ("norm_type", str, "layer_norm"),
)
_TEXT = (
    ("model_type", str, _REQ), ("hidden_size", int, _REQ), ("num_hidden_layers", int, _REQ), ("intermediate_size", int, _REQ),
    ("num_attention_heads", int, _REQ), ("rms_norm_eps", float, _REQ), ("vocab_size", int, _REQ), ("hidden_act", str, "silu"),
    ("num_key_value_heads", Optional[int], 8), ("head_dim", Optional[int], None), ("max_window_layers", Optional[int], None),
    ("max_position_embeddings", Optional[int], 40960), ("rope_theta", float, 1000000.0), ("rope_traditional", bool, False),
    ("rope_scaling", Optional[Dict[str, Union[float, str]]], None), ("tie_word_embeddings", bool, False),
    ("attention_bias", bool, True), ("sliding_window", Optional[int], None), ("use_sliding_window", bool, False),
    ("use_cache", bool, True),
)
_MODEL = (
    ("text_config", Any, _REQ), ("vision_config", Any, _REQ), ("model_type", str, _REQ), ("ignore_index", int, -100),
    ("image_token_index", int, 151667), ("video_token_index", int, 151656), ("vision_feature_select_strategy", str, "default"),
    ("vision_feature_layer", int, -1), ("vocab_size", int, 32000), ("downsample_ratio", float, 0.5),
    ("eos_token_id", Optional[List[int]], None),
)


def _build(name, table, namespace=None):
    specs = [(n, t) if d is _REQ else (n, t, field(default=d)) for n, t, d in table]
    cls = make_dataclass(name, specs, bases=(BaseModelConfig,), namespace=namespace or {})
    cls.__module__ = __name__
    return cls


def _first_int(v):
    """config.py:25-35: `image_size: [448, 448]` -> 448"""
    if isinstance(v, (list, tuple)) and len(v) > 0:
        v = v[0]
    try:
        return int(v)
    except Exception:
        return v


def _vision_from_dict(cls, params):
    p = dict(params)
    for k in ("image_size", "patch_size"):
        if k in p:
            p[k] = _first_int(p[k])
    return cls(**{k: v for k, v in p.items() if k in inspect.signature(cls).parameters})


def _check_text(self):
    if self.num_key_value_heads is None:
        self.num_key_value_heads = self.num_attention_heads


VisionConfig = _build("VisionConfig", _VISION, {"from_dict": classmethod(_vision_from_dict)})
TextConfig = _build("TextConfig", _TEXT, {"__post_init__": _check_text})


def _model_from_dict(cls, params):
    raw = dict(params)
    cfg = cls(**{k: v for k, v in raw.items() if k in inspect.signature(cls).parameters})
    if isinstance(cfg.text_config, dict):
        cfg.text_config = TextConfig.from_dict(cfg.text_config)
    if isinstance(cfg.vision_config, dict):
        cfg.vision_config = VisionConfig.from_dict(cfg.vision_config)
    return cfg


ModelConfig = _build("ModelConfig", _MODEL, {"from_dict": classmethod(_model_from_dict)})

__all__ = ["ModelConfig", "TextConfig", "VisionConfig"]
