"""Qwen2.5-VL language model: the Qwen2-VL engine model, unchanged.

The reference's `mlx_vlm/models/qwen2_5_vl/language.py` differs from `qwen2_vl/language.py` in comments and in one line of
`Attention.__call__` (93: the position ids it MAKES when none are passed are tiled over the batch, `(3, B, 1)` instead of
`(3, 1, 1)`).  The engine model never takes that branch: its prefill always carries explicit position ids, broadcast over
the batch rows (models/qwen2_vl/language.py, `__call__`).  `get_rope_index` for images is the same function; video inputs
stay refused exactly as for Qwen2-VL.
"""
from ..qwen2_vl.language import DecodeState, LanguageModel, _to_np

__all__ = ["DecodeState", "LanguageModel", "_to_np"]
