"""Qwen3-VL processor - host mirror of the reference's mlx_vlm/models/qwen3_vl/processing_qwen3_vl.py.

Its image processor (smart_resize, bicubic resize, rescale, normalise, the 10-D patch shuffle: 182-205, 302-354) IS the one
models/qwen2_vl restates as Qwen2VLImageProcessor - here with patch 16 and mean / std 0.5 unless preprocessor_config.json says
otherwise - and the placeholder expansion is the Qwen2-VL one.  Video inputs are out of scope; `return_mm_token_type_ids` as
for Qwen2.5-VL.
"""
from __future__ import annotations

from ..qwen2_5_vl.processing_qwen2_5_vl import Qwen2_5_VLProcessor
from ..qwen2_vl.processing_qwen2_vl import Qwen2VLImageProcessor


class Qwen3VLImageProcessor(Qwen2VLImageProcessor):
    """the reference's Qwen3VLImageProcessor defaults (processing_qwen3_vl.py:242-266): patch 16, merge 2, the pixel bounds of
    the Qwen2-VL processor, mean / std 0.5"""

    def __init__(self, patch_size: int = 16, temporal_patch_size: int = 2, merge_size: int = 2, min_pixels: int = 56 * 56,
                 max_pixels: int = 14 * 14 * 4 * 1280, **kwargs):
        super().__init__(patch_size=patch_size, temporal_patch_size=temporal_patch_size, merge_size=merge_size,
                         min_pixels=min_pixels, max_pixels=max_pixels, **kwargs)


class Qwen3VLProcessor(Qwen2_5_VLProcessor):
    def __call__(self, images=None, text=None, videos=None, **kwargs):
        if videos is not None:
            raise NotImplementedError("video inputs are outside the built hot path")
        return super().__call__(images=images, text=text, **kwargs)


__all__ = ["Qwen3VLImageProcessor", "Qwen3VLProcessor"]
