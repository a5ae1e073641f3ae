"""Qwen2.5-VL processor - host mirror of the reference's mlx_vlm/models/qwen2_5_vl/processing_qwen2_5_vl.py.

The reference's file is its Qwen2-VL processor (same smart_resize / patchify image processor with patch 14, same
placeholder expansion) plus one option, `return_mm_token_type_ids` (123-133): 1 at image tokens, 2 at video tokens.  The image
processor and the expansion are reused from models/qwen2_vl; video stays out of scope as there.
"""
from __future__ import annotations

import numpy as np

from ..qwen2_vl.processing_qwen2_vl import Qwen2VLImageProcessor, Qwen2VLProcessor


class Qwen2_5_VLProcessor(Qwen2VLProcessor):
    def __init__(self, image_processor, tokenizer, image_token: str = "<|image_pad|>", video_token: str = "<|video_pad|>"):
        super().__init__(image_processor, tokenizer, image_token)
        self.video_token = getattr(tokenizer, "video_token", video_token)

    def _token_id(self, token):
        tid = self.tokenizer.convert_tokens_to_ids(token)
        return -1 if tid is None else int(tid)

    def __call__(self, images=None, text=None, **kwargs):
        want_types = kwargs.pop("return_mm_token_type_ids", None)
        out = super().__call__(images=images, text=text, **kwargs)
        if want_types:
            ids = out["input_ids"]
            types = np.zeros_like(ids)
            types[ids == self._token_id(self.image_token)] = 1
            types[ids == self._token_id(self.video_token)] = 2
            out["mm_token_type_ids"] = types.tolist()            # a list of lists, as the reference stores it (133)
        return out


__all__ = ["Qwen2VLImageProcessor", "Qwen2_5_VLProcessor"]
