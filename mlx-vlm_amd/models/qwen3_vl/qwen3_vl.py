"""Qwen3-VL glue model on MI355X - host mirror of the reference's mlx_vlm/models/qwen3_vl/qwen3_vl.py (Model:
get_input_embeddings with DeepStack features, merge_input_ids_with_image_features, sanitize, __call__).

Against the Qwen2-VL glue model: the tower returns (features, [tap features]); `get_input_embeddings` hands both the image-token
mask and the taps on as `visual_pos_masks` / `deepstack_visual_embeds` (44-133); `cached_image_features` means no DeepStack
(70-79: the reference's own rule - a vision-cache hit skips the tower, and the taps are not cached); `sanitize` maps the
`model.language_model.` / `model.visual.` layout (238-252).  Video and the MoE variant are refused.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ..base import InputEmbeddingsFeatures
from ..qwen2_vl.qwen2_vl import Model as _Qwen2VLModel
from . import processing_qwen3_vl  # noqa: F401
from .config import ModelConfig
from .language import LanguageModel, _to_np
from .vision import VisionModel


class Model(_Qwen2VLModel):
    def __init__(self, config: ModelConfig, device="cuda", **engine_kwargs):
        if str(config.model_type).lower() != "qwen3_vl":
            raise NotImplementedError(f"model_type {config.model_type}: the dense Qwen3-VL family is built (qwen3_vl_moe is not)")
        if getattr(config, "skip_vision", False):
            raise NotImplementedError("skip_vision: a Qwen3-VL model without its tower is not built")
        self.config = config
        self.device = device
        self.vision_tower = VisionModel(config.vision_config, device=device)
        self.language_model = LanguageModel(config.text_config, config, device=device, **engine_kwargs)

    # ------------------------------------------------------------------ reference qwen3_vl.py:44-133
    def get_input_embeddings(self, input_ids=None, pixel_values=None, **kwargs):
        if kwargs.get("pixel_values_videos") is not None or kwargs.get("video_grid_thw") is not None:
            raise NotImplementedError("video inputs are outside the built hot path")
        image_grid_thw = kwargs.get("image_grid_thw", None)
        mask = kwargs.get("mask", None)
        ids = _to_np(input_ids)
        lm = self.language_model
        if pixel_values is None:
            position_ids, rope_deltas = lm.get_rope_index(ids, attention_mask=mask)
            return InputEmbeddingsFeatures(inputs_embeds=lm.embed_tokens(ids), position_ids=position_ids, rope_deltas=rope_deltas)
        inputs_embeds = lm.embed_tokens(ids)
        cached = kwargs.get("cached_image_features", None)
        deepstack = None
        if cached is not None:
            feats = cached
        else:
            feats, taps = self.vision_tower(torch.as_tensor(pixel_values), _to_np(image_grid_thw))
            deepstack = torch.stack(taps) if taps else None
        final = self.merge_input_ids_with_image_features(self.config.image_token_index, self.config.video_token_index, feats,
                                                         inputs_embeds, ids)
        visual_pos_masks = (ids == self.config.image_token_index) | (ids == self.config.video_token_index)
        position_ids, rope_deltas = lm.get_rope_index(ids, image_grid_thw, None, mask)
        return InputEmbeddingsFeatures(inputs_embeds=final, visual_pos_masks=visual_pos_masks, deepstack_visual_embeds=deepstack,
                                       position_ids=position_ids, rope_deltas=rope_deltas)

    def encode_image(self, pixel_values, image_grid_thw=None, **kwargs):
        """Projected image features - what `cached_image_features` carries.  The DeepStack taps are not part of it: a
        vision-cache hit runs without DeepStack, as in the reference (qwen3_vl.py:70-79)."""
        return self.vision_tower(torch.as_tensor(pixel_values), _to_np(image_grid_thw))[0]

    def __call__(self, input_ids, pixel_values=None, mask=None, cache=None, **kwargs):
        f = self.get_input_embeddings(input_ids, pixel_values, mask=mask, **kwargs)
        kwargs = {**kwargs, "pixel_values": pixel_values, "position_ids": f.position_ids, "rope_deltas": f.rope_deltas,
                  "visual_pos_masks": f.visual_pos_masks, "deepstack_visual_embeds": f.deepstack_visual_embeds}
        return self.language_model(input_ids, f.inputs_embeds, mask=mask, cache=cache, **kwargs)

    def sanitize(self, weights: Dict[str, torch.Tensor]):
        """reference qwen3_vl.py:238-252"""
        out = {}
        for key, value in weights.items():
            if "model" in key:
                if "model.language_model" in key:
                    key = key.replace("model.language_model", "language_model.model")
                elif "model.visual" in key:
                    key = key.replace("model.visual", "vision_tower")
            elif "lm_head" in key:
                key = key.replace("lm_head", "language_model.lm_head")
            out[key] = value
        return out


__all__ = ["LanguageModel", "Model", "VisionModel"]
