"""Qwen2.5-VL glue model on MI355X - host mirror of the reference's mlx_vlm/models/qwen2_5_vl/qwen2_5_vl.py.

`get_input_embeddings`, `merge_input_ids_with_image_features`, `encode_image`, `__call__` and `sanitize` of the reference's
file are those of its qwen2_vl.py line for line (20-76, 78-150, 156-182, 184-195), so the Qwen2-VL glue model is reused;
what differs is the vision tower (RMSNorm, biased SwiGLU, window attention: vision.py) and the configuration classes.
"""
from __future__ import annotations

from ..qwen2_vl.qwen2_vl import Model as _Qwen2VLModel
from . import processing_qwen2_5_vl  # noqa: F401
from .config import ModelConfig
from .language import LanguageModel
from .vision import VisionModel


class Model(_Qwen2VLModel):
    def __init__(self, config: ModelConfig, device="cuda", **engine_kwargs):
        self.config = config
        self.device = device
        self.vision_tower = VisionModel(config.vision_config, device=device)
        self.language_model = LanguageModel(config.text_config, config, device=device, **engine_kwargs)


__all__ = ["LanguageModel", "Model", "VisionModel"]
