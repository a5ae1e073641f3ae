"""`models.internvl_chat` (InternVL3 / InternVL3.5): the reference's module contract for this model type
(mlx_vlm/models/internvl_chat/__init__.py)."""
from .config import ModelConfig, TextConfig, VisionConfig
from .internvl_chat import Model, pixel_shuffle_index
from .language import LanguageModel
from .processor import InternVLChatProcessor, InternVLImageProcessor
from .vision import VisionModel

__all__ = ["InternVLChatProcessor", "InternVLImageProcessor", "LanguageModel", "Model", "ModelConfig", "TextConfig", "VisionConfig",
           "VisionModel", "pixel_shuffle_index"]
