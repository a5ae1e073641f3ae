from .config import ModelConfig, TextConfig, VisionConfig
from .language import LanguageModel
from .qwen2_5_vl import Model
from .vision import VisionModel
