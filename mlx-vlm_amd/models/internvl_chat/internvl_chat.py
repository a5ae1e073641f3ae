"""InternVL3 / InternVL3.5 glue model - host mirror of the reference's `mlx_vlm/models/internvl_chat/internvl_chat.py`
(Model 13-32, get_input_embeddings 34-86, _merge_input_ids_with_image_features 88-107) with the connector on the C-ABI kernels:

    tower rows [tiles * (1 + P), E]  -- drop CLS + pixel_shuffle: ONE row gather by a host-built table -->  [tiles * P r^2, E / r^2]
    mlp1 = LayerNorm(E / r^2) -> Linear + GELU(erf) -> Linear                     (vlm_layernorm, two GEMM epilogues)

`pixel_shuffle` (reference models/base.py:436-458) only moves whole token rows: output row j is the concatenation of 1 / r^2
source rows.  `pixel_shuffle_index` gets that table by running the reference's own reshape / transpose sequence over the token
numbers, and the CLS drop is folded into it (+ 1 + tile * (1 + P)), so the connector's input is made by vlm_embed_gather in one pass.

The image features replace the embeddings at the <IMG_CONTEXT> positions in order (the video token's positions when there are
none, as the reference).  Positions are plain (see language.py).  Checkpoint names need no remap (`vision_model.*`, `mlp1.{0,1,3}.*`,
`language_model.model.*`, `language_model.lm_head.*`); `sanitize` applies the tower's conv-layout fix and drops rotary tables.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from ... import _lib, ops
from ..base import InputEmbeddingsFeatures
from ..qwen2_vl.language import _to_np
from .config import ModelConfig
from .language import LanguageModel
from .vision import VisionModel

_V, _L, _M = "vision_model.", "language_model.", "mlp1."


def pixel_shuffle_index(num_patches: int, shuffle_ratio: float) -> np.ndarray:
    """base.pixel_shuffle over the token numbers 0 .. num_patches - 1 -> int32 [num_patches * r^2, 1 / r^2]: the source tokens whose
    channels, in this order, make output row j"""
    g = int(math.sqrt(num_patches))
    inv = round(1 / shuffle_ratio)
    if g * g != num_patches or abs(inv * shuffle_ratio - 1) > 1e-9 or g % inv:
        raise NotImplementedError(f"pixel_shuffle of {num_patches} patches at ratio {shuffle_ratio}")
    t = np.arange(num_patches, dtype=np.int32).reshape(1, g, g, 1)
    t = t.reshape(1, g, int(g * shuffle_ratio), int(1 / shuffle_ratio)).transpose(0, 2, 1, 3)
    t = t.reshape(1, int(g * shuffle_ratio), int(g * shuffle_ratio), int(1 / (shuffle_ratio ** 2))).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(t.reshape(-1, t.shape[-1]))


class Model:
    def __init__(self, config: ModelConfig, device="cuda", **engine_kwargs):
        if str(config.model_type).lower() != "internvl_chat":
            raise ValueError(f"Unsupported model type: {config.model_type}")
        self.config = config
        self.model_type = config.model_type
        self.device = device
        self.vision_model = VisionModel(config.vision_config, device=device)
        self.vision_tower = self.vision_model              # the name the loader and the vision cache look the tower up by
        self.language_model = LanguageModel(config.text_config, config, device=device, **engine_kwargs)
        self.downsample_ratio = config.downsample_ratio
        self.shuffle_index = pixel_shuffle_index(self.vision_model.num_patches, self.downsample_ratio)
        self.tokens_per_tile = self.shuffle_index.shape[0]
        self._mlp1: Dict[str, torch.Tensor] = {}
        self._gather_idx: Dict[int, torch.Tensor] = {}

    # ------------------------------------------------------------------ weights
    def load_weights(self, weights: Dict[str, torch.Tensor], strict: bool = True):
        from .. import quantized as Qz

        vt = {k[len(_V):]: v for k, v in weights.items() if k.startswith(_V)}
        lm = {k[len(_L):]: v for k, v in weights.items() if k.startswith(_L)}
        pj = {k[len(_M):]: v for k, v in weights.items() if k.startswith(_M)}
        if strict and len(vt) + len(lm) + len(pj) != len(weights):
            extra = [k for k in weights if not k.startswith((_V, _L, _M))]
            raise ValueError(f"unexpected weight names: {extra[:5]}")
        self.vision_model.load_weights(vt)
        self.language_model.load_weights(lm)
        dev, bf = self.device, torch.bfloat16

        def g(name):
            if name.endswith(".weight") and Qz.has_scales(pj, name[: -len(".weight")]):      # a 4-bit Linear: dequantised once
                return Qz.dequantize_bf16(Qz.take(pj, name[: -len(".weight")]), dev).contiguous()
            return pj[name].to(device=dev, dtype=bf).contiguous()

        self._mlp1 = {k: g(k) for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias")}
        return self

    def eval(self):
        return self

    @property
    def layers(self):
        return self.language_model.layers

    # ------------------------------------------------------------------ connector (reference internvl_chat.py:65-75)
    def _tile_gather_index(self, n_tiles: int) -> torch.Tensor:
        idx = self._gather_idx.get(n_tiles)
        if idx is None:
            T = self.vision_model.num_positions
            rows = (np.arange(n_tiles, dtype=np.int32)[:, None, None] * T + 1 + self.shuffle_index[None]).reshape(-1)
            idx = self._gather_idx[n_tiles] = _lib.h2d(rows.astype(np.int32), self.device)
        return idx

    def connector(self, hidden: torch.Tensor) -> torch.Tensor:
        """last tower state [tiles * (1 + P), E] -> image features bf16 [tiles * tokens_per_tile, llm hidden]"""
        E = hidden.shape[1]
        n_tiles = hidden.shape[0] // self.vision_model.num_positions
        k = self.shuffle_index.shape[1]
        x = ops.embed_gather(self._tile_gather_index(n_tiles), hidden).view(n_tiles * self.tokens_per_tile, k * E)
        p = self._mlp1
        x = ops.layernorm(x, p["0.weight"], p["0.bias"], eps=1e-5)                      # nn.LayerNorm's default eps
        h = ops.gemm(x, p["1.weight"], bias=p["1.bias"], epilogue=ops.EPI_BIAS | ops.EPI_GELU_ERF)
        return ops.gemm(h, p["3.weight"], bias=p["3.bias"], epilogue=ops.EPI_BIAS)

    def encode_image(self, pixel_values, **kwargs) -> torch.Tensor:
        pix = torch.as_tensor(pixel_values)
        if pix.ndim == 5:                  # (1, tiles, C, H, W), as the reference's processor hands them over
            pix = pix[0]
        return self.connector(self.vision_model(pix))

    # ------------------------------------------------------------------ reference internvl_chat.py:34-107
    def get_input_embeddings(self, input_ids=None, pixel_values=None, **kwargs):
        lm = self.language_model
        ids = _to_np(input_ids)
        if kwargs.get("video_grid_thw") is not None or kwargs.get("pixel_values_videos") is not None:
            raise NotImplementedError("video inputs are outside the built hot path")
        pos, deltas = lm.get_rope_index(ids)
        emb = lm.embed_tokens(ids)
        cached = kwargs.get("cached_image_features", None)
        if pixel_values is None and cached is None:
            return InputEmbeddingsFeatures(inputs_embeds=emb, position_ids=pos, rope_deltas=deltas)
        feats = cached if cached is not None else self.encode_image(pixel_values)
        image_token_index = kwargs.get("image_token_index", None)
        if image_token_index is None:
            image_token_index = self.config.image_token_index
        where = ids == int(image_token_index)
        if where.sum() == 0:
            where = ids == self.config.video_token_index
        rows = np.nonzero(where.reshape(-1))[0].astype(np.int32)
        feats = feats.reshape(-1, feats.shape[-1])
        if rows.size != feats.shape[0]:
            raise ValueError(f"{rows.size} image placeholder tokens for {feats.shape[0]} image feature rows")
        B, L = ids.shape
        flat = emb.reshape(B * L, -1)
        ops.scatter_rows_(feats, _lib.h2d(rows, self.device), flat)
        return InputEmbeddingsFeatures(inputs_embeds=flat.view(B, L, -1), position_ids=pos, rope_deltas=deltas)

    def __call__(self, input_ids, pixel_values=None, mask=None, cache=None, **kwargs):
        f = self.get_input_embeddings(input_ids, pixel_values, **kwargs)
        return self.language_model(input_ids, inputs_embeds=f.inputs_embeds, cache=cache, mask=None, position_ids=f.position_ids)

    # ------------------------------------------------------------------ checkpoint names
    def sanitize(self, weights):
        vt = self.vision_model.sanitize({k: v for k, v in weights.items() if k.startswith(_V)})
        rest = {k: v for k, v in weights.items() if not k.startswith(_V) and "rotary_emb.inv_freq" not in k}
        return {**rest, **vt}
