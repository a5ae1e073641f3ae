"""InternViT-300M vision tower of InternVL3 / InternVL3.5 on the C-ABI kernels - host mirror of the reference's
`mlx_vlm/models/internvl_chat/vision.py` (VisionEmbeddings 164-222, Attention 27-80, MLP 83-94, EncoderLayer 97-132 with its
layer scale, VisionModel 225-265), up to the last encoder state.

Per tile: patch GEMM (+bias, + the learned position rows as the residual operand) into rows 1.. of the tile's 1 + P rows, row 0
= T(class_embedding + position_embedding[0]) made once at load.  Then the native encoder loop (vlm_encoder_forward): LayerNorm ->
one fused qkv GEMM -> flash attention over the tile's 1 + P tokens (one segment per tile, 64-wide heads) -> proj GEMM whose
epilogue is bias, LAYER SCALE and residual (VLM_EPI_LAYERSCALE: x + ls1 * proj(..), each step rounded as the reference's typed
graph rounds it) -> LayerNorm -> fc1 GEMM + bias + GELU -> fc2 GEMM + bias + ls2 + residual.

The MLP's activation is `nn.GELU(approx="precise")` in the reference (vision.py:86), which in MLX is the TANH approximation
(mlx.nn.gelu_approx), not the erf form of the original InternViT: the engine follows the reference (VLM_EPI_GELU_TANH).

Outside the built path (NotImplementedError at construction): the InternViT-6B tower of the 38B / 78B models
(`qk_normalization` / `norm_type == "rms_norm"`), a head width the attention kernel does not have, a tile size other than
`image_size` (the reference interpolates the position table; at the native size that interpolation is the identity)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib, ops
from .config import VisionConfig

_KERNEL_HEAD_DIMS = (64, 80, 128)


class VisionModel:
    def __init__(self, config: VisionConfig, device="cuda"):
        if config.model_type not in ("siglip_vision_model", "intern_vit_6b"):
            raise ValueError(f"Unsupported model type: {config.model_type}")
        if config.qk_normalization or config.norm_type != "layer_norm":
            raise NotImplementedError("the InternViT-6B tower (qk_normalization / norm_type == 'rms_norm', the 38B / 78B models) is "
                                      "not built: the InternViT-300M form (LayerNorm, no QK-norm) is")
        if config.hidden_size % config.num_attention_heads:
            raise ValueError("hidden_size must be divisible by num_attention_heads")
        self.config = config
        self.model_type = config.model_type
        self.device = device
        c = config
        self.grid = c.image_size // c.patch_size
        self.num_patches = self.grid * self.grid
        self.num_positions = self.num_patches + 1
        self.head_dim = c.hidden_size // c.num_attention_heads
        if self.head_dim not in _KERNEL_HEAD_DIMS:
            raise NotImplementedError(f"vision head_dim {self.head_dim}: the attention kernel has {_KERNEL_HEAD_DIMS}")
        self.patch_dim = c.patch_size * c.patch_size * c.num_channels
        self.patch_k = (self.patch_dim + 63) // 64 * 64
        self._w: Dict[str, torch.Tensor] = {}
        self._enc = None

    # ------------------------------------------------------------------ weights
    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: names relative to `vision_model.` (patch weight (O, kH, kW, C), as sanitize leaves it).  A 4-bit Linear of a
        quantized checkpoint is dequantised once."""
        from .. import quantized as Qz

        self._enc = None
        c, dev, bf = self.config, self.device, torch.bfloat16
        E = c.hidden_size

        def g(name):
            if name.endswith(".weight") and Qz.has_scales(W, name[: -len(".weight")]):
                return Qz.dequantize_bf16(Qz.take(W, name[: -len(".weight")]), dev).contiguous()
            return W[name].to(device=dev, dtype=bf).contiguous()

        wp = torch.zeros(E, self.patch_k, dtype=bf, device=dev)
        wp[:, : self.patch_dim] = g("embeddings.patch_embedding.weight").reshape(E, -1)
        pos = g("embeddings.position_embedding").reshape(-1, E)
        if pos.shape[0] != self.num_positions:
            raise ValueError(f"position_embedding has {pos.shape[0]} rows for {self.num_positions} positions")
        cls = g("embeddings.class_embedding").reshape(1, E)
        # embeddings + position_embedding is ONE typed add (vision.py:220): the CLS row does not depend on the image
        cls_row = (cls.float() + pos[:1].float()).to(bf)
        self._w.update(wpatch=wp, bpatch=g("embeddings.patch_embedding.bias"), pos=pos[1:].contiguous(), cls_row=cls_row)
        for i in range(c.num_hidden_layers):
            p = f"encoder.layers.{i}."
            bqkv = g(p + "attn.qkv.bias") if c.qkv_bias else torch.zeros(3 * E, dtype=bf, device=dev)
            self._w.update({f"{i}.wqkv": g(p + "attn.qkv.weight"), f"{i}.bqkv": bqkv, f"{i}.wo": g(p + "attn.proj.weight"),
                            # [2, E]: the bias row, then the layer-scale row (VLM_EPI_LAYERSCALE, include/vlm_hip.h)
                            f"{i}.bo": ops.bias_scale(g(p + "attn.proj.bias"), g(p + "ls1")),
                            f"{i}.ln1w": g(p + "norm1.weight"), f"{i}.ln1b": g(p + "norm1.bias"),
                            f"{i}.ln2w": g(p + "norm2.weight"), f"{i}.ln2b": g(p + "norm2.bias"),
                            f"{i}.w1": g(p + "mlp.fc1.weight"), f"{i}.b1": g(p + "mlp.fc1.bias"),
                            f"{i}.w2": g(p + "mlp.fc2.weight"),
                            f"{i}.b2": ops.bias_scale(g(p + "mlp.fc2.bias"), g(p + "ls2"))})
        return self

    # ------------------------------------------------------------------ forward
    def patchify(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """[B, 3, S, S] float -> bf16 [B * P, patch_k]: each row one patch flattened (kH, kW, C)-major, which is what the NHWC
        Conv2d with kernel = stride = patch contracts"""
        c, G, P = self.config, self.grid, self.config.patch_size
        x = pixel_values
        if not x.is_cuda:
            x = _lib.h2d(x, self.device)
        B = x.shape[0]
        x = x.to(torch.float32).reshape(B, c.num_channels, G, P, G, P)
        x = x.permute(0, 2, 4, 3, 5, 1).reshape(B * G * G, self.patch_dim).contiguous()      # data movement only
        return ops.cast_pad(x, self.patch_k)

    def embeddings(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """VisionEmbeddings (vision.py:202-222) -> bf16 [B * (1 + P), E], tile b in rows b (1 + P) .."""
        c, w = self.config, self._w
        S = c.image_size
        if pixel_values.ndim != 4 or tuple(pixel_values.shape[1:]) != (c.num_channels, S, S):
            raise NotImplementedError(f"tiles of {tuple(pixel_values.shape[1:])}: only the native {S} x {S} tile is built (any other "
                                      "size interpolates the position table)")
        E, Np, T = c.hidden_size, self.num_patches, self.num_positions
        patches = self.patchify(pixel_values)
        B = patches.shape[0] // Np
        x = torch.empty(B * T, E, dtype=torch.bfloat16, device=self.device)
        for b in range(B):            # + bias, then + position rows: the table is the residual operand of each tile
            ops.gemm(patches[b * Np:(b + 1) * Np], w["wpatch"], bias=w["bpatch"], res=w["pos"], out=x[b * T + 1:(b + 1) * T],
                     epilogue=ops.EPI_BIAS | ops.EPI_RESIDUAL)
        x.view(B, T, E)[:, 0].copy_(w["cls_row"].expand(B, E))
        return x

    def __call__(self, pixel_values: torch.Tensor, output_hidden_states: Optional[bool] = None) -> torch.Tensor:
        """pixel_values [B, 3, S, S] (channels first, as the processor emits the tiles) -> the last encoder state as
        bf16 [B * (1 + P), E] (CLS row first in every tile)."""
        c = self.config
        x = self.embeddings(torch.as_tensor(pixel_values))
        T = self.num_positions
        B = x.shape[0] // T
        cu = _lib.h2d(np.arange(B + 1, dtype=np.int32) * T, self.device)
        nqb = B * ((T + 127) // 128)
        if self._enc is None:
            self._enc = ops.EncoderLayers(self._w, c.num_hidden_layers)
        return self._enc.forward_(x, c.num_attention_heads, self.head_dim, c.layer_norm_eps,
                                  ops.EPI_GELU_TANH | ops.EPI_LAYERSCALE, cu, nqb, float(self.head_dim) ** -0.5)

    # ------------------------------------------------------------------ checkpoint fix-ups (reference vision.py:247-265)
    def sanitize(self, weights):
        out = {}
        for k, v in weights.items():
            if "position_ids" in k:
                continue
            if "patch_embedding.weight" in k and v.ndim == 4:
                O, a, b_, c_ = v.shape
                if not (O >= a and O >= b_ and a == b_):       # torch layout (O, C, kH, kW) -> (O, kH, kW, C)
                    v = v.permute(0, 2, 3, 1)
            out[k] = v
        return out
