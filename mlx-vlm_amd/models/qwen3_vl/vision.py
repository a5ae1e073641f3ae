"""Qwen3-VL vision tower on MI355X - host mirror of the reference's mlx_vlm/models/qwen3_vl/vision.py (VisionModel, same
constructor / call / sanitize contract; the call returns (features, [DeepStack tap features])).

The host side the Qwen towers share (geometry, patch-weight fold, q / k interleave, rotary and per-frame tables, workspaces,
the engine call) is qwen2_vl.vision.VisionTower; this file adds the family's tensors, flag word and position-embedding tables.
The numerical work is one call into the native ViT engine, vlm_vit_forward with the Qwen3 facts (csrc/engine.hip: patch GEMM +
bias + position rows
-> depth x [LayerNorm, qkv GEMM + bias + 2-D rope, attention over cu_seqlens, proj GEMM + bias + residual, LayerNorm, fc1 GEMM +
bias + tanh-GELU, fc2 GEMM + bias + residual; behind a tap block the post-shuffle merger] -> PatchMerger).  The host prepares the
integer tables from `grid_thw`, which the reference also does on the host with .tolist() (vision.py:238-377): rotary rows,
cu_seqlens, and the four corner indices and weights of the bilinear interpolation of `pos_embed`.  The interpolation itself
(four row gathers, three typed multiplies-and-adds per element, once per call) stays torch on the device.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ..qwen2_vl.vision import VisionTower
from .config import VisionConfig

MLP_PAD = 64               # intermediate_size is zero-padded to a multiple of this (4304 -> 4352): gelu_tanh(0 + 0) = 0
SUPPORTED_HEAD_DIMS = (64, 80, 128)      # what the rope-in-epilogue GEMM (head_dim % 16 == 0) and the attention kernel take


def pos_embed_tables(grid_thw, num_grid_per_side: int, merge: int):
    """fast_pos_embed_interpolate's host half (reference vision.py:299-377), as numpy: for every patch ROW of the call (in the
    patch rows' merge-unit order, temporal copies included) the four corner indices into `pos_embed` and their bilinear weights.
    The reference computes both in float32 (mx.linspace, float products) and turns the weights into python floats before they
    become an array of the table's dtype; float32 numpy arithmetic here gives the same numbers.
    -> (idx int64 [4, N], weights float32 [4, N])"""
    S = int(num_grid_per_side)
    idx_all, w_all = [], []
    for t, h, w in np.asarray(grid_thw).tolist():
        t, h, w = int(t), int(h), int(w)
        hs = linspace_f32(0, S - 1, h)
        ws = linspace_f32(0, S - 1, w)
        hf, wf = hs.astype(np.int32), ws.astype(np.int32)
        hc, wc = np.minimum(hf + 1, S - 1), np.minimum(wf + 1, S - 1)
        dh, dw = hs - hf.astype(np.float32), ws - wf.astype(np.float32)
        bh, bhc = hf * S, hc * S
        one = np.float32(1)
        idx = np.stack([(bh[:, None] + wf[None, :]).reshape(-1), (bh[:, None] + wc[None, :]).reshape(-1),
                        (bhc[:, None] + wf[None, :]).reshape(-1), (bhc[:, None] + wc[None, :]).reshape(-1)]).astype(np.int64)
        wt = np.stack([((one - dh)[:, None] * (one - dw)[None, :]).reshape(-1), ((one - dh)[:, None] * dw[None, :]).reshape(-1),
                       (dh[:, None] * (one - dw)[None, :]).reshape(-1), (dh[:, None] * dw[None, :]).reshape(-1)]).astype(np.float32)

        def merge_order(a):          # [4, h * w] -> tile over t, then (t, h/m, m, w/m, m) -> (t, h/m, w/m, m, m)
            a = np.tile(a.reshape(4, 1, h, w), (1, t, 1, 1))
            a = a.reshape(4, t, h // merge, merge, w // merge, merge).transpose(0, 1, 2, 4, 3, 5)
            return a.reshape(4, -1)

        idx_all.append(merge_order(idx))
        w_all.append(merge_order(wt))
    return np.concatenate(idx_all, axis=1), np.concatenate(w_all, axis=1)


def linspace_f32(start, stop, num: int) -> np.ndarray:
    """the reference's mx.linspace(start, stop, num) in float32, taken as torch.linspace (what the goldens' MLX stand-in and
    transformers' own implementation of this function both call)"""
    return torch.linspace(float(start), float(stop), int(num), dtype=torch.float32).numpy()


class VisionModel(VisionTower):
    def __init__(self, config: VisionConfig, device="cuda"):
        if config.model_type != "qwen3_vl":
            raise ValueError(f"Unsupported model type: {config.model_type}")
        super().__init__(config, device, config.hidden_size, config.out_hidden_size,
                         (config.intermediate_size + MLP_PAD - 1) // MLP_PAD * MLP_PAD)
        self.num_grid_per_side = int(config.num_position_embeddings ** 0.5)
        self.deepstack_visual_indexes = list(config.deepstack_visual_indexes)

    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: sanitized names relative to the tower (`patch_embed.proj.{weight,bias}`, `pos_embed.weight`, `blocks.i....`,
        `merger....`, `deepstack_merger_list.j....`)."""
        c, keep = self.config, self._keep
        if self.head_dim not in SUPPORTED_HEAD_DIMS:
            raise NotImplementedError(f"vision head_dim = {self.head_dim}: the tower's rope-in-epilogue GEMM and attention kernel "
                                      f"are built for head_dim in {SUPPORTED_HEAD_DIMS} (Qwen3-VL 2B / 4B: 64; the 8B / 32B "
                                      "towers have 72)")
        taps = self.deepstack_visual_indexes
        if len(set(taps)) != len(taps) or any(i < 0 or i >= c.depth for i in taps):
            raise ValueError(f"deepstack_visual_indexes = {taps}: distinct block indices below depth = {c.depth}")
        if c.hidden_size * c.spatial_merge_size ** 2 > 8192:
            raise NotImplementedError("the post-shuffle LayerNorm is built for merge^2 * hidden_size <= 8192")
        wp = self._patch_weight(W)
        bp = keep("patch_embed.proj.bias", W["patch_embed.proj.bias"])
        keep("pos_embed.weight", W["pos_embed.weight"])
        E, I, Ip = c.hidden_size, c.intermediate_size, self.mlp_hidden
        self._create(_lib.VIT_QK_INTERLEAVED | _lib.VIT_FORM_QWEN3)
        perm = self.qk_perm()
        merger = ("norm.weight", "norm.bias", "linear_fc1.weight", "linear_fc1.bias", "linear_fc2.weight", "linear_fc2.bias")
        for i in range(c.depth):
            p = f"blocks.{i}."
            w1 = W[p + "mlp.linear_fc1.weight"].new_zeros(Ip, E)
            w1[:I] = W[p + "mlp.linear_fc1.weight"]
            b1 = W[p + "mlp.linear_fc1.bias"].new_zeros(Ip)
            b1[:I] = W[p + "mlp.linear_fc1.bias"]
            w2 = W[p + "mlp.linear_fc2.weight"].new_zeros(E, Ip)
            w2[:, :I] = W[p + "mlp.linear_fc2.weight"]
            wqkv, bqkv = W[p + "attn.qkv.weight"], W[p + "attn.qkv.bias"]
            tensors = [keep(p + "norm1.weight", W[p + "norm1.weight"]), keep(p + "norm1.bias", W[p + "norm1.bias"]),
                       keep(p + "attn.qkv.weight", wqkv[perm.to(wqkv.device)]), keep(p + "attn.qkv.bias", bqkv[perm.to(bqkv.device)]),
                       keep(p + "attn.proj.weight", W[p + "attn.proj.weight"]), keep(p + "attn.proj.bias", W[p + "attn.proj.bias"]),
                       keep(p + "norm2.weight", W[p + "norm2.weight"]), keep(p + "norm2.bias", W[p + "norm2.bias"]),
                       keep(p + "mlp.linear_fc1.weight", w1), keep(p + "mlp.linear_fc1.bias", b1),
                       keep(p + "mlp.linear_fc2.weight", w2), keep(p + "mlp.linear_fc2.bias", W[p + "mlp.linear_fc2.bias"])]
            if i in taps:
                q = f"deepstack_merger_list.{taps.index(i)}."
                tensors += [keep(q + n, W[q + n]) for n in merger]
            self._set_block(i, tensors)
        self._set_globals([wp] + [keep("merger." + n, W["merger." + n]) for n in merger] + [bp])

    # ------------------------------------------------------------------ host tables
    def _make_tables(self, grid_thw) -> dict:
        hit = super()._make_tables(grid_thw)
        idx, wt = pos_embed_tables(grid_thw, self.num_grid_per_side, self.spatial_merge_size)
        hit["pos_idx"] = _lib.h2d(idx, self.device)
        hit["pos_w"] = _lib.h2d(torch.from_numpy(wt).to(torch.bfloat16), self.device)          # weights in the table's dtype (342)
        return hit

    def fast_pos_embed_interpolate(self, grid_thw) -> torch.Tensor:
        """reference vision.py:299-377 -> bf16 [N, hidden_size], rows in the patch rows' merge-unit order.  The typed graph:
        four gathered rows times their weight (one rounding each), summed left to right (one rounding per add)."""
        t = self._tables(grid_thw)
        e = self._w["pos_embed.weight"][t["pos_idx"]] * t["pos_w"][:, :, None]
        return ((e[0] + e[1]) + e[2]) + e[3]

    # ------------------------------------------------------------------ forward
    def __call__(self, hidden_states: torch.Tensor, grid_thw, output_hidden_states: Optional[bool] = None, **kwargs):
        """hidden_states: pixel_values [N, C*T*ph*pw] (f32 or bf16, rows as the processor emits them).
        -> (features bf16 [N / merge^2, out_hidden_size], [tap features, same shape, one per deepstack_visual_indexes entry
        in BLOCK order - the order the reference appends them in])"""
        x = self._patch_rows(hidden_states)
        pos_rows = self.fast_pos_embed_interpolate(grid_thw).contiguous()
        n_taps = len(self.deepstack_visual_indexes)
        tap_out = torch.empty(n_taps, x.shape[0] // self.spatial_merge_size ** 2, self.out_dim, dtype=torch.bfloat16,
                              device=self.device)
        out = self._forward(x, self._tables(grid_thw), pos_rows=pos_rows.data_ptr(),
                            tap_out=tap_out.data_ptr() if n_taps else None, n_taps=n_taps)
        return out, [tap_out[j] for j in range(n_taps)]
