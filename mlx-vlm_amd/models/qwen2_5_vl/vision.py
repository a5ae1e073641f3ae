"""Qwen2.5-VL vision tower on MI355X - host mirror of the reference's
mlx_vlm/models/qwen2_5_vl/vision.py (VisionModel, same constructor / call / sanitize contract).

The host side the Qwen towers share (geometry, patch-weight fold, q / k interleave, rotary and per-frame tables, workspaces,
the engine call) is qwen2_vl.vision.VisionTower; this file adds the family's tensors, flag word and window tables.  The numerical
work is one call into the native ViT engine, vlm_vit_forward with the Qwen2.5 facts (csrc/engine.hip: patch GEMM -> gather into
window order -> depth x [RMSNorm, qkv GEMM + bias + 2-D rope, window or full attention, proj GEMM + bias + residual, RMSNorm,
gate/up GEMM + bias + SwiGLU, down GEMM + bias + residual] -> PatchMerger -> gather back).  The host prepares integer tables
from `grid_thw`, which the reference also does on the host with .tolist() (vision.py:228,269,340-346): the window index, the
window table, the rotary rows in window order, the full-image cu_seqlens and the reverse index.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ..qwen2_vl.vision import VisionTower, full_cu_seqlens, rot_pos_ids
from .config import VisionConfig

ONE_TILE_MAX = 64          # tokens of the one-tile attention kernel (csrc/attn_window.hip)
# The tower's default for its window blocks.  The one-tile kernel is the default while its launch beats the general kernel's at
# both measured shapes by more than the run-to-run spread and the whole tower is nowhere slower (profiles/qwen2_5_vl_window_attn.txt,
# MI355X, real tower widths): launch 5.05 against 5.79 us at one 448 x 448 image and 34.6 against 141.2 at 16 (spread 0.3 %); whole
# 32-block tower 23.3 against 25.3 ms at 16 images, 0.2 - 0.3 % less at one image (the edge of the spread: nothing a user sees).
ONE_TILE_DEFAULT = True
MLP_PAD = 64               # intermediate_size is zero-padded to a multiple of this (3420 -> 3456)


def get_window_index(grid_thw, window_size: int, spatial_merge_size: int, patch_size: int):
    """VisionModel.get_window_index (reference vision.py:261-324), integer-exact.
    -> (window_index int64 [N / merge^2], cu_window_seqlens int64 list as the reference returns it: with the repeated entries of
    the padding windows it adds when a grid side is a multiple of the window)."""
    window_index, cu = [], [0]
    window_index_id = 0
    unit = spatial_merge_size * spatial_merge_size
    vw = window_size // spatial_merge_size // patch_size
    for grid_t, grid_h, grid_w in np.asarray(grid_thw).tolist():
        lh, lw = grid_h // spatial_merge_size, grid_w // spatial_merge_size
        index = np.arange(grid_t * lh * lw).reshape(grid_t, lh, lw)
        pad_h, pad_w = vw - lh % vw, vw - lw % vw                     # a full extra window when the side is a multiple
        nh, nw = (lh + pad_h) // vw, (lw + pad_w) // vw
        padded = np.pad(index, ((0, 0), (0, pad_h), (0, pad_w)), mode="constant", constant_values=-100)
        padded = padded.reshape(grid_t, nh, vw, nw, vw).transpose(0, 1, 3, 2, 4).reshape(grid_t, nh * nw, vw, vw)
        seqlens = (padded != -100).sum(axis=(2, 3)).reshape(-1)
        flat = padded.reshape(-1)
        window_index.append(flat[flat != -100] + window_index_id)
        cu.extend((np.cumsum(seqlens) * unit + cu[-1]).tolist())
        window_index_id += int(grid_t * lh * lw)
    return np.concatenate(window_index, axis=0).astype(np.int64), [int(x) for x in cu]


def dedup_cu(cu) -> np.ndarray:
    """first occurrence of each value (reference vision.py:337-346): the zero-length windows leave the table"""
    seen, out = set(), []
    for x in cu:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return np.asarray(out, dtype=np.int32)


def host_tables(grid_thw, window_size: int, spatial_merge_size: int, patch_size: int):
    """-> dict of numpy tables: window_index, cu_window (zero-length windows dropped), reverse_index, cu_full, pos (the
    (h, w) rotary position ids [N, 2] in WINDOW order)."""
    unit = spatial_merge_size ** 2
    wi, cu = get_window_index(grid_thw, window_size, spatial_merge_size, patch_size)
    pos = rot_pos_ids(np.asarray(grid_thw), spatial_merge_size)
    pos = pos.reshape(-1, unit, 2)[wi].reshape(-1, 2)                 # rotary_pos_emb[window_index] (354-358)
    return {"window_index": wi, "cu_window": dedup_cu(cu), "reverse_index": np.argsort(wi, kind="stable").astype(np.int64),
            "cu_full": full_cu_seqlens(grid_thw), "pos": pos}


def pad_mlp(wg, bg, wu, bu, wd, pad_to: int = MLP_PAD):
    """gate / up rows and biases and down's columns zero-padded to a multiple of `pad_to`, gate / up interleaved
    (g0, u0, g1, u1, ...) for the SwiGLU epilogue.  A padded unit is silu(0 + 0) * (0 + 0) = 0 times a zero column of down.
    -> (wgu [2 Ip, E], bgu [2 Ip], wd [E, Ip], Ip)"""
    inter, E = wg.shape
    ip = (inter + pad_to - 1) // pad_to * pad_to
    wgu = wg.new_zeros(2 * ip, E)
    bgu = bg.new_zeros(2 * ip)
    wgu[0:2 * inter:2], wgu[1:2 * inter:2] = wg, wu
    bgu[0:2 * inter:2], bgu[1:2 * inter:2] = bg, bu
    wdp = wd.new_zeros(wd.shape[0], ip)
    wdp[:, :inter] = wd
    return wgu, bgu, wdp, ip


class VisionModel(VisionTower):
    def __init__(self, config: VisionConfig, device="cuda"):
        if config.model_type != "qwen2_5_vl":
            raise ValueError(f"Unsupported model type: {config.model_type}")
        super().__init__(config, device, config.hidden_size, config.out_hidden_size,
                         (config.intermediate_size + MLP_PAD - 1) // MLP_PAD * MLP_PAD)
        self.spatial_merge_unit = config.spatial_merge_size ** 2
        self.window_size = config.window_size
        self.patch_size = config.patch_size
        self.fullatt_block_indexes = list(config.fullatt_block_indexes)

    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: sanitized names relative to the tower (`patch_embed.proj.weight`, `blocks.i....`, `merger....`)."""
        c, keep = self.config, self._keep
        if self.head_dim != 80:
            raise NotImplementedError(f"vision head_dim = {self.head_dim}: the Qwen2.5-VL tower is built for head_dim 80 "
                                      "(hidden_size 1280 / 16 heads)")
        if c.depth > 64 or any(i < 0 or i >= c.depth for i in self.fullatt_block_indexes):
            raise NotImplementedError(f"depth = {c.depth}, fullatt_block_indexes = {self.fullatt_block_indexes}: up to 64 blocks")
        wp = self._patch_weight(W)
        self._create(_lib.VIT_QK_INTERLEAVED | _lib.VIT_FORM_QWEN2_5)
        perm = self.qk_perm()
        for i in range(c.depth):
            p = f"blocks.{i}."
            wgu, bgu, wd, ip = pad_mlp(W[p + "mlp.gate_proj.weight"], W[p + "mlp.gate_proj.bias"], W[p + "mlp.up_proj.weight"],
                                       W[p + "mlp.up_proj.bias"], W[p + "mlp.down_proj.weight"])
            assert ip == self.mlp_hidden
            wqkv, bqkv = W[p + "attn.qkv.weight"], W[p + "attn.qkv.bias"]
            self._set_block(i, [
                keep(p + "norm1.weight", W[p + "norm1.weight"]), None,
                keep(p + "attn.qkv.weight", wqkv[perm.to(wqkv.device)]), keep(p + "attn.qkv.bias", bqkv[perm.to(bqkv.device)]),
                keep(p + "attn.proj.weight", W[p + "attn.proj.weight"]), keep(p + "attn.proj.bias", W[p + "attn.proj.bias"]),
                keep(p + "norm2.weight", W[p + "norm2.weight"]), None,
                keep(p + "mlp.gate_up.weight", wgu), keep(p + "mlp.gate_up.bias", bgu),
                keep(p + "mlp.down_proj.weight", wd), keep(p + "mlp.down_proj.bias", W[p + "mlp.down_proj.bias"])])
        m = {n: keep("merger." + n, W["merger." + n]) for n in ("ln_q.weight", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
                                                                 "mlp.2.bias")}
        self._set_globals([wp, m["ln_q.weight"], None, m["mlp.0.weight"], m["mlp.0.bias"], m["mlp.2.weight"], m["mlp.2.bias"]])
        self._fullatt_mask = sum(1 << i for i in set(self.fullatt_block_indexes))

    # ------------------------------------------------------------------ host tables
    def get_window_index(self, grid_thw):
        """reference vision.py:261-324 -> (window_index, cu_window_seqlens) as numpy arrays"""
        wi, cu = get_window_index(grid_thw, self.window_size, self.spatial_merge_size, self.patch_size)
        return wi, np.asarray(cu, dtype=np.int64)

    def _make_tables(self, grid_thw) -> dict:
        t = host_tables(grid_thw, self.window_size, self.spatial_merge_size, self.patch_size)
        hit = super()._make_tables(grid_thw, t["pos"])                                          # rotary rows in window order
        win_lens = np.diff(t["cu_window"])
        hit.update({
            "cu_win": _lib.h2d(t["cu_window"], self.device), "win_nseg": len(win_lens),
            "win_nqb": int(sum((int(n) + 127) // 128 for n in win_lens)), "win_max": int(win_lens.max()),
            "window_index": _lib.h2d(t["window_index"].astype(np.int32), self.device),
            "reverse_index": _lib.h2d(t["reverse_index"].astype(np.int32), self.device),
        })
        return hit

    def one_tile(self, win_max: int) -> bool:
        """window blocks on the one-tile kernel?  Every window must fit its tile; VLM_VIT_WINDOW_ATTN=0 forces the general
        kernel over the same window table, =1 the one-tile kernel (A/B knob)."""
        env = os.environ.get("VLM_VIT_WINDOW_ATTN", "")
        want = ONE_TILE_DEFAULT if env == "" else env != "0"
        return bool(want and win_max <= ONE_TILE_MAX and self.head_dim == 80)

    # ------------------------------------------------------------------ forward
    def __call__(self, hidden_states: torch.Tensor, grid_thw, output_hidden_states: Optional[bool] = None):
        """hidden_states: pixel_values [N, C*T*ph*pw] (f32 or bf16, rows as the processor emits them).
        -> [N / merge^2, out_hidden_size] bf16, rows in the processor's order."""
        x = self._patch_rows(hidden_states)
        t = self._tables(grid_thw)
        return self._forward(x, t, win_cu_seqlens=t["cu_win"].data_ptr(), win_nseg=t["win_nseg"], win_total_qblocks=t["win_nqb"],
                             win_max_seg=t["win_max"], win_one_tile=int(self.one_tile(t["win_max"])),
                             window_index=t["window_index"].data_ptr(), reverse_index=t["reverse_index"].data_ptr(),
                             fullatt_mask=self._fullatt_mask)
