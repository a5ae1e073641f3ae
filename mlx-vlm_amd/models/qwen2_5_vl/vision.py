"""Qwen2.5-VL vision tower on MI355X - host mirror of the reference's
mlx_vlm/models/qwen2_5_vl/vision.py (VisionModel, same constructor / call / sanitize contract).

The numerical work is one call into the native ViT engine in its Qwen2.5 form (csrc/engine.hip: patch GEMM -> gather into
window order -> depth x [RMSNorm, qkv GEMM + bias + 2-D rope, window or full attention, proj GEMM + bias + residual, RMSNorm,
gate/up GEMM + bias + SwiGLU, down GEMM + bias + residual] -> PatchMerger -> gather back).  The host prepares integer tables
from `grid_thw`, which the reference also does on the host with .tolist() (vision.py:228,269,340-346): the window index, the
window table, the rotary rows in window order, the full-image cu_seqlens and the reverse index.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ..._lib import check
from ..qwen2_vl.vision import check_array_shape, rot_pos_ids
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


def full_cu_seqlens(grid_thw) -> np.ndarray:
    """reference vision.py:360-373: one segment per frame"""
    lens = []
    for t, h, w in np.asarray(grid_thw).tolist():
        lens += [h * w] * t
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


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


class VisionModel:
    def __init__(self, config: VisionConfig, device="cuda"):
        self.config = config
        self.model_type = config.model_type
        if self.model_type != "qwen2_5_vl":
            raise ValueError(f"Unsupported model type: {self.model_type}")
        self.spatial_merge_size = config.spatial_merge_size
        self.spatial_merge_unit = config.spatial_merge_size ** 2
        self.window_size = config.window_size
        self.patch_size = config.patch_size
        self.fullatt_block_indexes = list(config.fullatt_block_indexes)
        self.device = device
        self.embed_dim = config.hidden_size
        self.num_heads = config.num_heads
        self.head_dim = config.hidden_size // config.num_heads
        self.patch_dim = config.in_channels * config.temporal_patch_size * config.patch_size * config.patch_size
        self.patch_k = (self.patch_dim + 63) // 64 * 64          # K of the patch GEMM, zero padded
        self.mlp_hidden = (config.intermediate_size + MLP_PAD - 1) // MLP_PAD * MLP_PAD
        self._handle = None
        self._w: Dict[str, torch.Tensor] = {}
        self._tab_cache: Dict[tuple, tuple] = {}

    # ------------------------------------------------------------------ weights
    @property
    def dtype(self):
        return torch.bfloat16

    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: sanitized names relative to the tower (`patch_embed.proj.weight`, `blocks.i....`, `merger....`)."""
        c, dev = self.config, self.device
        if self.head_dim != 80:
            raise NotImplementedError(f"vision head_dim = {self.head_dim}: the Qwen2.5-VL tower is built for head_dim 80 "
                                      "(hidden_size 1280 / 16 heads)")
        if c.depth > 64 or any(i < 0 or i >= c.depth for i in self.fullatt_block_indexes):
            raise NotImplementedError(f"depth = {c.depth}, fullatt_block_indexes = {self.fullatt_block_indexes}: up to 64 blocks")
        L = _lib.lib()
        bf = torch.bfloat16

        def keep(name, t):
            t = t.to(device=dev, dtype=bf).contiguous()
            self._w[name] = t
            return t

        pw = W["patch_embed.proj.weight"]
        if pw.dim() == 5:
            # (O, T, H, W, C) channels-last after sanitize -> columns in the processor's (C, T, ph, pw) order (as Qwen2-VL)
            pw = pw.permute(0, 4, 1, 2, 3).reshape(pw.shape[0], -1)
        wp = torch.zeros(c.hidden_size, self.patch_k, dtype=bf, device=dev)
        wp[:, : self.patch_dim] = pw.to(device=dev, dtype=bf)
        self._w["patch"] = wp

        E, hd, half = c.hidden_size, self.head_dim, self.head_dim // 2
        cfg = _lib.VitConfig(c.depth, E, c.num_heads, self.mlp_hidden, self.patch_k, c.spatial_merge_size, c.out_hidden_size,
                             1e-6, _lib.VIT_QK_INTERLEAVED | _lib.VIT_FORM_QWEN2_5)   # nn.RMSNorm(eps=1e-6): vision.py:110,180-181
        # q / k rows interleaved per head for the rope-in-epilogue GEMM: (d, d + hd/2) -> (2d, 2d + 1), as Qwen2-VL does
        inter = torch.stack([torch.arange(half), torch.arange(half) + half], dim=1).reshape(-1)
        perm = (torch.arange(2 * c.num_heads)[:, None] * hd + inter[None, :]).reshape(-1)
        qk_perm = torch.cat([perm, torch.arange(2 * E, 3 * E)])
        h = C.c_void_p()
        check(L.vlm_vit_create(C.byref(cfg), C.byref(h)), "vit_create")
        self._handle = h
        for i in range(c.depth):
            p = f"blocks.{i}."
            wgu, bgu, wd, ip = pad_mlp(W[p + "mlp.gate_proj.weight"], W[p + "mlp.gate_proj.bias"], W[p + "mlp.up_proj.weight"],
                                       W[p + "mlp.up_proj.bias"], W[p + "mlp.down_proj.weight"])
            assert ip == self.mlp_hidden
            ptr = {
                "ln1_w": keep(p + "norm1.weight", W[p + "norm1.weight"]),
                "wqkv": keep(p + "attn.qkv.weight", W[p + "attn.qkv.weight"][qk_perm.to(W[p + "attn.qkv.weight"].device)]),
                "bqkv": keep(p + "attn.qkv.bias", W[p + "attn.qkv.bias"][qk_perm.to(W[p + "attn.qkv.bias"].device)]),
                "wproj": keep(p + "attn.proj.weight", W[p + "attn.proj.weight"]),
                "bproj": keep(p + "attn.proj.bias", W[p + "attn.proj.bias"]),
                "ln2_w": keep(p + "norm2.weight", W[p + "norm2.weight"]),
                "wfc1": keep(p + "mlp.gate_up.weight", wgu), "bfc1": keep(p + "mlp.gate_up.bias", bgu),
                "wfc2": keep(p + "mlp.down_proj.weight", wd), "bfc2": keep(p + "mlp.down_proj.bias", W[p + "mlp.down_proj.bias"]),
            }
            blk = _lib.VitBlock(ptr["ln1_w"].data_ptr(), None, ptr["wqkv"].data_ptr(), ptr["bqkv"].data_ptr(),
                                ptr["wproj"].data_ptr(), ptr["bproj"].data_ptr(), ptr["ln2_w"].data_ptr(), None,
                                ptr["wfc1"].data_ptr(), ptr["bfc1"].data_ptr(), ptr["wfc2"].data_ptr(), ptr["bfc2"].data_ptr())
            check(L.vlm_vit_set_block(h, i, C.byref(blk)), "vit_set_block")
        m = {n: keep("merger." + n, W["merger." + n]) for n in ("ln_q.weight", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
                                                                 "mlp.2.bias")}
        gl = _lib.VitGlobals(wp.data_ptr(), m["ln_q.weight"].data_ptr(), None, m["mlp.0.weight"].data_ptr(),
                             m["mlp.0.bias"].data_ptr(), m["mlp.2.weight"].data_ptr(), m["mlp.2.bias"].data_ptr())
        check(L.vlm_vit_set_globals(h, C.byref(gl)), "vit_set_globals")
        self._fullatt_mask = sum(1 << i for i in set(self.fullatt_block_indexes))

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().vlm_vit_destroy(self._handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ host tables
    def get_window_index(self, grid_thw):
        """reference vision.py:261-324 -> (window_index, cu_window_seqlens) as numpy arrays"""
        wi, cu = get_window_index(grid_thw, self.window_size, self.spatial_merge_size, self.patch_size)
        return wi, np.asarray(cu, dtype=np.int64)

    def rot_pos_emb(self, grid_thw, pos=None) -> torch.Tensor:
        """freqs [N, head_dim/2] fp32 (reference vision.py:225-259); pos: position ids in another row order"""
        g = np.asarray(grid_thw)
        if pos is None:
            pos = rot_pos_ids(g, self.spatial_merge_size)
        dim = self.head_dim // 2
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
        seq = torch.arange(int(g[:, 1:].max()), dtype=torch.float32)
        full = torch.outer(seq, inv_freq)
        return full[torch.from_numpy(pos)].reshape(pos.shape[0], -1)

    def _tables(self, grid_thw):
        key = tuple(map(tuple, np.asarray(grid_thw).tolist()))
        hit = self._tab_cache.get(key)
        if hit is None:
            t = host_tables(grid_thw, self.window_size, self.spatial_merge_size, self.patch_size)
            freqs = self.rot_pos_emb(grid_thw, t["pos"])                                        # rows in window order
            cs = _lib.h2d(torch.stack([torch.cos(freqs), torch.sin(freqs)]).contiguous(), self.device)   # ONE table
            full_lens, win_lens = np.diff(t["cu_full"]), np.diff(t["cu_window"])
            hit = {
                "cos": cs[0], "sin": cs[1], "cs": cs,
                "cu_full": _lib.h2d(t["cu_full"], self.device), "nseg": len(full_lens),
                "nqb": int(sum((int(l) + 127) // 128 for l in full_lens)), "uniform": int(len(set(full_lens.tolist())) == 1),
                "cu_win": _lib.h2d(t["cu_window"], self.device), "win_nseg": len(win_lens),
                "win_nqb": int(sum((int(l) + 127) // 128 for l in win_lens)), "win_max": int(win_lens.max()),
                "window_index": _lib.h2d(t["window_index"].astype(np.int32), self.device),
                "reverse_index": _lib.h2d(t["reverse_index"].astype(np.int32), self.device),
            }
            if len(self._tab_cache) > 64:
                self._tab_cache.clear()
            self._tab_cache[key] = hit
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
        from ... import ops

        c = self.config
        if not hidden_states.is_cuda:
            hidden_states = _lib.h2d(hidden_states, self.device)
        N = hidden_states.shape[0]
        if hidden_states.dtype != torch.float32:
            hidden_states = hidden_states.to(torch.float32)          # bf16 -> fp32 -> bf16 is lossless
        x = ops.cast_pad(hidden_states.contiguous(), self.patch_k)
        t = self._tables(grid_thw)
        E, dev = c.hidden_size, self.device
        mm = self.spatial_merge_unit
        bf = torch.bfloat16
        ws = {n: torch.empty(N, d, dtype=bf, device=dev) for n, d in
              (("x", E), ("xn", E), ("qkv", 3 * E), ("attn", E), ("mlp", self.mlp_hidden))}
        mrg = torch.empty(N // mm, E * mm, dtype=bf, device=dev)
        out = torch.empty(N // mm, c.out_hidden_size, dtype=bf, device=dev)
        a = _lib.VitArgs(x.data_ptr(), N, t["cos"].data_ptr(), t["sin"].data_ptr(), t["cu_full"].data_ptr(), t["nseg"], t["nqb"],
                         ws["x"].data_ptr(), ws["xn"].data_ptr(), ws["qkv"].data_ptr(), ws["attn"].data_ptr(),
                         ws["mlp"].data_ptr(), mrg.data_ptr(), out.data_ptr(), t["uniform"],
                         t["cu_win"].data_ptr(), t["win_nseg"], t["win_nqb"], t["win_max"], int(self.one_tile(t["win_max"])),
                         t["window_index"].data_ptr(), t["reverse_index"].data_ptr(), self._fullatt_mask)
        check(_lib.lib().vlm_vit_forward(self._handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "vit_forward")
        return out

    # ------------------------------------------------------------------ checkpoint key/layout fixups
    def sanitize(self, weights):
        """reference vision.py:395-413."""
        out = {}
        for k, v in weights.items():
            if "position_ids" in k:
                continue
            if "patch_embed.proj.weight" in k:
                out[k] = v if check_array_shape(v) else v.permute(0, 2, 3, 4, 1)
            else:
                out[k] = v
        return out

