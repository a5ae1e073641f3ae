"""Qwen2-VL vision tower on MI355X - host mirror of the reference's
mlx_vlm/models/qwen2_vl/vision.py (VisionModel, same constructor / call /
sanitize contract).  The numerical work is one call into the native ViT engine
(csrc/engine.hip, vlm_vit_forward: patch GEMM -> 32 x [LN, qkv GEMM+bias, 2-D rope,
varlen flash attention, proj GEMM+bias+residual, LN, fc1 GEMM+bias+GELU, fc2
GEMM+bias+residual] -> PatchMerger); the host only prepares integer position tables
(rot_pos_emb, cu_seqlens) from `grid_thw`, which the reference also does on the
host with .tolist() (vision.py:63,219-279).

VisionTower is the host side every Qwen tower shares (this one, qwen2_5_vl and
qwen3_vl): geometry, the patch-weight fold, the q / k interleave, the rotary and
per-frame segment tables with their cache, the workspaces and the engine call.
A family's VisionModel adds its tensors, its flag word and its own tables.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ..._lib import check
from .config import VisionConfig


def check_array_shape(arr) -> bool:
    """reference vision.py:9-26 (is the conv weight already channels-last?)."""
    shape = arr.shape
    if len(shape) not in [4, 5]:
        return False
    B, out_channels, kH, KW, t = shape
    if t == 3:
        return True
    return bool((out_channels >= kH) and (out_channels >= KW) and (kH == KW))


def rot_pos_ids(grid_thw: np.ndarray, merge: int) -> np.ndarray:
    """Integer part of VisionModel.rot_pos_emb (reference vision.py:219-247)."""
    out = []
    for t, h, w in np.asarray(grid_thw).tolist():
        hpos = np.repeat(np.arange(h)[:, None], w, axis=1)
        wpos = np.repeat(np.arange(w)[None, :], h, axis=0)

        def window(a):
            return a.reshape(h // merge, merge, w // merge, merge).transpose(0, 2, 1, 3).reshape(-1)

        out.append(np.tile(np.stack([window(hpos), window(wpos)], axis=-1), (t, 1)))
    return np.concatenate(out, axis=0).astype(np.int64)


def full_cu_seqlens(grid_thw) -> np.ndarray:
    """one attention segment per frame (reference vision.py:257-279)"""
    lens = []
    for t, h, w in np.asarray(grid_thw).tolist():
        lens += [h * w] * t
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


class VisionTower:
    def __init__(self, config, device, embed_dim: int, out_dim: int, mlp_hidden: int):
        self.config = config
        self.model_type = config.model_type
        self.spatial_merge_size = config.spatial_merge_size
        self.device = device
        self.embed_dim = embed_dim
        self.out_dim = out_dim
        self.num_heads = config.num_heads
        self.head_dim = embed_dim // config.num_heads
        self.patch_dim = config.in_channels * config.temporal_patch_size * config.patch_size * config.patch_size
        self.patch_k = (self.patch_dim + 63) // 64 * 64          # K of the patch GEMM, zero padded
        self.mlp_hidden = mlp_hidden
        self._handle = None
        self._w: Dict[str, torch.Tensor] = {}
        self._tab_cache: Dict[tuple, dict] = {}

    @property
    def dtype(self):
        return torch.bfloat16

    # ------------------------------------------------------------------ weights
    def _keep(self, name: str, t: torch.Tensor) -> torch.Tensor:
        t = t.to(device=self.device, dtype=torch.bfloat16).contiguous()
        self._w[name] = t
        return t

    def _patch_weight(self, W) -> torch.Tensor:
        pw = W["patch_embed.proj.weight"]
        if pw.dim() == 5:
            # (O, T, H, W, C) channels-last as the reference holds it after sanitize.  The reference moves the
            # PIXELS to channels-last on every call (vision.py:93-101); we fold that permutation into the weight
            # once: columns back to the processor's (C, T, ph, pw) order, so pixel rows feed the GEMM as they are.
            pw = pw.permute(0, 4, 1, 2, 3).reshape(pw.shape[0], -1)
        wp = torch.zeros(self.embed_dim, self.patch_k, dtype=torch.bfloat16, device=self.device)
        wp[:, : self.patch_dim] = pw.to(device=self.device, dtype=torch.bfloat16)
        self._w["patch"] = wp
        return wp

    def qk_perm(self) -> torch.Tensor:
        """row order of wqkv / bqkv for the 2-D rope in the qkv GEMM epilogue (vlm_gemm_bf16_rope2d): the q / k rows of every
        head interleaved, (d, d + hd/2) -> (2d, 2d + 1).  q.k does not change under a common permutation of the head dimension,
        v and everything downstream are untouched."""
        E, hd, half = self.embed_dim, self.head_dim, self.head_dim // 2
        inter = torch.stack([torch.arange(half), torch.arange(half) + half], dim=1).reshape(-1)          # 0, hd/2, 1, hd/2+1, ...
        perm = (torch.arange(2 * self.num_heads)[:, None] * hd + inter[None, :]).reshape(-1)                # q and k heads
        return torch.cat([perm, torch.arange(2 * E, 3 * E)])

    def _create(self, flags: int):
        """the engine handle; eps: nn.LayerNorm / nn.RMSNorm(eps=1e-6) is hard-coded in all three references"""
        c = self.config
        cfg = _lib.VitConfig(c.depth, self.embed_dim, c.num_heads, self.mlp_hidden, self.patch_k, c.spatial_merge_size, self.out_dim,
                             1e-6, flags)
        h = C.c_void_p()
        check(_lib.lib().vlm_vit_create(C.byref(cfg), C.byref(h)), "vit_create")
        self._handle = h

    def _set_block(self, i: int, tensors):
        """tensors: the block's vlm_vit_block fields in order, None where the form has none"""
        blk = _lib.VitBlock(*[None if t is None else t.data_ptr() for t in tensors])
        check(_lib.lib().vlm_vit_set_block(self._handle, i, C.byref(blk)), "vit_set_block")

    def _set_globals(self, tensors):
        gl = _lib.VitGlobals(*[None if t is None else t.data_ptr() for t in tensors])
        check(_lib.lib().vlm_vit_set_globals(self._handle, C.byref(gl)), "vit_set_globals")

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().vlm_vit_destroy(self._handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ host tables
    def rot_pos_emb(self, grid_thw, pos=None) -> torch.Tensor:
        """freqs [N, head_dim/2] fp32 (reference vision.py:219-255); pos: position ids in another row order"""
        g = np.asarray(grid_thw)
        if pos is None:
            pos = rot_pos_ids(g, self.spatial_merge_size)
        dim = self.head_dim // 2
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
        seq = torch.arange(int(g[:, 1:].max()), dtype=torch.float32)
        full = torch.outer(seq, inv_freq)
        return full[torch.from_numpy(pos)].reshape(pos.shape[0], -1)

    def _make_tables(self, grid_thw, pos=None) -> dict:
        """device tables of one grid_thw: the rotary rows as ONE cos | sin table and one attention segment per frame"""
        freqs = self.rot_pos_emb(grid_thw, pos)
        cu = full_cu_seqlens(grid_thw)
        lens = np.diff(cu).tolist()
        cs = _lib.h2d(torch.stack([torch.cos(freqs), torch.sin(freqs)]).contiguous(), self.device)
        return {"cos": cs[0], "sin": cs[1], "cs": cs, "cu": _lib.h2d(cu, self.device), "nseg": len(lens),
                "nqb": int(sum((n + 127) // 128 for n in lens)), "uniform": int(len(set(lens)) == 1)}

    def _tables(self, grid_thw) -> dict:
        key = tuple(map(tuple, np.asarray(grid_thw).tolist()))
        hit = self._tab_cache.get(key)
        if hit is None:
            hit = self._make_tables(grid_thw)
            if len(self._tab_cache) > 64:
                self._tab_cache.clear()
            self._tab_cache[key] = hit
        return hit

    # ------------------------------------------------------------------ forward
    def _patch_rows(self, hidden_states: torch.Tensor) -> torch.Tensor:
        """PatchEmbed (vision.py:93-101): astype(weight dtype) + zero pad of K (the channels-last move is folded into the
        weight, see _patch_weight)"""
        from ... import ops

        if not hidden_states.is_cuda:
            hidden_states = _lib.h2d(hidden_states, self.device)
        if hidden_states.dtype != torch.float32:
            hidden_states = hidden_states.to(torch.float32)          # bf16 -> fp32 -> bf16 is lossless
        return ops.cast_pad(hidden_states.contiguous(), self.patch_k)

    def _forward(self, x: torch.Tensor, t: dict, **form_args) -> torch.Tensor:
        """x: patch rows bf16 [N, patch_k]; t: _tables' entry; form_args: the vlm_vit_args fields of the tower's form"""
        N, E, dev, bf = x.shape[0], self.embed_dim, self.device, torch.bfloat16
        mm = self.spatial_merge_size ** 2
        ws = {n: torch.empty(N, d, dtype=bf, device=dev) for n, d in
              (("x", E), ("xn", E), ("qkv", 3 * E), ("attn", E), ("mlp", self.mlp_hidden))}
        mrg = torch.empty(N // mm, E * mm, dtype=bf, device=dev)
        out = torch.empty(N // mm, self.out_dim, dtype=bf, device=dev)
        a = _lib.VitArgs(x.data_ptr(), N, t["cos"].data_ptr(), t["sin"].data_ptr(), t["cu"].data_ptr(), t["nseg"], t["nqb"],
                         ws["x"].data_ptr(), ws["xn"].data_ptr(), ws["qkv"].data_ptr(), ws["attn"].data_ptr(),
                         ws["mlp"].data_ptr(), mrg.data_ptr(), out.data_ptr(), t["uniform"], **form_args)
        check(_lib.lib().vlm_vit_forward(self._handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "vit_forward")
        return out

    # ------------------------------------------------------------------ checkpoint key/layout fixups
    def sanitize(self, weights):
        """reference vision.py:292-310 (the same function in all three families)."""
        out = {}
        for k, v in weights.items():
            if "position_ids" in k:
                continue
            if "patch_embed.proj.weight" in k:
                out[k] = v if check_array_shape(v) else v.permute(0, 2, 3, 4, 1)
            else:
                out[k] = v
        return out


BLOCK_TENSORS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


class VisionModel(VisionTower):
    def __init__(self, config: VisionConfig, device="cuda"):
        if config.model_type != "qwen2_vl":
            raise ValueError(f"Unsupported model type: {config.model_type}")
        super().__init__(config, device, config.embed_dim, config.hidden_size, int(config.embed_dim * config.mlp_ratio))

    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: sanitized names relative to the tower (`patch_embed.proj.weight`, `blocks.i....`, `merger....`)."""
        wp = self._patch_weight(W)
        # VLM_VIT_ROPE_FUSED=0: plain q / k rows and a separate rope pass (A/B knob); head_dim % 16: what the epilogue takes
        self.rope_fused = os.environ.get("VLM_VIT_ROPE_FUSED", "1") != "0" and self.head_dim % 16 == 0
        self._create(int(self.rope_fused))
        perm = self.qk_perm()
        for i in range(self.config.depth):
            p = f"blocks.{i}."
            t = {n: W[p + n] for n in BLOCK_TENSORS}
            if self.rope_fused:
                for n in ("attn.qkv.weight", "attn.qkv.bias"):
                    t[n] = t[n][perm.to(t[n].device)]
            self._set_block(i, [self._keep(p + n, t[n]) for n in BLOCK_TENSORS])
        self._set_globals([wp] + [self._keep("merger." + n, W["merger." + n]) for n in (
            "ln_q.weight", "ln_q.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias")])

    def _patch_rows(self, hidden_states: torch.Tensor) -> torch.Tensor:
        """The device image processor's pixel_values (image_ops.tag_patch_matrix) already ARE the patch matrix."""
        from ... import image_ops

        if not hidden_states.is_cuda:
            hidden_states = _lib.h2d(hidden_states, self.device)
        x = image_ops.patch_matrix_of(hidden_states, self.patch_dim, self.patch_k)
        if x is None or x.device != hidden_states.device:
            x = super()._patch_rows(hidden_states)          # any other tensor, bf16 included
        return x

    def __call__(self, hidden_states: torch.Tensor, grid_thw, output_hidden_states: Optional[bool] = None):
        """hidden_states: pixel_values [N, C*T*ph*pw] (f32 or bf16, rows as the processor emits them:
        columns ordered (C, T, ph, pw)).  -> [N / merge^2, hidden_size] bf16."""
        return self._forward(self._patch_rows(hidden_states), self._tables(grid_thw))
