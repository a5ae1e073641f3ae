"""Qwen3-VL vision tower on MI355X - host mirror of the reference's mlx_vlm/models/qwen3_vl/vision.py (VisionModel, same
constructor / call / sanitize contract; the call returns (features, [DeepStack tap features])).

The numerical work is one call into the native ViT engine in its Qwen3 form (csrc/engine.hip: patch GEMM + bias + position rows
-> depth x [LayerNorm, qkv GEMM + bias + 2-D rope, attention over cu_seqlens, proj GEMM + bias + residual, LayerNorm, fc1 GEMM +
bias + tanh-GELU, fc2 GEMM + bias + residual; behind a tap block the post-shuffle merger] -> PatchMerger).  The host prepares the
integer tables from `grid_thw`, which the reference also does on the host with .tolist() (vision.py:238-377): rotary rows,
cu_seqlens, and the four corner indices and weights of the bilinear interpolation of `pos_embed`.  The interpolation itself
(four row gathers, three typed multiplies-and-adds per element, once per call) stays torch on the device.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ..._lib import check
from ..qwen2_vl.vision import check_array_shape, rot_pos_ids
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


class VisionModel:
    def __init__(self, config: VisionConfig, device="cuda"):
        self.config = config
        self.model_type = config.model_type
        if self.model_type != "qwen3_vl":
            raise ValueError(f"Unsupported model type: {self.model_type}")
        self.spatial_merge_size = config.spatial_merge_size
        self.device = device
        self.embed_dim = config.hidden_size
        self.num_heads = config.num_heads
        self.head_dim = config.hidden_size // config.num_heads
        self.patch_dim = config.in_channels * config.temporal_patch_size * config.patch_size * config.patch_size
        self.patch_k = (self.patch_dim + 63) // 64 * 64          # K of the patch GEMM, zero padded
        self.mlp_hidden = (config.intermediate_size + MLP_PAD - 1) // MLP_PAD * MLP_PAD
        self.num_grid_per_side = int(config.num_position_embeddings ** 0.5)
        self.deepstack_visual_indexes = list(config.deepstack_visual_indexes)
        self._handle = None
        self._w: Dict[str, torch.Tensor] = {}
        self._tab_cache: Dict[tuple, dict] = {}

    @property
    def dtype(self):
        return torch.bfloat16

    # ------------------------------------------------------------------ weights
    def load_weights(self, W: Dict[str, torch.Tensor]):
        """W: sanitized names relative to the tower (`patch_embed.proj.{weight,bias}`, `pos_embed.weight`, `blocks.i....`,
        `merger....`, `deepstack_merger_list.j....`)."""
        c, dev = self.config, self.device
        if self.head_dim not in SUPPORTED_HEAD_DIMS:
            raise NotImplementedError(f"vision head_dim = {self.head_dim}: the tower's rope-in-epilogue GEMM and attention kernel "
                                      f"are built for head_dim in {SUPPORTED_HEAD_DIMS} (Qwen3-VL 2B / 4B: 64; the 8B / 32B "
                                      "towers have 72)")
        taps = self.deepstack_visual_indexes
        if len(set(taps)) != len(taps) or any(i < 0 or i >= c.depth for i in taps):
            raise ValueError(f"deepstack_visual_indexes = {taps}: distinct block indices below depth = {c.depth}")
        if c.hidden_size * c.spatial_merge_size ** 2 > 8192:
            raise NotImplementedError("the post-shuffle LayerNorm is built for merge^2 * hidden_size <= 8192")
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
        bp = keep("patch_embed.proj.bias", W["patch_embed.proj.bias"])
        keep("pos_embed.weight", W["pos_embed.weight"])

        E, hd, half, I, Ip = c.hidden_size, self.head_dim, self.head_dim // 2, c.intermediate_size, self.mlp_hidden
        cfg = _lib.VitConfig(c.depth, E, c.num_heads, Ip, self.patch_k, c.spatial_merge_size, c.out_hidden_size, 1e-6,
                             _lib.VIT_QK_INTERLEAVED | _lib.VIT_FORM_QWEN3)      # nn.LayerNorm(eps=1e-6): vision.py:111,178-179
        inter = torch.stack([torch.arange(half), torch.arange(half) + half], dim=1).reshape(-1)
        perm = (torch.arange(2 * c.num_heads)[:, None] * hd + inter[None, :]).reshape(-1)
        qk_perm = torch.cat([perm, torch.arange(2 * E, 3 * E)])
        h = C.c_void_p()
        check(L.vlm_vit_create(C.byref(cfg), C.byref(h)), "vit_create")
        self._handle = h
        for i in range(c.depth):
            p = f"blocks.{i}."
            w1 = W[p + "mlp.linear_fc1.weight"].new_zeros(Ip, E)
            w1[:I] = W[p + "mlp.linear_fc1.weight"]
            b1 = W[p + "mlp.linear_fc1.bias"].new_zeros(Ip)
            b1[:I] = W[p + "mlp.linear_fc1.bias"]
            w2 = W[p + "mlp.linear_fc2.weight"].new_zeros(E, Ip)
            w2[:, :I] = W[p + "mlp.linear_fc2.weight"]
            ptrs = [keep(p + "norm1.weight", W[p + "norm1.weight"]), keep(p + "norm1.bias", W[p + "norm1.bias"]),
                    keep(p + "attn.qkv.weight", W[p + "attn.qkv.weight"][qk_perm.to(W[p + "attn.qkv.weight"].device)]),
                    keep(p + "attn.qkv.bias", W[p + "attn.qkv.bias"][qk_perm.to(W[p + "attn.qkv.bias"].device)]),
                    keep(p + "attn.proj.weight", W[p + "attn.proj.weight"]), keep(p + "attn.proj.bias", W[p + "attn.proj.bias"]),
                    keep(p + "norm2.weight", W[p + "norm2.weight"]), keep(p + "norm2.bias", W[p + "norm2.bias"]),
                    keep(p + "mlp.linear_fc1.weight", w1), keep(p + "mlp.linear_fc1.bias", b1),
                    keep(p + "mlp.linear_fc2.weight", w2), keep(p + "mlp.linear_fc2.bias", W[p + "mlp.linear_fc2.bias"])]
            tap = [None] * 6
            if i in taps:
                q = f"deepstack_merger_list.{taps.index(i)}."
                tap = [keep(q + n, W[q + n]) for n in ("norm.weight", "norm.bias", "linear_fc1.weight", "linear_fc1.bias",
                                                       "linear_fc2.weight", "linear_fc2.bias")]
            blk = _lib.VitBlock(*[t.data_ptr() for t in ptrs], *[t.data_ptr() if t is not None else None for t in tap])
            check(L.vlm_vit_set_block(h, i, C.byref(blk)), "vit_set_block")
        m = {n: keep("merger." + n, W["merger." + n]) for n in ("norm.weight", "norm.bias", "linear_fc1.weight", "linear_fc1.bias",
                                                                 "linear_fc2.weight", "linear_fc2.bias")}
        gl = _lib.VitGlobals(wp.data_ptr(), m["norm.weight"].data_ptr(), m["norm.bias"].data_ptr(),
                             m["linear_fc1.weight"].data_ptr(), m["linear_fc1.bias"].data_ptr(), m["linear_fc2.weight"].data_ptr(),
                             m["linear_fc2.bias"].data_ptr(), bp.data_ptr())
        check(L.vlm_vit_set_globals(h, C.byref(gl)), "vit_set_globals")

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().vlm_vit_destroy(self._handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ host tables
    def rot_pos_emb(self, grid_thw) -> torch.Tensor:
        """freqs [N, head_dim/2] fp32 (reference vision.py:238-297)"""
        g = np.asarray(grid_thw)
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
            freqs = self.rot_pos_emb(grid_thw)
            lens = []
            for t, h, w in key:
                lens += [h * w] * t
            cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            cs = _lib.h2d(torch.stack([torch.cos(freqs), torch.sin(freqs)]).contiguous(), self.device)   # ONE table
            idx, wt = pos_embed_tables(grid_thw, self.num_grid_per_side, self.spatial_merge_size)
            hit = {"cos": cs[0], "sin": cs[1], "cs": cs, "cu": _lib.h2d(cu, self.device), "nseg": len(lens),
                   "nqb": int(sum((n + 127) // 128 for n in lens)), "uniform": int(len(set(lens)) == 1),
                   "pos_idx": _lib.h2d(idx, self.device),
                   "pos_w": _lib.h2d(torch.from_numpy(wt).to(torch.bfloat16), self.device)}   # weights in the table's dtype (342)
            if len(self._tab_cache) > 64:
                self._tab_cache.clear()
            self._tab_cache[key] = hit
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
        from ... import ops

        c = self.config
        if not hidden_states.is_cuda:
            hidden_states = _lib.h2d(hidden_states, self.device)
        N = hidden_states.shape[0]
        if hidden_states.dtype != torch.float32:
            hidden_states = hidden_states.to(torch.float32)          # bf16 -> fp32 -> bf16 is lossless
        x = ops.cast_pad(hidden_states.contiguous(), self.patch_k)
        t = self._tables(grid_thw)
        pos_rows = self.fast_pos_embed_interpolate(grid_thw).contiguous()
        E, dev = c.hidden_size, self.device
        mm = self.spatial_merge_size ** 2
        bf = torch.bfloat16
        ws = {n: torch.empty(N, d, dtype=bf, device=dev) for n, d in
              (("x", E), ("xn", E), ("qkv", 3 * E), ("attn", E), ("mlp", self.mlp_hidden))}
        mrg = torch.empty(N // mm, E * mm, dtype=bf, device=dev)
        out = torch.empty(N // mm, c.out_hidden_size, dtype=bf, device=dev)
        n_taps = len(self.deepstack_visual_indexes)
        tap_out = torch.empty(n_taps, N // mm, c.out_hidden_size, dtype=bf, device=dev)
        a = _lib.VitArgs(x.data_ptr(), N, t["cos"].data_ptr(), t["sin"].data_ptr(), t["cu"].data_ptr(), t["nseg"], t["nqb"],
                         ws["x"].data_ptr(), ws["xn"].data_ptr(), ws["qkv"].data_ptr(), ws["attn"].data_ptr(),
                         ws["mlp"].data_ptr(), mrg.data_ptr(), out.data_ptr(), t["uniform"])
        a.pos_rows, a.tap_out, a.n_taps = pos_rows.data_ptr(), tap_out.data_ptr() if n_taps else None, n_taps
        check(_lib.lib().vlm_vit_forward(self._handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "vit_forward")
        return out, [tap_out[j] for j in range(n_taps)]

    # ------------------------------------------------------------------ checkpoint key/layout fixups
    def sanitize(self, weights):
        """reference vision.py:427-445."""
        out = {}
        for k, v in weights.items():
            if "position_ids" in k:
                continue
            if "patch_embed.proj.weight" in k:
                out[k] = v if check_array_shape(v) else v.permute(0, 2, 3, 4, 1)
            else:
                out[k] = v
        return out
