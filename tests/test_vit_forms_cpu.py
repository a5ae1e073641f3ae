"""vlm_vit_forward's three forms (first / Qwen2.5 / Qwen3) without a device: every refusal returns its code before the first
launch, so the calls run on the host with pointers that are compared and never dereferenced; and the host side the three
VisionModels share (the table cache, sanitize)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mlx_vlm_amd import _lib
from tests import qwen2_5_vl_ref as R25
from tests import qwen3_vl_ref as R3
from tests.helpers import model_config_from_oracle

P = 0x10000          # a pointer that is never read
FIRST, Q25, Q3 = 0, _lib.VIT_FORM_QWEN2_5, _lib.VIT_FORM_QWEN3
HEAD = {FIRST: (160, 2), Q25: (160, 2), Q3: (128, 2), Q25 | Q3: (160, 2)}          # embed_dim, heads: head_dim 80, 80, 64, 80


def _code(flags, cfg=None, args=None, taps=(0,), bpatch=P, split=False, null_args=False):
    """the return code of one vlm_vit_forward call on a handle of `flags` that is valid for its form but for what the case names:
    cfg / args override fields of vlm_vit_config / vlm_vit_args, taps = the blocks with a tap merger, split = sin_tab not
    directly behind cos_tab"""
    L = _lib.lib()
    E, H = HEAD[flags & (Q25 | Q3)]
    c = dict(depth=2, embed_dim=E, n_heads=H, mlp_hidden=192, patch_k=1216, merge=2, out_dim=256, ln_eps=1e-6, qk_interleaved=flags)
    c.update(cfg or {})
    h = C.c_void_p()
    assert L.vlm_vit_create(C.byref(_lib.VitConfig(**c)), C.byref(h)) == 0
    try:
        for i in range(c["depth"]):
            blk = _lib.VitBlock(*[P] * 12, *([P] * 6 if i in taps else [None] * 6))
            assert L.vlm_vit_set_block(h, i, C.byref(blk)) == 0
        assert L.vlm_vit_set_globals(h, C.byref(_lib.VitGlobals(*[P] * 7, bpatch))) == 0
        a = dict(patches=P, N=16, cos_tab=P, cu_seqlens=P, nseg=1, total_qblocks=1, x=P, xn=P, qkv=P, attn=P, mlp=P, mrg=P, out=P,
                 uniform_segments=1, win_cu_seqlens=P, win_nseg=4, win_total_qblocks=4, win_max_seg=4, win_one_tile=0,
                 window_index=P, reverse_index=P, fullatt_mask=2, pos_rows=P, tap_out=P, n_taps=len(taps))
        a.update(args or {})
        hd = c["embed_dim"] // c["n_heads"]
        a["sin_tab"] = a["cos_tab"] + a["N"] * (hd // 2) * 4 + (64 if split else 0)
        return L.vlm_vit_forward(h, None if null_args else C.byref(_lib.VitArgs(**a)), None)
    finally:
        L.vlm_vit_destroy(h)


I = _lib.VIT_QK_INTERLEAVED
CASES = [
    # common to all forms
    ("null args", dict(flags=FIRST | I, null_args=True), 1),
    ("null patches", dict(flags=FIRST | I, args=dict(patches=None)), 1),
    ("N = 0", dict(flags=Q25 | I, args=dict(N=0)), 1),
    ("N < 0", dict(flags=Q3 | I, args=dict(N=-4)), 1),
    ("both form bits", dict(flags=Q25 | Q3 | I), 1),
    # first form
    ("first: N % merge^2", dict(flags=FIRST | I, args=dict(N=18)), 2),
    ("first: N % merge^2, plain weights", dict(flags=FIRST, args=dict(N=18), split=True), 2),
    ("first: interleaved, split table", dict(flags=FIRST | I, split=True), 1),
    ("first: N % merge^2 and split table", dict(flags=FIRST | I, args=dict(N=18), split=True), 2),
    # Qwen2.5 form
    ("2.5: N % merge^2", dict(flags=Q25 | I, args=dict(N=18)), 2),
    ("2.5: head_dim % 16", dict(flags=Q25 | I, cfg=dict(embed_dim=168)), 2),
    ("2.5: depth > 64", dict(flags=Q25 | I, cfg=dict(depth=65)), 2),
    ("2.5: out_dim > merge^2 mlp_hidden", dict(flags=Q25 | I, cfg=dict(out_dim=769)), 2),
    ("2.5: bit 0 missing", dict(flags=Q25), 1),
    ("2.5: split table", dict(flags=Q25 | I, split=True), 1),
    ("2.5: null win_cu_seqlens", dict(flags=Q25 | I, args=dict(win_cu_seqlens=None)), 1),
    ("2.5: null window_index", dict(flags=Q25 | I, args=dict(window_index=None)), 1),
    ("2.5: null reverse_index", dict(flags=Q25 | I, args=dict(reverse_index=None)), 1),
    ("2.5: null cu_seqlens", dict(flags=Q25 | I, args=dict(cu_seqlens=None)), 1),
    ("2.5: win_nseg = 0", dict(flags=Q25 | I, args=dict(win_nseg=0)), 1),
    ("2.5: one tile, win_max_seg 65", dict(flags=Q25 | I, args=dict(win_one_tile=1, win_max_seg=65)), 2),
    ("2.5: one tile, head_dim 64", dict(flags=Q25 | I, cfg=dict(embed_dim=128), args=dict(win_one_tile=1)), 2),
    ("2.5: depth > 64 and bit 0 missing", dict(flags=Q25, cfg=dict(depth=65)), 2),
    ("2.5: out_dim and null window_index", dict(flags=Q25 | I, cfg=dict(out_dim=769), args=dict(window_index=None)), 2),
    ("2.5: one tile 65 and null reverse_index", dict(flags=Q25 | I, args=dict(win_one_tile=1, win_max_seg=65, reverse_index=None)), 1),
    # Qwen3 form
    ("3: N % merge^2", dict(flags=Q3 | I, args=dict(N=18)), 2),
    ("3: head_dim 72", dict(flags=Q3 | I, cfg=dict(embed_dim=144)), 2),
    ("3: head_dim 96", dict(flags=Q3 | I, cfg=dict(embed_dim=192)), 2),
    ("3: embed_dim merge^2 > 8192", dict(flags=Q3 | I, cfg=dict(embed_dim=2176, n_heads=17)), 2),
    ("3: bit 0 missing", dict(flags=Q3), 1),
    ("3: split table", dict(flags=Q3 | I, split=True), 1),
    ("3: null cu_seqlens", dict(flags=Q3 | I, args=dict(cu_seqlens=None)), 1),
    ("3: null pos_rows", dict(flags=Q3 | I, args=dict(pos_rows=None)), 1),
    ("3: null bpatch", dict(flags=Q3 | I, bpatch=None), 1),
    ("3: n_taps too small", dict(flags=Q3 | I, taps=(0, 1), args=dict(n_taps=1)), 1),
    ("3: n_taps too large", dict(flags=Q3 | I, taps=(), args=dict(n_taps=1)), 1),
    ("3: taps without tap_out", dict(flags=Q3 | I, args=dict(tap_out=None)), 1),
    ("3: head_dim 72 and null pos_rows", dict(flags=Q3 | I, cfg=dict(embed_dim=144), args=dict(pos_rows=None)), 2),
    ("3: head_dim 72 and n_taps", dict(flags=Q3 | I, cfg=dict(embed_dim=144), args=dict(n_taps=2)), 2),
]


@pytest.mark.parametrize("name,kw,want", CASES, ids=[c[0] for c in CASES])
def test_refusal_codes(name, kw, want):
    """1 = bad argument, 2 = unsupported shape; a shape refusal and an argument refusal together give 2, except the one-tile
    shape check of the Qwen2.5 form, which stands behind that form's argument checks"""
    assert _code(**kw) == want


# ---------------------------------------------------------------- the shared host side
def _towers():
    from oracle import qwen2_vl as oq
    from mlx_vlm_amd.models import qwen2_5_vl, qwen2_vl, qwen3_vl

    return {
        "qwen2_vl": qwen2_vl.VisionModel(model_config_from_oracle(oq.tiny_cfg()).vision_config, device="cpu"),
        "qwen2_5_vl": qwen2_5_vl.VisionModel(
            qwen2_5_vl.VisionConfig.from_dict(R25.model_config_dict(R25.tiny_cfg())["vision_config"]), device="cpu"),
        "qwen3_vl": qwen3_vl.VisionModel(
            qwen3_vl.VisionConfig.from_dict(R3.model_config_dict(R3.tiny_cfg())["vision_config"]), device="cpu"),
    }


@pytest.mark.parametrize("family", ["qwen2_vl", "qwen2_5_vl", "qwen3_vl"])
def test_table_cache(family):
    """one entry per grid_thw, the same object on a hit, everything dropped when a 66th grid arrives"""
    vm = _towers()[family]
    a = vm._tables(np.array([(1, 4, 6)]))
    assert vm._tables(np.array([(1, 4, 6)])) is a and vm._tables([(1, 4, 6)]) is a
    b = vm._tables(np.array([(1, 4, 6), (1, 2, 2)]))
    assert b is not a and vm._tables(np.array([(1, 4, 6)])) is a
    for i in range(64):                                 # 2 + 64 = 66 distinct grids
        vm._tables(np.array([(1, 2, 2 * (i + 2))]))
    assert len(vm._tab_cache) <= 2
    assert vm._tables(np.array([(1, 4, 6)])) is not a


@pytest.mark.parametrize("family", ["qwen2_vl", "qwen2_5_vl", "qwen3_vl"])
def test_sanitize_without_an_instance(family):
    VisionModel = type(_towers()[family])
    conv = torch.arange(8 * 3 * 2 * 14 * 14, dtype=torch.float32).reshape(8, 3, 2, 14, 14)          # (O, C, T, H, W)
    last = conv.permute(0, 2, 3, 4, 1)
    w = {"patch_embed.proj.weight": conv, "blocks.0.attn.qkv.weight": torch.zeros(3), "embeddings.position_ids": torch.zeros(2)}
    out = VisionModel.sanitize(None, w)
    assert sorted(out) == ["blocks.0.attn.qkv.weight", "patch_embed.proj.weight"]
    assert torch.equal(out["patch_embed.proj.weight"], last) and out["blocks.0.attn.qkv.weight"] is w["blocks.0.attn.qkv.weight"]
    # already channels-last: left as it is
    assert VisionModel.sanitize(None, {"patch_embed.proj.weight": last})["patch_embed.proj.weight"] is last
