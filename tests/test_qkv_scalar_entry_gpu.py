"""Bit 6 (64) of VLM_TUNE_GEMV_VARIANT (include/vlm_hip.h): the one-row qkv launch at hidden <= 1536 and Hq * D <= 1536 takes
(Hq, Hkv, D) and long_from from a preloaded argument slot and fetches pos / slot / inv_freq on the scalar path, so nothing
but its x / norm_w / bias loads stands ahead of its weight stream.  It changes when the operands arrive, never what is
computed: the bit on is held to the BYTES of the bit off, in the same library (the off side is held to the exact result by
tests/test_kernarg_order_gpu.py and tests/test_ops_gpu.py).

Fused qkv (vlm_gemv_qkv_rope_kvwrite) over
    hidden 1536, Hq 12, Hkv 2, D 128     the headline shape
    hidden  128, Hq  2, Hkv 1, D  64     masked chunks (16 chunks on 64 lanes), waves past the last row
at slot = 0, 63, 64 and 1023 (first and last slot of a page, first of the next, last page of the table) with pos != slot, the
identity layout and a permuted block table, the q rows at a pitch of their own (N + 8; the entry point takes no other
leading dimension: x and W are dense by its signature), pools pre-filled with random bytes: equal q rows, equal K / V bytes
written, and every other byte of the pools equal (the whole pools are compared, and must differ from their initial fill).
M = 2, and hidden 3584 with 28 heads at M = 1 (Hq * D > 1536), keep today's entry: the same comparison shows the launcher
still takes them under the bit.

rope_qk_scale != 1 and the two-table rope (long_from > 0, slots on both sides of it) are arguments of the engine's qkv call
alone (vlm_llm_config.rope_qk_scale / rope_long_from - the C entry point of the bare op carries neither), so they are held
through the engine: the tiny Phi-3.5-vision model (qk_scale 1.19, two tables, hidden 384, 4 heads of 96) decodes one row
across original_max_position_embeddings with the bit off and on, and every step's logits - which read the K / V rows the
steps before them wrote - must be equal byte for byte.  Scale 1 with one table (long_from = 0) through the engine is the tiny
Qwen2-VL of tests/test_engine_tail_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from oracle import phi3_v as op
from oracle import qwen2_vl as oq
from tests.helpers import build_phi3v_model, build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BIT = 64
SHAPES = [(1536, 12, 2, 128), (128, 2, 1, 64)]
WIDE = (3584, 28, 4, 128)
MAX_PAGES = 16


@pytest.fixture(scope="module")
def variant():
    """set(on): the process-wide variant (travels through vlm_llm_set_tuning: the module builds a tiny model for its handle)"""
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    lm = build_product_model(cfg, W, kv_pool_tokens=1024, max_seqs=2).language_model
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~BIT
    yield lambda on: lm.apply_tuning(gemv_variant=base | (BIT if on else 0))
    lm.apply_tuning()


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(BF)


@pytest.fixture(scope="module")
def operands():
    """weights, bias and the pools' initial fill of a shape, made once"""
    made = {}

    def get(shape, M):
        if (shape, M) not in made:
            hidden, Hq, Hkv, D = shape
            N = (Hq + 2 * Hkv) * D
            n_pages = MAX_PAGES * M
            made[(shape, M)] = dict(
                h=_rnd(M, hidden, seed=3), nw=(1 + 0.1 * _rnd(hidden, seed=4).float()).to(BF),
                w=_rnd(N, hidden, seed=5, scale=0.05), b=_rnd(N, seed=6, scale=0.3), inv=O.mrope_inv_freq(D, 1e6).cuda(),
                k_init=_rnd(n_pages, Hkv, D // 8, 64, 8, seed=7), v_init=_rnd(n_pages, Hkv, D, 64, seed=8),
                # row m's pages run backwards from the end of the pool
                perm=torch.arange(n_pages - 1, -1, -1, dtype=torch.int32).reshape(M, MAX_PAGES).cuda())
        return made[(shape, M)]

    return get


def on_against_off(variant, operands, shape, M, slot0, pos0, layout):
    from mlx_vlm_amd import ops

    hidden, Hq, Hkv, D = shape
    N = (Hq + 2 * Hkv) * D
    o = operands(shape, M)
    pos = torch.tensor([pos0, 37][:M], dtype=torch.int32, device="cuda")
    slot = torch.tensor([slot0, 70][:M], dtype=torch.int32, device="cuda")
    assert all(int(p) != int(s) for p, s in zip(pos, slot))
    bt = o["perm"] if layout == "permuted" else None

    def run(on):
        variant(on)
        kpool, vpool = o["k_init"].clone(), o["v_init"].clone()
        buf = torch.full((M, N + 8), float("nan"), dtype=BF, device="cuda")
        out = buf[:, :N]
        ops.gemv_qkv_rope_kvwrite(o["h"], o["nw"], o["w"], o["b"], Hq, Hkv, D, pos, slot, o["inv"], bt, kpool, vpool, out=out,
                                  max_pages=MAX_PAGES)
        return buf.view(torch.int16)[:, :Hq * D].clone(), buf.view(torch.int16)[:, N:].clone(), kpool.view(torch.int16), vpool.view(torch.int16)

    q0, pad0, k0, v0 = run(False)
    q1, pad1, k1, v1 = run(True)
    assert bool(torch.isfinite(q0.view(BF).float()).all())
    written_k = int((k0 != o["k_init"].view(torch.int16)).sum())
    written_v = int((v0 != o["v_init"].view(torch.int16)).sum())
    assert 0 < written_k <= M * Hkv * D and 0 < written_v <= M * Hkv * D                 # one token per row, nothing else
    assert torch.equal(q1, q0) and torch.equal(pad1, pad0)
    assert torch.equal(k1, k0) and torch.equal(v1, v0)


def test_qkv_scalar_entry_under_a_scale_and_two_rope_tables(variant):
    """Phi-3.5-vision, tiny: q / k scaled by a typed factor != 1 before the rotation, short and long frequency tables with
    long_from = original_max_position_embeddings.  One row decodes 8 steps from offset long_from - 4: slots on both sides
    of the limit.  Bit off vs on: the logits of every step, byte for byte."""
    cfg = op.tiny_cfg()
    W = op.random_weights(cfg, seed=779, dtype=BF, std=0.04, embed_std=0.2)
    model = build_phi3v_model(cfg, W, kv_pool_tokens=16384, max_seqs=4)
    lm = model.language_model
    lim = cfg.text.original_max_position_embeddings
    assert lm.rope_long_from == lim and float(lm.args.rope_qk_scale) != 1.0
    rng = np.random.default_rng(912)
    prompt = rng.integers(3, 1000, lim - 4).astype(np.int64)
    forced = rng.integers(3, 1000, 8)
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~BIT

    def run(on):
        lm.apply_tuning(gemv_variant=base | (BIT if on else 0))
        c = lm.make_cache()
        lm(prompt[None], cache=c, logits_to_keep=1)
        rows = [lm(np.array([[int(t)]]), cache=c).logits[0, 0].clone() for t in forced]
        assert c[0].offset == lim + 4
        c[0]._seq.release()
        return torch.stack(rows)

    try:
        off, on = run(False), run(True)
    finally:
        lm.apply_tuning()
    assert bool(torch.isfinite(off.float()).all())
    assert not torch.equal(off[3], off[4])
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))


@pytest.mark.parametrize("layout", ["identity", "permuted"])
@pytest.mark.parametrize("slot0,pos0", [(0, 5), (63, 1000), (64, 63), (1023, 2047)])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "h%d_%d_%d_%d" % s)
def test_qkv_scalar_entry_gives_the_bytes_of_the_vector_entry(variant, operands, shape, M, slot0, pos0, layout):
    on_against_off(variant, operands, shape, M, slot0, pos0, layout)


def test_wide_heads_keep_todays_entry(variant, operands):
    on_against_off(variant, operands, WIDE, 1, 64, 63, "identity")
