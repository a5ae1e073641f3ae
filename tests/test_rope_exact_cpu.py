"""The rotary bar can fail, and its inputs are what they claim to be (tests/rope_exact.py).

For every geometry of the shared table: the lattice builder's assertions hold and the oracle's own GEMV reproduces y bit for
bit (bf16 and 4-bit); the exact reference stays under the mismatch cap and the honest fp32 evaluation passes the bar; and
each mutant of a subtly wrong kernel - a frequency index shifted over the top eight entries, the position through bf16,
cos / sin in bf16, a one-constant fp32 range reduction, the sine's sign flipped in the high half, the partner one element
off, the M-RoPE selector shifted by one, qk_scale without its bf16 rounding, K written one slot on, V in natural key order -
is rounded to bf16 like a kernel output and REJECTED by the same checker the GPU tests call."""
import pytest
import torch

from oracle import ops as O
from oracle import quant as Q
from tests import rope_exact as R

F64, BF = torch.float64, torch.bfloat16


@pytest.mark.parametrize("geo", R.GEOMETRIES, ids=R.geo_id)
def test_lattice_product_is_exact_in_the_oracle(geo):
    Hq, Hkv, D, K, _ = geo
    for M in (1, 2, 16):
        h, nw, W, bias, y = R.lattice_qkv(M, Hq, Hkv, D, K, False, seed=3)
        xn = O.rms_norm(h, nw, R.EPS)
        assert set(xn.abs().unique().tolist()) <= {0.5, 1.0, 2.0}
        assert int((W != 0).sum(1).max()) <= 4
        assert torch.equal(O.linear(xn, W, bias).to(F64), y)
        _, _, (wq, s, b), _, y4 = R.lattice_qkv(M, Hq, Hkv, D, K, True, seed=3)
        assert torch.equal(y4, y)
        assert torch.equal(Q.QW(wq, s, b).linear(xn, bias).to(F64), y)
        # a reversed summation order gives the same bits: nothing but the rotation is left to differ
        assert torch.equal((xn.to(torch.float32).flip(-1) @ W.to(torch.float32).flip(-1).T + bias.to(torch.float32)).to(F64), y)


def _cases():
    for geo in R.GEOMETRIES:
        for sections in R.SECTIONS:
            for scale in (1.0, R.QK_SCALE):
                yield geo, sections, scale


@pytest.mark.parametrize("geo,sections,scale", list(_cases()), ids=lambda v: R.geo_id(v) if isinstance(v, tuple) and len(v) == 5 else str(v))
def test_reference_under_the_cap_honest_fp32_passes_mutants_fail(geo, sections, scale):
    y, pos3, inv = R.cpu_case(geo, seed=3)
    ex, mag = R.exact_mrope(y, pos3, inv, sections, scale)
    name = f"cpu {R.geo_id(geo)} {sections} scale {scale}"
    honest = R.rotate_fp32(y, pos3, inv, sections, scale)
    need, share, _ = R.check_rot(name + " fp32", honest, ex, mag)
    assert need <= 2.5 and share <= R.CAP                     # (fp32 alone: up to 9.2e-5 of the elements, c needed 0.44)
    if scale == 1.0:
        x = y.to(BF).permute(1, 0, 2)[None]                   # [1, H, rows, D]
        sel = O.chunked_position_selector(list(sections), y.shape[-1] // 2)
        assert torch.equal(sel, R.selector(sections, y.shape[-1] // 2))
        orc = O.mrope_apply(x, pos3[:, None, :], inv, sel, "fused")[0].permute(1, 0, 2)
        R.check_rot(name + " oracle fused", orc, ex, mag)
        assert torch.equal(orc, honest)
    at0 = (pos3 == 0).all(0)
    assert bool(at0.any())
    assert torch.equal(honest[at0].to(F64), R.rne_bf16(y[at0] * scale))
    rejected = []
    for d in R.ROT_MUTANTS:
        if d == "scale_unrounded" and scale == 1.0:
            continue                                          # (the identity at scale 1: nothing to catch)
        mutant = R.rotate_fp32(y, pos3, inv, sections, scale, defect=d)
        bad, c_need, sh = R.rot_report(mutant, ex, mag)
        print(f"ROPE-EXACT mutant {d:16s} {name}: {bad} over the bar, c needed {c_need:.3g}, != rne(ex) {sh:.2e}")
        assert not R.passes(mutant, ex, mag), (d, name)
        rejected.append(d)
    assert len(rejected) >= len(R.ROT_MUTANTS) - 1


@pytest.mark.parametrize("geo", R.GEOMETRIES, ids=R.geo_id)
def test_pool_check_rejects_a_wrong_slot_and_a_wrong_v_order(geo):
    """a write to a wrong slot that REPLACES a right one keeps the count of written words: the sentinel check sees it"""
    Hq, Hkv, D, K, theta = geo
    case = dict(entry="gemv_qkv_rope_kvwrite_ws", gi=R.GEOMETRIES.index(geo), M=16)
    for paged in (True, False):
        i = R.fused_inputs(case, paged)
        k_bf = R.rne_bf16(i["ex"][:, Hq:]).to(BF)
        v_bf = i["y3"][:, Hq + Hkv:].to(BF)
        for defect in (None,) + R.POOL_MUTANTS:
            kpool, vpool = R.pools_new(i["n_pages"], Hkv, D)
            R.pools_write(kpool, vpool, k_bf, v_bf, i["pages"], i["within"], defect)
            k_rows, v_rows, stray = R.pools_read(kpool, vpool, i["pages"], i["within"])
            if defect is None:
                R.check_pools(f"cpu pools {R.geo_id(geo)}", k_rows, v_rows, stray, i["ex"][:, Hq:], i["mag"][:, Hq:], v_bf.to(F64))
                continue
            with pytest.raises(AssertionError):
                R.check_pools(f"cpu pools {defect}", k_rows, v_rows, stray, i["ex"][:, Hq:], i["mag"][:, Hq:], v_bf.to(F64))


def test_case_table_reaches_every_form():
    forms = {(R.ENTRIES[c["entry"]][0], c["form"]) for c in R.FUSED_CASES}
    assert forms == {(False, "dot2c"), (False, "mfma"), (False, "mfma2"), (True, "dot2c"), (True, "mfma2")}, forms
    # the 4-bit first form is the second form's fall-back: every 4-bit workspace case reaches it with the second form off
    assert all(R.form_of(True, True, c["M"], R.GEOMETRIES[c["gi"]][3], mfma2=False) == "mfma"
               for c in R.FUSED_CASES if c["entry"] == "gemv_w4_qkv_rope_kvwrite_ws")
    # what the entry points refuse: 3 and 5 rows (neither a v_dot2c row count nor enough for the matrix cores), and 9 rows
    # at K = 4096 without a workspace (two K segments there, and the activations pass 64 KiB)
    assert {(c["entry"], c["M"]) for c in R.REFUSED_CASES} == {("gemv_qkv_rope_kvwrite", 3), ("gemv_qkv_rope_kvwrite", 5),
                                                                ("gemv_qkv_rope_kvwrite", 9)}
    assert {R.GEOMETRIES[c["gi"]][3] for c in R.REFUSED_CASES if c["M"] == 9} == {4096}
