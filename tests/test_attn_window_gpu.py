"""The one-tile window attention (csrc/attn_window.hip; vlm_attn_prefill flag bit 3 / ops.attn_prefill(one_tile_max_seg=...)):
non-causal attention over segments of 1..64 tokens at D = 80, q / k / v as views of one qkv buffer.

Every case is held to the exactly rounded float64 result at the class the general kernel has at D = 80 ("single": one bf16 P),
and to the general kernel on the same inputs at test_attn_prefill's bar.  Whether a case also meets the "hilo" class is printed
(pytest -s), not asserted.  Measured on an MI355X: rel-rms 1.7e-3 .. 2.1e-3 against the exact result (bar 3e-3), elementwise need
1.7e-3 .. 5.3e-3 at 2 ulps (bar 2e-2); "hilo" (5e-4) is NOT met - P is one bf16 operand, as in the general kernel at D = 80 -
except where the softmax is one-hot (a single key, the spike cases), which come out exactly rounded."""
import numpy as np
import pytest
import torch

from tests import attn_exact as A
from tests.helpers import bf16_close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H, D = 2, 80
SCALE = D ** -0.5


def _seeded_37():
    """37 lengths from 1..64 whose total is no multiple of 64"""
    lens = np.random.default_rng(37).integers(1, 65, 37).tolist()
    if sum(lens) % 64 == 0:
        lens[0] = lens[0] % 64 + 1
    assert sum(lens) % 64 != 0 and len(lens) == 37 and 1 <= min(lens) and max(lens) <= 64
    return lens


CASES = {
    "one64": [64], "one4": [4], "one1": [1], "edges": [64, 64, 32, 32, 32, 16, 64, 4], "odd": [7, 63, 64, 1, 33],
    "seeded37": _seeded_37(),
}


def _inputs(lens, seed, spike=False):
    T = sum(lens)
    q, k, v = A.rnd(T, H, D, seed=seed), A.rnd(T, H, D, seed=seed + 1), A.rnd(T, H, D, seed=seed + 2)
    if spike:
        # one key per segment with a logit near +60 against every query, the rest near 0: exp() of the raw scores would overflow
        # a kernel that forgot the max subtraction is caught by the first such row
        q = (torch.ones(T, H, D) * 2.0).to(BF)
        k = A.rnd(T, H, D, seed=seed + 1, scale=0.02)
        off = 0
        for i, n in enumerate(lens):
            k[off + (i * 5) % n] = (torch.ones(H, D) * (60.0 / (2.0 * D * SCALE))).to(BF)
            off += n
    return q, k, v


def _run(q, k, v, lens, one_tile=True, out=None, max_seg=None):
    from mlx_vlm_amd import ops

    T = q.shape[0]
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).cuda()
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    if one_tile:
        return ops.attn_prefill(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], cu, None, H, H, D, SCALE, False, out=out,
                                one_tile_max_seg=max(lens) if max_seg is None else max_seg)
    nqb = sum((n + 127) // 128 for n in lens)
    return ops.attn_prefill(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], cu, nqb, H, H, D, SCALE, False, out=out)


def _check(name, lens, q, k, v):
    T = sum(lens)
    out = _run(q, k, v, lens).view(T, H, D)
    exact = A.prefill_exact(q, k, v, lens, SCALE, False, dev="cuda")
    segs = A.query_rows(lens)[1]
    assert A.prefill_class(D) == "single"
    A.check(f"attn_window {name}", out, exact, "single", segs)
    ok_hilo, _, _, rep = A.measure(out, exact, "hilo", segs)
    print(f"ATTN-WINDOW {name:24s} meets hilo: {ok_hilo}  {rep}")
    general = _run(q, k, v, lens, one_tile=False).view(T, H, D)
    ok, rep = bf16_close(out, general, ulps=2, atol_rms=2e-2)
    assert ok, (name, rep)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_window_attention_vs_exact_and_general_kernel(name):
    lens = CASES[name]
    _check(name, lens, *_inputs(lens, seed=100 + len(lens)))


@pytest.mark.parametrize("name", ["edges", "odd", "one1"])
def test_spike_logit_needs_the_max_subtraction(name):
    lens = CASES[name]
    q, k, v = _inputs(lens, seed=300, spike=True)
    out = _check(name + "/spike", lens, q, k, v)
    assert bool(torch.isfinite(out.float()).all())


def test_a_segments_rows_do_not_depend_on_its_neighbours():
    """cu covers every row (there are none outside a segment); the output rows of one segment stay bit-identical when the
    inputs of the segments around it change"""
    lens = CASES["edges"]
    q, k, v = _inputs(lens, seed=400)
    base = _run(q, k, v, lens).cpu()
    off = np.concatenate([[0], np.cumsum(lens)])
    for s in (0, 3, len(lens) - 1):
        q2, k2, v2 = _inputs(lens, seed=500 + s)
        for t in (q2, k2, v2):
            t[off[s]:off[s + 1]] = 0
        keep = torch.zeros(sum(lens), dtype=torch.bool)
        keep[off[s]:off[s + 1]] = True
        for src, dst in ((q, q2), (k, k2), (v, v2)):
            dst[keep] = src[keep]
        other = _run(q2, k2, v2, lens).cpu()
        assert torch.equal(other[keep], base[keep])
        assert not torch.equal(other[~keep], base[~keep])


def test_refusals_leave_the_output_untouched():
    """D = 128, a declared maximum of 65 and Hq != Hkv return the shape error with nothing enqueued"""
    from mlx_vlm_amd import _lib, ops

    lens = [64, 4]
    T = sum(lens)
    q, k, v = _inputs(lens, seed=600)
    out = torch.full((T, H * D), 7.0, dtype=BF, device="cuda")
    with pytest.raises(_lib.VlmHipError, match="rc=2"):
        _run(q, k, v, lens, out=out, max_seg=65)
    q128 = A.rnd(T, 3 * H * 128, seed=601).cuda()
    cu = torch.tensor([0, 64, 68], dtype=torch.int32).cuda()
    out128 = torch.full((T, H * 128), 7.0, dtype=BF, device="cuda")
    with pytest.raises(_lib.VlmHipError, match="rc=2"):
        ops.attn_prefill(q128, q128[:, H * 128:], q128[:, 2 * H * 128:], cu, None, H, H, 128, 128 ** -0.5, False, out=out128,
                         one_tile_max_seg=64)
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).cuda()
    with pytest.raises(_lib.VlmHipError, match="rc=2"):
        ops.attn_prefill(qkv, qkv[:, H * D:], qkv[:, (H + 1) * D:], cu, None, H, 1, D, SCALE, False, out=out, one_tile_max_seg=64)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out128 == 7.0).all())
