"""Rotary embedding and the paged KV write of every kernel that does them, exact on a lattice (tests/rope_exact.py).

The fused decode forms get inputs whose qkv product is exact in every summation order, so what is compared is the rotation,
the pair addressing and the pool layout alone - against the float64 rotation of the kernels' contract, at the bar "the correct
bf16 rounding of a value within fp32 evaluation error" (no bf16-ulp tolerance), positions up to 2^24 - 1, every geometry of
the model families, every row count the entry points accept, block-table and identity layouts, pools prefilled with a
sentinel so that a write to ANY wrong place shows.  A census in a child process reads the kernels' own debug lines and
asserts that the case table reached every form the shape policy can pick.  The prompt form (mrope_kvwrite_, with kv_gather_
reading the pools back) and the vision form (rope2d_vision_) are held the same way on lattice values written straight into
the qkv buffer."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import rope_exact as R

pytestmark = pytest.mark.gpu

BF, F64 = torch.bfloat16, torch.float64


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


# ------------------------------------------------------------------ the fused decode forms
@pytest.mark.parametrize("case", R.FUSED_CASES, ids=R.fused_id)
def test_fused_qkv_rotation_and_kv_write_are_exact(vops, case):
    for paged in (True, False):
        name = f"{R.fused_id(case)} {'paged' if paged else 'identity'} [{case['form']}]"
        R.check_fused(name, case, paged, *R.run_fused(vops, case, paged))


@pytest.mark.parametrize("case", R.REFUSED_CASES, ids=R.fused_id)
def test_fused_qkv_row_counts_no_kernel_takes_are_refused(vops, case):
    """no quiet fall-back: 3 or 5 rows, and 9 rows at K = 4096 without a workspace, are an error and enqueue nothing"""
    stray = R.run_fused(vops, case, True, refused=True)
    assert stray == 0


_CENSUS_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from mlx_vlm_amd import ops as vops
from tests import rope_exact as R
ws_only = sys.argv[3] == "ws"
out = {}
for idx, case in enumerate(R.FUSED_CASES):
    if ws_only and not R.ENTRIES[case["entry"]][1]:
        continue
    print(f"CASE {idx}", file=sys.stderr, flush=True)
    res = R.run_fused(vops, case, True)
    torch.cuda.synchronize()
    out[idx] = res
print("CASE end", file=sys.stderr, flush=True)
torch.save(out, sys.argv[2])
"""


def _debug_forms(stderr):
    """stderr of the child -> {case index: the LAST debug line of a rope launch printed during that case, or None}"""
    forms, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("CASE "):
            cur = line.split()[1]
            if cur != "end":
                forms[int(cur)] = None
        elif line.startswith("[gemv_mfma") and "epi=-1" in line and cur not in (None, "end"):
            forms[int(cur)] = line
    return forms


def _form_of_line(line):
    if line is None:
        return None
    tag = line.split("]")[0][1:]                        # gemv_mfma | gemv_mfma2
    w4 = " w4 " in line
    return (w4, "mfma2" if tag == "gemv_mfma2" else "mfma")


def test_form_census_every_form_is_reached_and_exact(vops, tmp_path):
    """The shape policy's choice is invisible to the caller, so the table could miss a form without anyone noticing.  The
    kernels print one line per matrix-core launch under VLM_GEMV_MFMA_DEBUG=1 (read once per process: a child runs the cases);
    a second child with VLM_GEMV_MFMA2=0 sends the workspace cases to the first form, the 4-bit one's only way there."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = set()
    for run, extra in (("all", {}), ("ws", {"VLM_GEMV_MFMA2": "0"})):
        path = str(tmp_path / f"census_{run}.pt")
        env = dict(os.environ, VLM_GEMV_MFMA_DEBUG="1", **extra)
        if not extra:
            env.pop("VLM_GEMV_MFMA2", None)
        r = subprocess.run([sys.executable, "-c", _CENSUS_CHILD, root, path, run], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        res = torch.load(path)
        forms = _debug_forms(r.stderr)
        assert forms.keys() == res.keys() and len(res) > 0
        for idx, saved in res.items():
            case = R.FUSED_CASES[idx]
            w4, ws, _ = R.ENTRIES[case["entry"]]
            want = R.form_of(w4, ws, case["M"], R.GEOMETRIES[case["gi"]][3], mfma2=not extra)
            got = _form_of_line(forms[idx])
            name = f"census[{run}] {R.fused_id(case)} [{want}]"
            if want == "dot2c":
                assert got is None, (name, forms[idx])              # no debug line: the v_dot2c kernels took the call
            else:
                assert got == (w4, want), (name, forms[idx])
            seen.add((w4, want))
            R.check_fused(name, case, True, *saved)
        if not extra:
            # every case of <= 8 rows went to the v_dot2c kernels
            assert all(forms[i] is None for i, c in enumerate(R.FUSED_CASES) if c["M"] <= 8)
    assert seen == {(False, "mfma"), (False, "mfma2"), (True, "mfma2"), (True, "mfma"), (False, "dot2c"), (True, "dot2c")}, seen


# ------------------------------------------------------------------ the prompt form
@pytest.mark.parametrize("scale", [None, R.QK_SCALE])
@pytest.mark.parametrize("sections", R.SECTIONS, ids=str)
@pytest.mark.parametrize("D", [128, 96, 64])
def test_mrope_kvwrite_prompt_form_is_exact_and_kv_gather_returns_the_pool(vops, D, sections, scale):
    T, Hq, Hkv = 150, 4, 2
    H = Hq + 2 * Hkv
    y = R.lattice_y(T, H, D, seed=500 + D)
    g = torch.Generator().manual_seed(501)
    pos3 = torch.randint(0, 2 ** 24, (3, T), generator=g)
    for a in range(3):                                               # the three axes are distinct
        pos3[a, :10] = torch.tensor(R.POSITIONS).roll(3 * a)
    pos3[:, 10] = 0                                                  # the identity row
    pos3[:, 11] = 2 ** 24 - 1
    inv = O.mrope_inv_freq(D, 1e6 if D == 128 else 1e4)
    # two sequences: tokens [0, 100) -> sequence 0, slots 28 .. 127; tokens [100, 150) -> sequence 1, slots 0 .. 49
    kv_seq = torch.cat([torch.zeros(100), torch.ones(50)]).to(torch.int32)
    kv_slot = torch.cat([torch.arange(100) + 28, torch.arange(50)]).to(torch.int32)
    n_pages = 8
    bt = torch.tensor([[3, 1, 0, 0], [6, 0, 0, 0]], dtype=torch.int32)
    pages = bt[kv_seq.long(), (kv_slot // 64).long()].long()
    within = (kv_slot % 64).long()
    kpool, vpool = R.pools_new(n_pages, Hkv, D, "cuda")
    qkv = y.to(BF).reshape(T, H * D).cuda()
    out = vops.mrope_kvwrite_(qkv, Hq, Hkv, D, pos3[0].int().cuda(), pos3[1].int().cuda(), pos3[2].int().cuda(), inv.cuda(),
                              sections[0], sections[1], kv_seq.cuda(), kv_slot.cuda(), bt.cuda(), kpool, vpool, qk_scale=scale)
    o = out.view(T, H, D).cpu()
    s = 1.0 if scale is None else scale
    ex, mag = R.exact_mrope(y[:, :Hq + Hkv], pos3, inv, sections, s)
    name = f"mrope_kvwrite_ D={D} {sections} scale={scale}"
    R.check_rot(name + " q, k", o[:, :Hq + Hkv], ex, mag)
    assert torch.equal(o[:, Hq + Hkv:].to(F64), y[:, Hq + Hkv:])                              # v columns untouched
    assert torch.equal(o[10, :Hq + Hkv].to(F64), R.rne_bf16(y[10, :Hq + Hkv] * s))            # position 0: the identity
    k_rows, v_rows, stray = R.pools_read(kpool, vpool, pages, within)
    assert R.check_pools(name, k_rows, v_rows, stray, ex[:, Hq:], mag[:, Hq:], y[:, Hq + Hkv:])[1] <= R.CAP
    assert torch.equal(k_rows, o[:, Hq:Hq + Hkv])                                             # the pool holds what the buffer holds
    # the fetch half: kv_gather_ returns the pooled rows bit for bit and touches no q column
    back = torch.full((T, H * D), R.SENTINEL, dtype=torch.int16, device="cuda").view(BF)
    vops.kv_gather_(back, Hq, Hkv, D, kv_slot.cuda(), bt.cuda(), kpool, vpool, kv_seq=kv_seq.cuda())
    b = back.view(T, H, D).cpu()
    assert torch.equal(b[:, Hq:Hq + Hkv], k_rows) and torch.equal(b[:, Hq + Hkv:], v_rows)
    assert bool((b[:, :Hq].contiguous().view(torch.int16) == R.SENTINEL).all())


# ------------------------------------------------------------------ the vision form
@pytest.mark.parametrize("N", [144, 132, 77])
@pytest.mark.parametrize("D", [80, 64])
def test_rope2d_vision_is_exact_on_the_table_it_is_given(vops, D, N):
    Hh = 4
    # 108 + 36 rows, 96 + 36 rows (no multiple of 8) and the first 77 of 80
    grid = np.array({144: [[1, 6, 18], [1, 6, 6]], 132: [[1, 8, 12], [1, 6, 6]], 77: [[1, 10, 8]]}[N])
    freqs = O.vision_rotary_freqs(grid, D)[:N].contiguous()
    assert freqs.shape == (N, D // 2)
    cos, sin = torch.cos(freqs), torch.sin(freqs)
    y = R.lattice_y(N, 3 * Hh, D, seed=600 + D + N)
    out = vops.rope2d_vision_(y.to(BF).reshape(N, 3 * Hh * D).cuda(), cos.cuda(), sin.cuda(), Hh).view(N, 3 * Hh, D).cpu()
    ex, mag = R.rotate_table(y[:, :2 * Hh], cos, sin)
    R.check_rot(f"rope2d_vision_ D={D} N={N}", out[:, :2 * Hh], ex, mag)
    assert torch.equal(out[:, 2 * Hh:].to(F64), y[:, 2 * Hh:])                                  # v untouched
