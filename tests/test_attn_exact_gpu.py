"""Every attention kernel form against the exactly rounded result (tests/attn_exact.py), at the shapes the model sweeps
never reached: each G = Hq / Hkv template instance 1..8 of every decode entry point, both KV layouts, contexts on both sides
of a page edge up to 4100 tokens (unwritten pool slots NaN), the 8-bit kernel's 64-key and half-page forms, prefill at
G = 1 / 4 / 6 / 7 / 8 with segments straddling the 64-key tile and the 128-row query block, q_start at the new G values,
and the padded heads of SigLIP (72 in 80), Phi-3.5 (96 in 128) and nanoLLaVA (64 in 128).  The float64 references run on
the device (torch float64), the bars are the classes of attn_exact.BARS."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attn_exact as A

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def vops():
    from mlx_vlm_amd import ops

    return ops


def _rows(B):
    return [(b, b + 1) for b in range(B)]


def _decode_forms(vops, name, q, ks, vs, exact, scale, identity, seed, Hq, Hkv, wo_forms=True):
    """every bf16 decode entry point over the same pools -> A.check each ("hilo")"""
    B, D = q.shape[0], 128
    bt, kpool, vpool, mp = A.build_pools(ks, vs, seed=seed, identity=identity)
    qd, kd, vd = q.cuda(), kpool.cuda(), vpool.cuda()
    btd = None if identity else bt.cuda()
    lens = [k.shape[0] for k in ks]
    kv_len = torch.tensor(lens, dtype=torch.int32).cuda()
    segs = _rows(B)
    lay = "identity" if identity else "block table"
    # vlm_attn_decode_paged: nsplit = 1 -> one workgroup per (row, kv head) writes bf16; nsplit = 4 -> partials + combine
    for ns in (1, 4):
        out = vops.attn_decode_paged(qd, kd, vd, btd, kv_len, 0, Hq, Hkv, D, scale, ns, max_pages=mp)
        A.check(f"{name} paged nsplit {ns}, {lay}", out, exact, "hilo", segs)
    # vlm_attn_decode_paged_split, merging: the last arriving workgroup merges (16 splits: splits without a page too)
    out = vops.attn_decode_paged_split(qd, kd, vd, btd, kv_len, 0, Hq, Hkv, D, scale, 16, max_pages=mp)
    A.check(f"{name} page-split merge x16, {lay}", out, exact, "hilo", segs)
    if not wo_forms:
        return
    # partial-only + the o_proj prologue merge (one decode row per launch): Wo = I and a random Wo
    K = Hq * D
    eye = torch.eye(K, dtype=BF, device=DEV)
    wo = A.rnd(K, K, seed=seed + 7, scale=0.03)
    got_eye, got_wo = [], []
    for b in range(B):
        kb, vb = (kd[b * mp:(b + 1) * mp], vd[b * mp:(b + 1) * mp]) if identity else (kd, vd)
        po, pml = vops.attn_decode_paged_split(qd[b:b + 1], kb, vb, None if identity else btd[b:b + 1], kv_len[b:b + 1], 0, Hq,
                                               Hkv, D, scale, 16, max_pages=mp, merge=False)
        got_eye.append(vops.gemv_attn_out_bf16_(po, pml, eye, torch.zeros(1, K, dtype=BF, device=DEV), Hq, D))
        got_wo.append(vops.gemv_attn_out_bf16_(po, pml, wo.cuda(), torch.zeros(1, K, dtype=BF, device=DEV), Hq, D))
    att = torch.cat(got_eye)
    A.check(f"{name} partials + o_proj prologue (Wo = I), {lay}", att, exact, "hilo", segs)
    # the GEMV behind the merge, against the exact product of the bf16 attention the prologue fed it (the Wo = I output):
    # against oproj_exact(exact) every near-tie the attention rounds the other way (legitimately, within 1 ulp) would move
    # all K outputs at once - 1e-4 .. 6e-4 of noise that says nothing about the GEMV
    A.check(f"{name} partials + o_proj prologue (random Wo), {lay}", torch.cat(got_wo), A.oproj_exact(att, wo, dev=DEV), "hilo", segs)


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("case", A.DECODE_CASES, ids=A.case_id)
def test_decode_every_form_and_g_instance_exact(vops, case, identity):
    Hq, Hkv = case["Hq"], case["Hkv"]
    q, ks, vs = A.decode_inputs(case["lens"], Hq, Hkv, seed=2000 + case["G"])
    exact = A.decode_exact(q, ks, vs, 128 ** -0.5, dev=DEV)
    _decode_forms(vops, f"decode G={case['G']}", q, ks, vs, exact, 128 ** -0.5, identity, 2100 + case["G"], Hq, Hkv)


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("case", A.PAD_DECODE_CASES, ids=A.case_id)
def test_decode_padded_heads_exact(vops, case, identity):
    """a 96- / 64-wide head inside the D = 128 decode kernels: zero pad columns, scale real ** -0.5, pad outputs exactly 0"""
    Hq, Hkv, real = case["Hq"], case["Hkv"], case["real"]
    q, ks, vs = A.decode_inputs(case["lens"], Hq, Hkv, seed=2200 + real, real=real)
    exact = A.decode_exact(q, ks, vs, real ** -0.5, real=real, dev=DEV)
    _decode_forms(vops, f"decode head {real} in 128", q, ks, vs, exact, real ** -0.5, identity, 2300 + real, Hq, Hkv, wo_forms=False)
    bt, kpool, vpool, mp = A.build_pools(ks, vs, seed=2300 + real, identity=identity)
    kv_len = torch.tensor(case["lens"], dtype=torch.int32).cuda()
    btd = None if identity else bt.cuda()
    for ns in (1, 4):
        out = vops.attn_decode_paged(q.cuda(), kpool.cuda(), vpool.cuda(), btd, kv_len, 0, Hq, Hkv, 128, real ** -0.5, ns, max_pages=mp)
        assert bool((out.view(-1, Hq, 128)[..., real:] == 0).all())
    out = vops.attn_decode_paged_split(q.cuda(), kpool.cuda(), vpool.cuda(), btd, kv_len, 0, Hq, Hkv, 128, real ** -0.5, 16, max_pages=mp)
    assert bool((out.view(-1, Hq, 128)[..., real:] == 0).all())


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("case", A.Q8_CASES, ids=A.case_id)
def test_decode_q8_every_g_instance_and_form_exact(vops, case, identity):
    """vlm_attn_decode_paged_q8, the new token quantised by the launch.  case["form"] names the form the dispatch takes:
    B * Hkv >= 128 with nsplit <= 16 -> half-page units (2 * nsplit splits of 32 keys), otherwise 64-key pages"""
    Hq, Hkv, lens, ns = case["Hq"], case["Hkv"], case["lens"], case["nsplit"]
    assert (len(lens) * Hkv >= 128 and ns <= 16) == (case["form"] == "half-page")
    q, ks, vs = A.decode_inputs(lens, Hq, Hkv, seed=2400 + case["G"], kscale=0.8, outlier=True)
    exact = A.decode_q8_exact(q, ks, vs, 128 ** -0.5, dev=DEV)
    bt, kpool, vpool, mp = A.build_pools(ks, vs, seed=2500 + case["G"], identity=identity)
    kd, vd = kpool.cuda(), vpool.cuda()
    n = kpool.numel()
    k8 = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    v8 = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    ksb = torch.full((n // 64,), 0x7fc07fc0, dtype=torch.int32, device=DEV)      # unwritten (scale | bias) words: NaN | NaN
    vsb = torch.full((n // 64,), 0x7fc07fc0, dtype=torch.int32, device=DEV)
    btd = bt.cuda()
    seq = torch.cat([torch.full((m - 1,), b, dtype=torch.int32) for b, m in enumerate(lens)])
    slot = torch.cat([torch.arange(m - 1, dtype=torch.int32) for m in lens])
    if seq.numel():
        vops.kv_quantize_tokens(kd, vd, k8, v8, ksb, vsb, seq.cuda(), slot.cuda(), btd, Hkv, 128)
    kv_len = torch.tensor(lens, dtype=torch.int32).cuda()
    out = vops.attn_decode_paged_q8(q.cuda(), kd, vd, k8, v8, ksb, vsb, None if identity else btd, kv_len, 0, Hq, Hkv, 128,
                                    128 ** -0.5, ns, quantize_new=True, max_pages=mp)
    A.check(f"q8 decode G={case['G']} {len(lens)}x{Hkv} {case['form']}, {'identity' if identity else 'block table'}", out,
            exact, "q8", _rows(len(lens)))


def _prefill_run(vops, case, seed, starts=None):
    D, Hq, Hkv, lens, causal, real = case["D"], case["Hq"], case["Hkv"], case["lens"], case["causal"], case.get("real")
    scale = (real or D) ** -0.5
    q, k, v = A.prefill_inputs(lens, Hq, Hkv, D, seed=seed, real=real)
    T = sum(lens)
    exact = A.prefill_exact(q, k, v, lens, scale, causal, starts=starts, real=real, dev=DEV)
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).cuda()
    off = np.concatenate([[0], np.cumsum(lens)])
    cu = torch.tensor(off, dtype=torch.int32).cuda()
    st = starts or [0] * len(lens)
    nqb = sum((n - s0 + 127) // 128 for n, s0 in zip(lens, st))
    is_q, segs = A.query_rows(lens, starts)
    out = torch.full((T, Hq * D), 7.0, dtype=BF, device=DEV)
    vops.attn_prefill(qkv, qkv[:, Hq * D:], qkv[:, (Hq + Hkv) * D:], cu, nqb, Hq, Hkv, D, scale, causal, out=out,
                      q_start=None if starts is None else torch.tensor(starts, dtype=torch.int32).cuda())
    o = out.cpu().view(T, Hq, D)
    if starts is not None:
        assert bool((o[~is_q].float() == 7.0).all())                  # the keys-only prefix rows are not written
    return o[is_q], exact[is_q], segs


@pytest.mark.parametrize("case", A.PREFILL_CASES, ids=A.case_id)
def test_prefill_every_g_and_tile_edge_exact(vops, case):
    got, want, segs = _prefill_run(vops, case, seed=2600 + case["D"] + case["G"])
    A.check(f"prefill D={case['D']} causal={case['causal']} G={case['G']} lens={case['lens']}", got, want,
            A.prefill_class(case["D"]), segs)


@pytest.mark.parametrize("case", A.QSTART_CASES, ids=A.case_id)
def test_prefill_q_start_exact(vops, case):
    got, want, segs = _prefill_run(vops, case, seed=2700 + case["D"] + case["G"], starts=case["starts"])
    A.check(f"prefill q_start D={case['D']} G={case['G']} starts={case['starts']}", got, want, A.prefill_class(case["D"]), segs)


@pytest.mark.parametrize("case", A.PAD_PREFILL_CASES, ids=A.case_id)
def test_prefill_padded_heads_exact(vops, case):
    got, want, segs = _prefill_run(vops, case, seed=2800 + case["real"])
    A.check(f"prefill head {case['real']} in {case['D']} causal={case['causal']}", got, want, A.prefill_class(case["D"]), segs)
    assert bool((got[..., case["real"]:] == 0).all())


_HILO_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from mlx_vlm_amd import ops as vops
from tests import attn_exact as A
D, causal, lens, Hq, Hkv = int(sys.argv[3]), sys.argv[4] == "1", [300, 64, 129, 1], 6, 1
T = sum(lens)
q, k, v = A.prefill_inputs(lens, Hq, Hkv, D, seed=2900 + D)
qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).cuda()
cu = torch.tensor([0, 300, 364, 493, 494], dtype=torch.int32).cuda()
out = vops.attn_prefill(qkv, qkv[:, Hq * D:], qkv[:, (Hq + Hkv) * D:], cu, 3 + 1 + 2 + 1, Hq, Hkv, D, D ** -0.5, causal)
torch.save(dict(out=out.cpu().view(T, Hq, D), exact=A.prefill_exact(q, k, v, lens, D ** -0.5, causal)), sys.argv[2])
"""


def test_prefill_p_operand_knob_moves_a_case_across_the_class_bars(vops, tmp_path):
    """the bars tell the two P forms apart on hardware: VLM_ATTN_PREFILL_HILO=0 puts the D = 128 kernel on one bf16 P
    operand (it must fail the hi + lo class and pass the single-P class); VLM_ATTN_PREFILL_HILO=1 puts the D = 80 kernel on
    hi + lo (it must pass the hi + lo class).  The knob is read once per process: each form runs in a child process, and
    no child starts after one has failed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for knob, D, causal in (("0", 128, "1"), ("1", 80, "0")):
        path = str(tmp_path / f"hilo{knob}.pt")
        env = dict(os.environ, VLM_ATTN_PREFILL_HILO=knob)
        r = subprocess.run([sys.executable, "-c", _HILO_CHILD, root, path, str(D), causal], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[knob] = torch.load(path)
    _, segs = A.query_rows([300, 64, 129, 1])
    ok, _, _, rep = A.measure(res["0"]["out"], res["0"]["exact"], "hilo", segs)
    print("ATTN-EXACT D=128 causal prefill, HILO=0, hi + lo class:", rep)
    assert not ok, rep
    A.check("D=128 causal prefill, VLM_ATTN_PREFILL_HILO=0 (one bf16 P)", res["0"]["out"], res["0"]["exact"], "single", segs)
    A.check("D=80 prefill, VLM_ATTN_PREFILL_HILO=1 (hi + lo P)", res["1"]["out"], res["1"]["exact"], "hilo", segs)
