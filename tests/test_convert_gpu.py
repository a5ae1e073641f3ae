"""convert() on the device: the 4-bit quantizer (the quantise direction of vlm_dequant_w4) against mx.quantize restated
(oracle/quant.py::quantize_affine) - BIT-EXACT, no tolerance and no excluded element: the oracle is defined and deterministic
on every input used here (the scale is clamped at 1e-7, so there is no 0 / 0) - and the checkpoints convert() writes."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import quant as Q
from oracle import qwen2_vl as oq
from tests.convert_helpers import assert_same_tensors, read_tensors, write_tiny_checkpoint
from tests.helpers import synth_request

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SHAPES = [(1, 64), (3, 192), (7, 1536), (65, 128), (130, 8960)]


def _fused_sb(scales, biases):
    """the bf16 bits of scales / biases fused as models/quantized.py::take fuses them (int32 bit patterns)"""
    from mlx_vlm_amd.models import quantized as Qz

    return Qz._bf16_bits(scales).to(torch.int64) | (Qz._bf16_bits(biases).to(torch.int64) << 16)


def _check_bit_exact(w_dev):
    """ops.quantize_w4 on a device matrix (any row stride) == the oracle on the same values"""
    from mlx_vlm_amd import ops

    wq, sb = ops.quantize_w4(w_dev)
    torch.cuda.synchronize()
    ref_wq, ref_s, ref_b = Q.quantize_affine(w_dev.cpu().contiguous(), 64, 4)
    N, K = w_dev.shape
    assert wq.dtype == torch.int32 and sb.dtype == torch.int32 and wq.shape == (N, K // 8) and sb.shape == (N, K // 64)
    assert torch.equal(wq.cpu(), ref_wq)
    assert torch.equal(sb.cpu().to(torch.int64) & 0xFFFFFFFF, _fused_sb(ref_s, ref_b))
    return wq, sb, (ref_wq, ref_s, ref_b)


def _hand_built() -> torch.Tensor:
    """[8, 192] bf16: 24 groups, each one of the corner cases of the rule (every value is exact in bf16)"""
    g = torch.Generator().manual_seed(11)
    noise = lambda s: (torch.randn(64, generator=g) * s).to(BF).float()
    groups = []
    groups.append(torch.zeros(64))                                            # all zeros: scale = the 1e-7 clamp, q0 = 0
    groups.append(torch.full((64,), 0.37))                                    # constant != 0: w_max == w_min
    groups.append(torch.full((64,), -2.5))                                    # constant < 0
    x = noise(1.0).clamp(-8, 3); x[5], x[40] = -8.0, 3.0                      # |w_min| > |w_max|
    groups.append(x)
    x = noise(1.0).clamp(-3, 8); x[63], x[0] = 8.0, -3.0                      # |w_min| < |w_max|
    groups.append(x)
    x = noise(1.5).clamp(-4, 4); x[17], x[18] = -4.0, 4.0                     # |w_min| == |w_max|: the mask tie
    groups.append(x)
    x = noise(0.01); x[33] = 10.0                                             # one outlier 1000 x the rest
    groups.append(x)
    x = noise(0.01); x[2] = -10.0
    groups.append(x)
    # rint ties: min 0, max 30 -> scale -2, bias 30; the odd integers are bias + (n + 0.5) * scale
    x = torch.tensor([0.0, 30.0] + [float(2 * (i % 15) + 1) for i in range(62)])
    groups.append(x)
    groups.append(-x)                                                         # the mirrored group: edge = w_min
    x = torch.tensor([0.0, 15.0] + [(i % 15) + 0.5 for i in range(62)])       # scale -1: ties at every half
    groups.append(x)
    x = torch.zeros(64); x[::2] = -0.0                                        # -0.0 and +0.0 only
    groups.append(x)
    x = noise(0.05); x[7], x[8] = -0.0, 0.0                                   # -0.0 among ordinary values
    groups.append(x)
    x = noise(0.05).abs(); x[9] = -0.0                                        # -0.0 is the minimum
    groups.append(x)
    x = -noise(0.05).abs(); x[9] = -0.0                                       # -0.0 is the maximum
    groups.append(x)
    x = torch.zeros(64); x[11] = 2.0 ** -120                                  # a range far below the clamp
    groups.append(x)
    x = noise(1.0) * 1e30                                                     # near the top of the bf16 range
    groups.append(x)
    x = torch.zeros(64); x[0] = 1.0                                           # one nonzero element
    groups.append(x)
    while len(groups) < 24:
        groups.append(noise(0.05 * len(groups)))
    return torch.stack(groups).to(BF).reshape(8, 192)


@pytest.mark.parametrize("std", [0.05, 30.0])
@pytest.mark.parametrize("N,K", SHAPES)
def test_quantize_w4_bit_exact_normal_data(N, K, std):
    g = torch.Generator().manual_seed(1000 * N + K + int(std))
    w = (torch.randn(N, K, generator=g) * std).to(BF)
    _check_bit_exact(w.cuda())


@pytest.mark.parametrize("N,K", SHAPES)
def test_quantize_w4_bit_exact_strided_source(N, K):
    """ld > K: a column slice of a wider tensor (16-byte aligned: read in place) and one at an odd column (copied first)"""
    g = torch.Generator().manual_seed(N + K)
    wide = (torch.randn(N, K + 72, generator=g) * 0.05).to(BF).cuda()
    _check_bit_exact(wide[:, :K])
    _check_bit_exact(wide[:, 64:64 + K])
    _check_bit_exact(wide[:, 3:3 + K])


def test_quantize_w4_bit_exact_hand_built_groups():
    w = _hand_built()
    assert torch.isfinite(w.float()).all() and bool((w.view(torch.int16) == -32768).any())      # -0.0 survived the packing
    wq, sb, (ref_wq, ref_s, ref_b) = _check_bit_exact(w.cuda())
    s = ref_s.float().reshape(-1)
    assert s[0].abs() == torch.tensor(1e-7).to(BF).float() and ref_b.float().reshape(-1)[0] == 0      # the clamp, q0 == 0
    # the tie groups do hold exact .5 quotients (the construction is not vacuous)
    g8 = w.float().reshape(-1, 64)[8]
    assert bool((((g8 - 30.0) / -2.0) % 1 == 0.5).sum() == 62)
    # and as single rows of every width, so that each group also meets each position of a wave
    _check_bit_exact(w.reshape(1, -1).cuda())
    _check_bit_exact(w.reshape(24, 64).cuda())


def test_quantize_w4_checks_its_input():
    from mlx_vlm_amd import ops

    for bad in (torch.zeros(4, 64), torch.zeros(64, dtype=BF), torch.zeros(2, 4, 64, dtype=BF), torch.zeros(4, 96, dtype=BF),
                torch.zeros(4, 0, dtype=BF)):
        with pytest.raises(ValueError):
            ops.quantize_w4(bad.cuda())


@pytest.mark.parametrize("N,K,std", [(3, 192, 0.05), (65, 128, 30.0), (7, 1536, 0.05)])
def test_quantize_dequantize_round_trip_bit_exact(N, K, std):
    from mlx_vlm_amd import ops

    g = torch.Generator().manual_seed(N * K)
    w = (torch.randn(N, K, generator=g) * std).to(BF)
    back = ops.dequant_w4(*ops.quantize_w4(w.cuda())).cpu()
    ref = Q.dequantize(*Q.quantize_affine(w, 64, 4))
    assert ref.dtype == BF and torch.equal(back.view(torch.int16), ref.view(torch.int16))
    hb = _hand_built()
    assert torch.equal(ops.dequant_w4(*ops.quantize_w4(hb.cuda())).cpu().view(torch.int16),
                       Q.dequantize(*Q.quantize_affine(hb, 64, 4)).view(torch.int16))


# ------------------------------------------------------------------------------------------------ convert()
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """cfg, bf16 weights, their oracle quantization (language model only - the tower is a multimodal module), the HF-layout
    source directory and the directory `convert(quantize=True)` made of it.  Written once, read by every test below."""
    from mlx_vlm_amd import convert

    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=4321, dtype=BF, std=0.05, embed_std=0.2)
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    base = tmp_path_factory.mktemp("convert")
    src, q_dir = str(base / "hf"), str(base / "mlx_q4")
    write_tiny_checkpoint(src, cfg, W)
    convert(src, q_dir, quantize=True)
    return dict(cfg=cfg, W=W, ck=ck, ow=ow, src=src, q_dir=q_dir, base=base)


def _greedy(model, cfg, n_new=12):
    from mlx_vlm_amd.generate import generate_step

    ids, pix, thw = synth_request(cfg, [(56, 56)], n_text=11, seed=46)
    toks, lps = [], []
    for t, lp in generate_step(ids, model, torch.from_numpy(pix), None, max_tokens=n_new, temperature=0.0, image_grid_thw=thw):
        toks.append(int(t))
        lps.append(lp.detach().cpu().clone())
    return toks, torch.stack(lps)


def _prefill_logits(model, cfg):
    ids, pix, thw = synth_request(cfg, [(56, 56)], n_text=11)
    lm = model.language_model
    f = model.get_input_embeddings(ids, torch.from_numpy(pix), image_grid_thw=thw)
    return lm(ids, f.inputs_embeds, cache=lm.make_cache(), position_ids=f.position_ids).logits.detach().cpu().clone()


def test_convert_quantize_equals_the_oracle_checkpoint_and_generates_the_same(tiny, tmp_path):
    from mlx_vlm_amd import load

    got = read_tensors(tiny["q_dir"])
    assert_same_tensors(got, tiny["ck"])
    scaled = sorted(k[:-len(".scales")] for k in got if k.endswith(".scales"))
    want = sorted(k[:-len(".weight")] for k, v in tiny["W"].items() if k.startswith("language_model.") and k.endswith(".weight")
                  and v.dim() == 2)
    assert scaled == want and len(scaled) > 8
    for k, v in tiny["W"].items():
        if k.startswith("vision_tower."):
            assert got[k].dtype == BF and torch.equal(got[k].view(torch.int16), v.view(torch.int16)), k
    conf = json.load(open(os.path.join(tiny["q_dir"], "config.json")))
    q = {"group_size": 64, "bits": 4, "mode": "affine"}
    assert conf["quantization"] == q and conf["quantization_config"] == q
    assert "torch_dtype" not in conf and "_name_or_path" not in conf and list(conf) == sorted(conf)
    model, _ = load(tiny["q_dir"], kv_pool_tokens=4096, max_seqs=4)
    assert model.language_model.quantized
    toks, lps = _greedy(model, tiny["cfg"])
    del model
    # the same tensors written from the oracle's own quantized dict (the flow of test_quantized_4bit_checkpoint_load_and_generate)
    ref_dir = str(tmp_path / "oracle_q4")
    write_tiny_checkpoint(ref_dir, tiny["cfg"], tiny["ck"], config_extra={"quantization": {"group_size": 64, "bits": 4}})
    ref_model, _ = load(ref_dir, kv_pool_tokens=4096, max_seqs=4)
    assert ref_model.language_model.quantized
    ref_toks, ref_lps = _greedy(ref_model, tiny["cfg"])
    assert len(toks) == 12 and toks == ref_toks
    assert lps.dtype == ref_lps.dtype and lps.shape == ref_lps.shape
    assert torch.equal(lps.view(torch.int16 if lps.element_size() == 2 else torch.int32),
                       ref_lps.view(torch.int16 if lps.element_size() == 2 else torch.int32))


def test_convert_without_quantize_loads_with_identical_prefill_logits(tiny, tmp_path):
    from mlx_vlm_amd import convert, load

    out = str(tmp_path / "mlx_bf16")
    convert(tiny["src"], out)
    assert_same_tensors(read_tensors(out), tiny["W"])
    a, _ = load(out, kv_pool_tokens=4096, max_seqs=4)
    assert not a.language_model.quantized
    la = _prefill_logits(a, tiny["cfg"])
    del a
    b, _ = load(tiny["src"], kv_pool_tokens=4096, max_seqs=4)
    lb = _prefill_logits(b, tiny["cfg"])
    assert la.shape == lb.shape and la.dtype == lb.dtype and la.shape[-1] == tiny["cfg"].text.vocab_size
    assert torch.equal(la.view(torch.int16 if la.element_size() == 2 else torch.int32),
                       lb.view(torch.int16 if lb.element_size() == 2 else torch.int32))


def test_convert_dequantize(tiny, tmp_path):
    from mlx_vlm_amd import convert, ops
    from mlx_vlm_amd.models import quantized as Qz

    out = str(tmp_path / "mlx_deq")
    convert(tiny["q_dir"], out, dequantize=True)
    got, src = read_tensors(out), read_tensors(tiny["q_dir"])
    assert not [k for k in got if k.endswith((".scales", ".biases"))]
    assert sorted(got) == sorted(tiny["W"])
    paths = [k[:-len(".scales")] for k in src if k.endswith(".scales")]
    assert len(paths) > 8
    for p in paths:
        q = Qz.take(src, p).to("cuda")
        want = ops.dequant_w4(q.wq, q.sb).cpu()
        assert got[p + ".weight"].dtype == BF and torch.equal(got[p + ".weight"].view(torch.int16), want.view(torch.int16)), p
    for k, v in src.items():                                   # everything else is carried over as it was
        if k.rsplit(".", 1)[0] not in paths:
            assert torch.equal(got[k].view(torch.int16), v.view(torch.int16)), k
    conf = json.load(open(os.path.join(out, "config.json")))
    assert "quantization" not in conf and "quantization_config" not in conf
    with pytest.raises(ValueError):
        convert(tiny["q_dir"], str(tmp_path / "never"), quantize=True)        # already quantized
    assert not os.path.exists(str(tmp_path / "never"))


def test_convert_cli_in_a_fresh_process(tiny, tmp_path):
    out = str(tmp_path / "cli_q4")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "mlx_vlm_amd.convert", "--hf-path", tiny["src"], "--mlx-path", out, "-q"],
                       timeout=120, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert_same_tensors(read_tensors(out), read_tensors(tiny["q_dir"]))
    assert json.load(open(os.path.join(out, "config.json"))) == json.load(open(os.path.join(tiny["q_dir"], "config.json")))
