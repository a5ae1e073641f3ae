"""VLM_DECODE_HOST_RING (include/vlm_hip.h): the step's tail stores its token into a pinned ring with a system-scope store
and generate_step reads slot step % ring_len behind the step's event - no device-to-host copy between two replays.  Where a
token travels changes nothing it is: with the host ring on and off, generate_step on the tiny Qwen2-VL yields equal tokens
and `torch.equal` log-probs, through each of the three tails (fused greedy, fused sampled, and the plain advance that steps
with logits processors take), under a window (max_kv_size), at lookahead 1 and 8; and over 300 steps - the ring wraps four
times with 8 steps in flight - every token read from the ring is the one the step left on the device.

The model carries the peaked head of tests/test_parity_decode_gpu.py: its greedy stream steps through a permutation, no
token repeats within 1000 steps, so a slot read too early or too late cannot hold the right token by accident."""
import numpy as np
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def tiny():
    cfg = oq.tiny_cfg()
    cfg.text.tie_word_embeddings = False
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * 0.5).to(BF)
    W = oq.peak_head(W, cfg, gamma=4.0, stride=389, n_cycle=1000)
    return build_product_model(cfg, W, kv_pool_tokens=4096, max_seqs=4)


def _ids(seed=21, n=40):
    return np.random.default_rng(seed).integers(3, 1000, (1, n))


def _run(model, host_ring, n=70, **kw):
    from mlx_vlm_amd.generate import generate_step

    out = [(t, lp.float().cpu()) for t, lp in generate_step(_ids(), model, None, None, max_tokens=n, host_ring=host_ring, **kw)]
    assert len(out) == n
    return [t for t, _ in out], torch.stack([lp for _, lp in out])


def _same(model, **kw):
    toks0, lps0 = _run(model, False, **kw)
    toks1, lps1 = _run(model, True, **kw)
    assert toks1 == toks0, kw
    assert torch.equal(lps1, lps0), kw
    return toks0


@pytest.mark.parametrize("lookahead", [1, 8])
@pytest.mark.parametrize("sampler", [dict(temperature=0.0), dict(temperature=0.8, top_p=0.9, seed=7)], ids=["greedy", "sampled"])
def test_host_ring_yields_the_copy_paths_tokens_and_logprobs(tiny, sampler, lookahead):
    toks = _same(tiny, lookahead=lookahead, **sampler)
    if sampler["temperature"] == 0:
        assert len(set(toks)) == len(toks)


def test_host_ring_under_a_window(tiny):
    _same(tiny, lookahead=8, temperature=0.0, max_kv_size=24)


def test_host_ring_with_a_logits_processor_penalty(tiny):
    _same(tiny, lookahead=8, temperature=0.0, repetition_penalty=1.3, repetition_context_size=20)
    _same(tiny, lookahead=8, temperature=0.8, seed=3, repetition_penalty=1.3, repetition_context_size=20)


def test_host_ring_unfused_tail(tiny):
    """vlm_decode_advance_win, the tail of a step without the fused sampler launches"""
    lm = tiny.language_model
    lm.apply_tuning(fused_tail=0)
    try:
        _same(tiny, lookahead=8, temperature=0.0)
    finally:
        lm.apply_tuning()


def test_300_steps_read_from_the_ring_are_the_devices_tokens(tiny, monkeypatch):
    from mlx_vlm_amd.generate import generate_step

    lm = tiny.language_model
    n = 300
    hist = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    issued = [0]
    run = lm.decode_run

    def recording_run(st, n_steps, *a, **kw):
        assert kw.get("host_ring") is True and n_steps == 1
        run(st, n_steps, *a, **kw)
        hist[issued[0]:issued[0] + 1].copy_(st.tok)        # device to device, in stream order behind the step
        issued[0] += 1

    monkeypatch.setattr(lm, "decode_run", recording_run)
    toks = [t for t, _ in generate_step(_ids(), tiny, None, None, max_tokens=n, temperature=0.0, lookahead=8,
                                        return_logprobs=False, host_ring=True)]
    assert issued[0] == n - 1 and len(toks) == n
    assert toks[1:] == hist[:n - 1].cpu().tolist()          # (token 0 comes from the prefill's own sampler call)
    assert len(set(toks)) == n
