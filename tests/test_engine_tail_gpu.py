"""The switches of the one-row step's entry and tail, all on against all off, through generate_step on the tiny Qwen2-VL:

    bit 6 of VLM_TUNE_GEMV_VARIANT     the qkv launch that waits for no scalar load ahead of its weights
    bit 13                             lse partials in one pass over memory
    bit 14                             the tail's logits loads ahead of its partials, one ticket level for one row
    skip_logprobs                      a return_logprobs=False generation hands the tail no log-prob pointer
    host_ring                          tokens through the pinned ring, no copy kernel between two replays

None of them changes what a step computes: 40 greedy tokens at lookahead 8 are equal, with return_logprobs False and True,
and the log-probs are `torch.equal` where they were asked for.  A generation that does not ask for them leaves the decode
state's log-prob row alone when the switch is on (a canary stays) and overwrites it when it is off - the switch is what
decides.  The model carries the peaked head of tests/test_parity_decode_gpu.py: no token repeats, so a step that read a
stale row, slot or token cannot give the right stream by accident."""
import numpy as np
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BITS = 64 | 1 << 13 | 1 << 14
N_TOK = 40


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


def _run(model, on, return_logprobs):
    from mlx_vlm_amd.generate import generate_step

    lm = model.language_model
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~BITS
    lm.apply_tuning(gemv_variant=base | (BITS if on else 0), skip_logprobs=int(on))
    ids = np.random.default_rng(21).integers(3, 1000, (1, 40))
    lm.decode_state(1).logprobs.fill_(-7.0)                      # canary
    out = list(generate_step(ids, model, None, None, max_tokens=N_TOK, temperature=0.0, lookahead=8, host_ring=on,
                             return_logprobs=return_logprobs))
    torch.cuda.synchronize()
    assert len(out) == N_TOK
    toks = [t for t, _ in out]
    lps = torch.stack([lp.float().cpu() for _, lp in out]) if return_logprobs else None
    assert return_logprobs or all(lp is None for _, lp in out)
    canary_left = bool((lm.decode_state(1).logprobs == -7.0).all())
    return toks, lps, canary_left


@pytest.fixture(scope="module")
def streams(tiny):
    """(tokens, log-probs, canary left) of the four runs, made once"""
    lm = tiny.language_model
    try:
        return {(on, rl): _run(tiny, on, rl) for on in (False, True) for rl in (False, True)}
    finally:
        lm.apply_tuning()


def test_all_switches_on_give_the_tokens_of_all_off(streams):
    ref = streams[(False, True)][0]
    assert len(set(ref)) == N_TOK
    for key, (toks, _, _) in streams.items():
        assert toks == ref, key


def test_logprobs_are_equal_where_they_were_asked_for(streams):
    off, on = streams[(False, True)][1], streams[(True, True)][1]
    assert bool(torch.isfinite(off).any())
    assert torch.equal(on, off)
    # the row of a token is that token's: its argmax is the token
    assert off.argmax(-1).tolist() == streams[(False, True)][0]


def test_a_generation_without_logprobs_leaves_the_row_alone_only_under_the_switch(streams):
    assert streams[(True, False)][2] is True
    assert streams[(False, False)][2] is False
    assert streams[(True, True)][2] is False and streams[(False, True)][2] is False
