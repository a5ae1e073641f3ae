"""Prompt chunks onto a cache that is ALREADY 8-bit (kv_bits = 8), through the model and the user-level entry points: the
reference's QuantizedKVCache takes an update of any length (cache.py:233-334) and quantized_scaled_dot_product_attention runs
under the offset causal mask at L > 1 (base.py:260-302,305-373); here LanguageModel._prefill_onto_cache quantises the chunk's
tokens layer by layer and attends over the 8-bit pools (vlm_attn_prefill_paged_q8).

  * module call: every row of a 9 / 70 / 200-token chunk against the oracle that quantises after the first forward, and
    closer to it than to the bf16-cache oracle (the two oracles differ by ~1e-2 per row, below the 2e-2 bar: only the second
    condition shows that the 8-bit pools were read); then teacher-forced decode steps on the same cache;
  * stream_generate(prompt_cache_state=, kv_bits=8) over three turns (the third trims the 8-bit cache),
    generate_step(prompt_cache=an 8-bit cache) in one chunk and in chunks of 32, and the refused mix of 8-bit and bf16
    sequences.
Tiny config and weights as tests/test_kv_quant_gpu.py's `tiny` fixture; its model-level bar (rel-rms < 2e-2 per row)."""
import numpy as np
import pytest
import torch

from oracle import quant
from oracle import qwen2_vl as oq
from tests.helpers import build_product_model, synth_request
from tests.test_engine_gpu import _tie_aware_equal

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROW_BAR = 2e-2           # tests/test_kv_quant_gpu.py: every row within 2e-2 rel-rms of the oracle of the same policy


def _rel_rms(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


@pytest.fixture(scope="module")
def tiny():
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    return cfg, W, build_product_model(cfg, W, kv_pool_tokens=8192, max_seqs=24)


def _pid(start, n):
    return (start + torch.arange(n)).view(1, 1, n).expand(3, 1, n).contiguous()


def _oracle_feed(W, cfg, cache, tokens, start_pos):
    """tokens [n] onto `cache` at rope positions start_pos .. -> logits [n, V]"""
    h = oq.qwen2_model(W, cfg, oq.embed_tokens(W, np.asarray(tokens)[None]), cache, _pid(start_pos, len(tokens)))
    return oq.lm_head(W, cfg, h)[0]


def _oracle_prompt(W, cfg, ids, pix, thw, quantize):
    emb, pos, deltas = oq.get_input_embeddings(W, cfg, ids, torch.from_numpy(pix).to(BF) if pix is not None else None, thw)
    cache = oq._make_prompt_cache(cfg)
    oq.qwen2_model(W, cfg, emb, cache, torch.from_numpy(np.asarray(pos)))
    if quantize:
        quant.maybe_quantize_kv_cache(cache, 0, 64, 8)
    return cache, int(deltas[0, 0])


@pytest.mark.parametrize("chunk", [9, 70, 200])
@pytest.mark.parametrize("sizes", [[(56, 84)], []])
def test_chunk_onto_the_quantized_cache_every_row_then_decode(tiny, sizes, chunk):
    cfg, W, model = tiny
    lm = model.language_model
    ids, pix, thw = synth_request(cfg, sizes, n_text=14, seed=160 + len(sizes)) if sizes else \
        (np.random.default_rng(161).integers(3, 1000, (1, 23)), None, None)
    rng = np.random.default_rng(162 + chunk)
    new, forced = rng.integers(3, 1000, chunk), rng.integers(3, 1000, 8)
    kw = dict(image_grid_thw=thw) if thw is not None else {}
    f = model.get_input_embeddings(ids, torch.from_numpy(pix) if pix is not None else None, **kw)
    cache = lm.make_cache()
    seq = cache[0]._seq
    try:
        lm(ids, f.inputs_embeds, cache=cache, position_ids=f.position_ids, rope_deltas=f.rope_deltas, logits_to_keep=1)
        L0 = seq.offset
        lm.quantize_kv([seq], bits=8, group_size=64)
        delta = int(np.asarray(f.rope_deltas).reshape(-1)[0])
        got = lm(new[None], cache=cache, position_ids=_pid(L0 + delta, chunk).numpy()).logits[0].clone()      # all rows
        assert got.shape[0] == chunk and seq.q8 and seq.offset == L0 + chunk
        steps = [lm(np.array([[int(y)]]), cache=cache).logits[0, -1].clone() for y in forced]
    finally:
        seq.release()
    refs = {}
    for name, quantize in (("q8", True), ("bf16", False)):
        oc, odelta = _oracle_prompt(W, cfg, ids, pix, thw, quantize)
        assert odelta == delta and oc[0].offset == L0
        rows = _oracle_feed(W, cfg, oc, new, L0 + delta)
        dec = [_oracle_feed(W, cfg, oc, [int(y)], oq._cache_offset(oc[0]) + delta)[0] for y in forced]
        refs[name] = (rows, dec)
    d_q = [_rel_rms(got[i], refs["q8"][0][i]) for i in range(chunk)]
    d_p = [_rel_rms(got[i], refs["bf16"][0][i]) for i in range(chunk)]
    print(f"chunk {chunk} images={len(sizes)}: worst row {max(d_q):.4f}; mean distance to the 8-bit oracle {np.mean(d_q):.4f}, "
          f"to the bf16-cache oracle {np.mean(d_p):.4f}")
    assert max(d_q) < ROW_BAR, (max(d_q), d_q)
    assert np.mean(d_q) < np.mean(d_p), (np.mean(d_q), np.mean(d_p))
    # the chunk's tokens landed quantised in the right slots: the decode steps behind it follow the same oracle
    e = [_rel_rms(steps[i], refs["q8"][1][i]) for i in range(len(forced))]
    assert max(e) < ROW_BAR, e


def _turn(model, ids, state, max_tokens):
    from mlx_vlm_amd.generate import stream_generate

    r = list(stream_generate(model, None, input_ids=ids, prompt_cache_state=state, kv_bits=8, quantized_kv_start=0,
                             temperature=0.0, max_tokens=max_tokens))
    return [x.token for x in r[:-1]], r[-1]


def test_stream_generate_turns_on_a_quantized_prompt_cache(tiny):
    """turn 1 carries the cache past quantized_kv_start = 0; turn 2 = turn 1 + its reply + a new user turn of 70 tokens: the
    suffix is prefilled onto the 8-bit cache; turn 3 shares only a part of turn 2's tokens: the 8-bit cache is trimmed and the
    stale slots are overwritten by the next chunk's quantisation.  The oracle replays the same history on its
    QuantizedKVCache (fed the product's tokens); tokens equal up to ties (tests/test_engine_gpu.py::_tie_aware_equal, 3e-2)."""
    from mlx_vlm_amd.generate import PromptCacheState

    cfg, W, model = tiny
    rng = np.random.default_rng(170)
    ids1 = rng.integers(3, 1000, (1, 30))
    state = PromptCacheState()
    n_new = 8
    try:
        t1, last1 = _turn(model, ids1, state, n_new)
        assert last1.cached_tokens == 0 and state.cache[0]._seq.q8
        oc, _ = _oracle_prompt(W, cfg, ids1, None, None, quantize=True)
        for y in t1[:-1]:                                               # the cache holds every token that was fed back
            _oracle_feed(W, cfg, oc, [y], oc[0].offset)
            quant.maybe_quantize_kv_cache(oc, 0, 64, 8)
        assert oc[0].offset == state.cache[0].offset == ids1.shape[1] + len(t1) - 1

        def oracle_turn(suffix, toks):
            logits = [_oracle_feed(W, cfg, oc, suffix, oc[0].offset)[-1]]
            for y in toks[:-1]:
                logits.append(_oracle_feed(W, cfg, oc, [y], oc[0].offset)[0])
            ref_logits = torch.stack(logits)
            return [int(r.float().argmax()) for r in ref_logits], ref_logits

        ids2 = np.concatenate([ids1[0], t1, rng.integers(3, 1000, 70)])[None]
        have = state.cache[0].offset
        t2, last2 = _turn(model, ids2, state, n_new)
        assert len(t2) == n_new and last2.cached_tokens == have > 0 and state.cache[0]._seq.q8
        ref2, ref2_logits = oracle_turn(ids2[0, have:], t2)
        ok, n, margin = _tie_aware_equal(t2, ref2, ref2_logits, tol=3e-2)
        assert ok, (t2, ref2, n, margin)

        # turn 3: the same conversation up to 12 tokens into turn 2's user text, then something else (75 tokens)
        keep = ids1.shape[1] + len(t1) + 12
        ids3 = np.concatenate([ids2[0, :keep], rng.integers(3, 1000, 75)])[None]
        have = state.cache[0].offset
        assert keep < have
        t3, last3 = _turn(model, ids3, state, n_new)
        assert len(t3) == n_new and last3.cached_tokens == keep and state.cache[0]._seq.q8
        assert state.cache[0].offset == ids3.shape[1] + n_new - 1
        for c in oc:
            c.trim(have - keep)
        ref3, ref3_logits = oracle_turn(ids3[0, keep:], t3)
        ok, n, margin = _tie_aware_equal(t3, ref3, ref3_logits, tol=3e-2)
        assert ok, (t3, ref3, n, margin)
    finally:
        state.release()


def test_generate_step_onto_a_caller_owned_quantized_cache_whole_and_chunked(tiny):
    """generate_step(prompt_cache=a cache that is already 8-bit) over a 90-token suffix, in one chunk and in chunks of 32:
    both complete and agree the way tests/test_kv_quant_gpu.py::test_generate_step_with_kv_bits_and_a_chunked_prompt compares
    its two runs (the chosen tokens' log-probs within 0.13, tokens equal up to the first bf16 tie, at least 4 of 8)."""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = tiny
    lm = model.language_model
    rng = np.random.default_rng(180)
    ids, suffix = rng.integers(3, 1000, (1, 40)), rng.integers(3, 1000, (1, 90))
    runs = []
    for step_size in (4096, 32):
        cache = lm.make_cache()
        seq = cache[0]._seq
        try:
            lm(ids, cache=cache, logits_to_keep=1)
            lm.quantize_kv([seq], bits=8, group_size=64)
            pos = _pid(seq.offset, suffix.shape[1]).numpy()
            runs.append([(t, lp.float().cpu()) for t, lp in generate_step(
                suffix, model, None, None, prompt_cache=cache, position_ids=pos, rope_deltas=np.zeros((1, 1), dtype=np.int64),
                prefill_step_size=step_size, max_tokens=8, temperature=0.0, kv_bits=8, quantized_kv_start=0)])
            assert seq.q8 and seq.offset == 40 + 90 + 7
        finally:
            seq.release()
    whole, chunked = runs
    assert len(whole) == len(chunked) == 8
    n_equal = 0
    for (ta, la), (tb, lb) in zip(whole, chunked):
        assert abs(float(la[ta]) - float(lb[ta])) <= 0.13
        if ta != tb:
            break
        n_equal += 1
    assert n_equal >= 4, (n_equal, [t for t, _ in whole], [t for t, _ in chunked])


def test_a_chunk_onto_mixed_quantized_and_bf16_sequences_is_refused(tiny):
    cfg, W, model = tiny
    lm = model.language_model
    rng = np.random.default_rng(190)
    caches = lm.make_cache_batch(2)
    seqs = [c[0]._seq for c in caches]
    try:
        for c in caches:
            lm(rng.integers(3, 1000, (1, 20)), cache=c, logits_to_keep=1)
        lm.quantize_kv(seqs[:1], bits=8, group_size=64)
        emb = lm.embed_tokens(rng.integers(3, 1000, (2, 6))).reshape(12, -1)
        pos = np.broadcast_to(np.concatenate([20 + np.arange(6)] * 2)[None], (3, 12))
        with pytest.raises(RuntimeError, match="mix"):
            lm.prefill(emb, pos, caches, [6, 6], "last")
        assert [s.offset for s in seqs] == [20, 20]
    finally:
        for s in seqs:
            s.release()
