"""`max_kv_size` on the CAPTURED decode step (MI355X): the reference's RotatingKVCache (models/cache.py:442-625, keep = 4) as a
device-resident window - the ring lives in the paged pool at the reference's ring slots, a decode step writes at the ring's
slot, attends over the entries held and its tail advances the ring itself (include/vlm_hip.h VLM_DECODE_WINDOW; the rule and its
host mirror are pinned on the CPU side, tests/test_window_rule_cpu.py).

  * decode_begin + decode_run over a rotating sequence: the reference's own tokens (rotating_ref.npz `gen.*`), no tie rule;
  * generate_step(max_kv_size=) runs graph launches, not the eager loop; un-captured window steps give the same tokens;
  * an image prompt longer than the window (rope delta != 0, the one move call), three wraps, against the oracle;
  * two rows, one shorter and one longer than the window; continuation through the module call; a plain-offset family;
  * what stays outside: two rope tables (eager, unchanged), the 8-bit cache (refused), a caller's cache (look-ahead 1)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import llava_bunny as ob
from oracle import ops as O
from oracle import qwen2_vl as oq
from tests.helpers import bf16_close, build_bunny_model, build_product_model, synth_request

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "rotating_ref.npz"))
MAXS = int(G["max_kv_size"])
GREEDY = dict(temperature=0.0, top_p=1.0, min_p=0.0, top_k=0, seed=0)


def _rel_rms(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _peaked_tiny():
    """tests/test_rotating_gpu.py::_peaked_tiny: the next token is a permutation successor with a wide top-2 margin at every step"""
    cfg = oq.tiny_cfg()
    cfg.text.tie_word_embeddings = False
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * 0.5).to(BF)
    return cfg, oq.peak_head(W, cfg, gamma=4.0, stride=389, n_cycle=1000)


@pytest.fixture(scope="module")
def peaked():
    cfg, W = _peaked_tiny()
    return cfg, W, build_product_model(cfg, W, kv_pool_tokens=8192, max_seqs=16)


def _prefill(model, cache, ids, pix=None, thw=None):
    """first prompt through the module contract -> (first token [1] int32 device, its log-probs [V], rope deltas)"""
    from mlx_vlm_amd import ops

    lm = model.language_model
    kw = dict(image_grid_thw=thw) if thw is not None else {}
    f = model.get_input_embeddings(ids, torch.from_numpy(pix) if pix is not None else None, **kw)
    out = lm(ids, f.inputs_embeds, cache=cache, position_ids=f.position_ids, rope_deltas=f.rope_deltas, logits_to_keep=1)
    tok0, lp0 = ops.sample(out.logits[:, -1, :].contiguous(), step=torch.zeros(1, dtype=torch.int32, device=out.logits.device),
                           want_logprobs=True, **GREEDY)
    return tok0, lp0[0].clone(), np.asarray(f.rope_deltas).reshape(-1)[:1]


def _captured_run(model, ids, n_tokens, max_kv_size, use_graph=True, pix=None, thw=None, keep_cache=False):
    """prefill + decode_begin + n_tokens - 1 decode_run steps (greedy) -> (tokens, log-prob rows, logits rows[, cache, state])"""
    from mlx_vlm_amd.models import cache as cache_mod

    lm = model.language_model
    cache = cache_mod.make_prompt_cache(lm, max_kv_size=max_kv_size)
    tok0, lp0, deltas = _prefill(model, cache, ids, pix, thw)
    st = lm.decode_begin([cache], tok0, deltas, max_new_tokens=n_tokens + 1)
    assert st.window == (max_kv_size, 4, 1)
    st.step.fill_(1)
    toks, lps, logits = [int(tok0[0])], [lp0.float().cpu()], [None]
    for _ in range(n_tokens - 1):
        lm.decode_run(st, 1, GREEDY, use_graph=use_graph)
        toks.append(int(st.tok[0]))
        lps.append(st.logprobs[0].float().cpu())
        logits.append(st.logits[0].float().cpu())
    seq = cache[0]._seq
    assert seq.offset == ids.shape[1] + n_tokens - 1 and seq.kv_entries <= max_kv_size - 1 and cache[0].size() == min(seq.offset, max_kv_size)
    if keep_cache:
        return toks, lps, logits, cache, st
    seq.release()
    return toks, lps, logits


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name", ["short", "long"])
def test_captured_decode_over_a_rotating_sequence_gives_the_references_tokens(peaked, name, use_graph):
    """the reference's own generate_step(max_kv_size=24) run: tokens IDENTICAL, log-probs within 2 ulps + 3 % rms (the bar of
    tests/test_rotating_gpu.py's golden test)"""
    cfg, W, model = peaked
    ids = G[f"gen.{name}.input_ids"]
    ref_toks, ref_lp = G[f"gen.{name}.tokens"].tolist(), torch.from_numpy(G[f"gen.{name}.logprobs"])
    toks, lps, _ = _captured_run(model, ids, len(ref_toks), MAXS, use_graph=use_graph)
    assert toks == ref_toks
    for i in range(len(toks)):
        ok, rep = bf16_close(lps[i], ref_lp[i].to(BF), ulps=2, atol_rms=3e-2)
        print(f"captured window {name} graph={use_graph} step {i}: {rep}")
        assert ok, (i, rep)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["short", "long"])
def test_generate_step_with_max_kv_size_takes_the_captured_path(peaked, name, monkeypatch):
    from mlx_vlm_amd import _lib
    from mlx_vlm_amd import generate as gen_mod

    cfg, W, model = peaked
    lm = model.language_model
    ids = G[f"gen.{name}.input_ids"]
    ref_toks = G[f"gen.{name}.tokens"].tolist()

    def no_eager(*a, **k):
        raise AssertionError("_generate_step_eager entered")

    monkeypatch.setattr(gen_mod, "_generate_step_eager", no_eager)
    L = _lib.lib()
    counts = {"launch": 0, "step": 0, "flags": set()}
    real_launch, real_step, real_build = L.vlm_llm_decode_graph_launch, L.vlm_llm_decode_step, L.vlm_llm_decode_graph_build

    def launch(*a):
        counts["launch"] += 1
        return real_launch(*a)

    def step(h, args, stream):
        counts["step"] += 1
        counts["flags"].add(int(args._obj.flags))
        return real_step(h, args, stream)

    def build(h, args, stream):
        counts["flags"].add(int(args._obj.flags))
        return real_build(h, args, stream)

    monkeypatch.setattr(L, "vlm_llm_decode_graph_launch", launch)
    monkeypatch.setattr(L, "vlm_llm_decode_step", step)
    monkeypatch.setattr(L, "vlm_llm_decode_graph_build", build)
    toks = [t for t, _ in gen_mod.generate_step(ids, model, None, None, max_tokens=len(ref_toks), temperature=0.0, max_kv_size=MAXS)]
    assert toks == ref_toks
    assert counts["launch"] == len(ref_toks) - 1 and counts["step"] == 0
    st = lm.decode_state(1)
    assert st.window == (MAXS, 4, 1) and (MAXS, 4, 1) in st.graph_key       # the graph key sees the mode
    assert all(f & _lib.DECODE_WINDOW for f in counts["flags"])              # (a build, if this run needed one)
    assert [L.vlm_llm_get_tuning(lm._handle, k) for k in (_lib.MODE_WINDOW_SIZE, _lib.MODE_WINDOW_KEEP, _lib.MODE_WINDOW_RING_POS)] == [MAXS, 4, 1]
    # un-captured window steps: the same tokens
    counts.update(launch=0, step=0)
    toks = [t for t, _ in gen_mod.generate_step(ids, model, None, None, max_tokens=len(ref_toks), temperature=0.0, max_kv_size=MAXS,
                                                use_graph=False)]
    assert toks == ref_toks and counts["launch"] == 0 and counts["step"] == len(ref_toks) - 1
    assert counts["flags"] and all(f & _lib.DECODE_WINDOW for f in counts["flags"])
    # and an unbounded run on the same model afterwards is untouched by the mode values
    plain = [t for t, _ in gen_mod.generate_step(ids, model, None, None, max_tokens=8, temperature=0.0)]
    assert plain == oq.generate_greedy(W, cfg, ids, max_tokens=8)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_image_prompt_longer_than_the_window_wraps_three_times(peaked):
    """rope delta != 0, the L > M start state and the one move call; 70 steps at max_kv_size 20"""
    cfg, W, model = peaked
    ids, pix, thw = synth_request(cfg, [(56, 84)], n_text=14, seed=44)
    maxs, n_tokens = 20, 71
    assert ids.shape[1] > maxs
    pix_t = torch.from_numpy(pix).to(BF)
    ref_toks = oq.generate_greedy(W, cfg, ids, pix_t, thw, max_tokens=n_tokens, max_kv_size=maxs)
    toks, lps, logits = _captured_run(model, ids, n_tokens, maxs, pix=pix, thw=thw)
    assert toks == ref_toks
    ref = oq.decode_teacher_forced(W, cfg, ids, pix_t, thw, toks[:-1], max_kv_size=maxs)
    errs_lp = [_rel_rms(lps[i], O.logprobs_from_logits(ref[i:i + 1])[0]) for i in range(n_tokens)]
    errs = [_rel_rms(logits[i], ref[i]) for i in range(1, n_tokens)]
    print(f"image prompt over the window: worst log-prob rel-rms {max(errs_lp):.4f}, worst logits rel-rms {max(errs):.4f}")
    assert max(errs_lp) < 2e-2, (max(errs_lp), errs_lp)
    assert max(errs) < 2e-2, (max(errs), errs)
    # the bound does change the function: past the wrap the rows are nearer the windowed oracle than the unbounded one
    plain = oq.decode_teacher_forced(W, cfg, ids, pix_t, thw, toks[:-1])
    assert np.mean([_rel_rms(logits[i], ref[i]) for i in range(3, n_tokens)]) < 0.5 * np.mean([_rel_rms(logits[i], plain[i]) for i in range(3, n_tokens)])


# ---------------------------------------------------------------------------------------------------------------- 4
def test_two_rows_one_shorter_and_one_longer_than_the_window(peaked):
    cfg, W, model = peaked
    lm = model.language_model
    prompts = [G["gen.short.input_ids"], G["gen.long.input_ids"]]
    assert prompts[0].shape[1] < MAXS < prompts[1].shape[1]
    n_tokens = 40
    singles = [_captured_run(model, p, n_tokens, MAXS) for p in prompts]
    caches = lm.make_cache_batch(2)
    for c in caches:
        c[0]._seq.set_rotating(MAXS, keep=4)
    firsts = [_prefill(model, c, p) for c, p in zip(caches, prompts)]
    tok0 = torch.cat([f[0] for f in firsts])
    st = lm.decode_begin(caches, tok0, np.zeros((2, 1), dtype=np.int64), max_new_tokens=n_tokens + 1)
    assert st.window == (MAXS, 4, 1)
    st.step.fill_(1)
    rows = [[int(tok0[b])] for b in range(2)]
    lps = [[firsts[b][1].float().cpu()] for b in range(2)]
    for _ in range(n_tokens - 1):
        lm.decode_run(st, 1, GREEDY)
        t = st.tok[:2].cpu().tolist()
        for b in range(2):
            rows[b].append(int(t[b]))
            lps[b].append(st.logprobs[b].float().cpu())
    for b in range(2):
        assert rows[b] == singles[b][0], b                    # (peaked head: tokens are decided - no tie rule)
        for i in range(n_tokens):
            ok, rep = bf16_close(lps[b][i], singles[b][1][i].to(BF), ulps=2, atol_rms=3e-2)
            assert ok, (b, i, rep)
        s = caches[b][0]._seq
        assert s.offset == prompts[b].shape[1] + n_tokens - 1 and s.kv_entries <= MAXS - 1
        s.release()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_module_calls_continue_a_captured_run(peaked):
    """30 captured steps, then three one-token module calls on the same cache: each against the oracle's teacher-forced row"""
    cfg, W, model = peaked
    lm = model.language_model
    ids = G["gen.long.input_ids"]
    toks, _, _, cache, st = _captured_run(model, ids, 31, MAXS, keep_cache=True)
    seq = cache[0]._seq
    state = seq.window_state()
    fed = toks + [17, 905]                                   # tok30 (sampled, not fed yet), then two arbitrary tokens
    ref = oq.decode_teacher_forced(W, cfg, ids, None, None, fed, max_kv_size=MAXS)
    lm._rope_deltas = np.zeros((1, 1), dtype=np.int64)
    for j, y in enumerate(fed[30:]):
        row = lm(np.array([[int(y)]]), cache=cache).logits[0, -1]
        err = _rel_rms(row, ref[31 + j])
        print(f"module call {j} after a captured run: rel-rms {err:.4f}")
        assert err < 2e-2, (j, err)
    assert seq.win_w is not None and seq.ring is None and seq.offset == ids.shape[1] + 33
    n, w, r = state
    from mlx_vlm_amd.models import cache as cache_mod
    for _ in range(3):
        n, w, r = cache_mod.window_step(n, w, r, MAXS, 4)
    assert seq.window_state() == (n, w, r)
    with pytest.raises(NotImplementedError):
        cache[0].trim(1)                                     # a wrapped window stays untrimmable
    seq.release()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_plain_offset_family_through_the_captured_window(monkeypatch):
    """nanoLLaVA (rope offset = cache.offset: ring_pos = 0), a text prompt longer than the window: every step's log-probs against
    the oracle's typed graph over RotatingKVCache(max_size, keep=4) fed the same tokens; tokens equal the oracle row's argmax up
    to bf16 ties of the log-probs"""
    from mlx_vlm_amd import generate as gen_mod
    from tests.test_vlm_family_llava_bunny_gpu import _tie_aware

    cfg = ob.tiny_cfg()
    W = {k: v.to(BF) for k, v in ob.random_weights(cfg, seed=4321, dtype=torch.float32, **ob.TEST_WEIGHT_SCALES).items()}
    model = build_bunny_model(cfg, W, kv_pool_tokens=4096, max_seqs=8)
    assert model.language_model.ROTATING_POS_FROM_RING is False

    def no_eager(*a, **k):
        raise AssertionError("_generate_step_eager entered")

    monkeypatch.setattr(gen_mod, "_generate_step_eager", no_eager)
    maxs, n_tokens = 20, 50
    ids = np.random.default_rng(21).integers(3, 200, (1, 33))
    toks, lps = [], []
    for t, lp in gen_mod.generate_step(ids, model, None, None, max_tokens=n_tokens, temperature=0.0, max_kv_size=maxs):
        toks.append(t)
        lps.append(lp.float().cpu())
    cache = [O.RotatingKVCache(maxs, keep=4) for _ in range(cfg.text.num_hidden_layers)]
    rows = [ob.language_model(W, cfg, ob.get_input_embeddings(W, cfg, ids, None), cache)[0, -1]]
    for y in toks[:-1]:
        rows.append(ob.language_model(W, cfg, ob.embed_tokens(W, np.array([[int(y)]])), cache)[0, -1])
    ref = torch.stack(rows)
    errs = [_rel_rms(lps[i], O.logprobs_from_logits(ref[i:i + 1])[0]) for i in range(n_tokens)]
    print(f"plain-offset family over the window: worst log-prob rel-rms {max(errs):.4f}")
    assert max(errs) < 2e-2, (max(errs), errs)
    for i in range(n_tokens):
        ok, _ = _tie_aware([toks[i]], [int(O.argmax_first(O.logprobs_from_logits(ref[i:i + 1]))[0])], ref[i:i + 1], tol=3e-2)
        assert ok, (i, toks[i])


# ---------------------------------------------------------------------------------------------------------------- 7
def test_two_rope_tables_stay_on_the_eager_path(monkeypatch):
    """Phi-3.5-vision: the qkv epilogue derives the long-factor regime from the slot - generate_step(max_kv_size=) keeps running
    the eager loop and gives what the module calls give"""
    from mlx_vlm_amd import generate as gen_mod
    from mlx_vlm_amd.models import cache as cache_mod
    from oracle import phi3_v as op
    from tests.helpers import build_phi3v_model
    from tests.test_vlm_family_phi3v_gpu import SCALES

    cfg = op.tiny_cfg()
    model = build_phi3v_model(cfg, op.random_weights(cfg, seed=4321, dtype=BF, **SCALES), kv_pool_tokens=4096, max_seqs=4)
    lm = model.language_model
    assert not lm.supports_window_decode()
    ids = np.random.default_rng(5).integers(3, 200, (1, 40))
    maxs, n_tokens = 48, 30
    entered = []
    real = gen_mod._generate_step_eager

    def spy(*a, **k):
        entered.append(1)
        return real(*a, **k)

    monkeypatch.setattr(gen_mod, "_generate_step_eager", spy)
    toks = [t for t, _ in gen_mod.generate_step(ids, model, None, None, max_tokens=n_tokens, temperature=0.0, max_kv_size=maxs)]
    assert entered == [1]
    # the same loop by hand through the module contract (the host-planned ring)
    cache = cache_mod.make_prompt_cache(lm, max_kv_size=maxs)
    logits = lm(ids, cache=cache, logits_to_keep=1).logits[:, -1, :]
    from mlx_vlm_amd import ops

    want = []
    step = torch.zeros(1, dtype=torch.int32, device=logits.device)
    for i in range(n_tokens):
        y = int(ops.sample(logits.reshape(1, -1).contiguous(), step=step, want_logprobs=False, **GREEDY)[0][0])
        want.append(y)
        if i < n_tokens - 1:
            logits = lm(np.array([[y]]), cache=cache).logits[:, -1, :]
    assert cache[0]._seq.win_w is None and cache[0]._seq.ring is not None
    cache[0]._seq.release()
    assert toks == want
    # the engine refuses the flag for such a config, and decode_begin refuses to bind such rows
    cache = cache_mod.make_prompt_cache(lm, max_kv_size=maxs)
    lm(ids, cache=cache, logits_to_keep=1)
    with pytest.raises(NotImplementedError):
        lm.decode_begin([cache], [5], np.zeros((1, 1), dtype=np.int64), max_new_tokens=4)
    cache[0]._seq.release()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_callers_cache_runs_one_step_ahead_and_holds_the_tokens_fed(peaked):
    from mlx_vlm_amd.generate import generate_step
    from mlx_vlm_amd.models import cache as cache_mod

    cfg, W, model = peaked
    lm = model.language_model
    ids = G["gen.long.input_ids"]                           # longer than the window: every look-ahead step overwrites an entry
    L = ids.shape[1]
    cache = cache_mod.make_prompt_cache(lm, max_kv_size=MAXS)
    runs = []
    real = lm.decode_run

    def spy(st, n, *a, **k):
        runs.append(n)
        return real(st, n, *a, **k)

    lm.decode_run = spy
    try:
        g = generate_step(ids, model, None, None, max_tokens=32, temperature=0.0, prompt_cache=cache, lookahead=4)
        toks = [next(g)[0] for _ in range(3)]
        g.close()
    finally:
        del lm.decode_run
    assert sum(runs) == 3                                    # one step ahead of the third token, not four
    seq = cache[0]._seq
    # the cache holds prompt + the tokens FED (every yielded token except the last); the host's window state is that of two steps
    n, w, src, dst = cache_mod.window_start(L, MAXS, 4)
    r = L
    for _ in range(2):
        n, w, r = cache_mod.window_step(n, w, r, MAXS, 4)
    assert cache[0].offset == L + 2 and seq.window_state() == (n, w, r)
    assert toks == G["gen.long.tokens"].tolist()[:3]
    # ... and so does the pool: the next module-call step (feeding the third token) against the oracle's teacher-forced row
    ref = oq.decode_teacher_forced(W, cfg, ids, None, None, toks, max_kv_size=MAXS)
    lm._rope_deltas = np.zeros((1, 1), dtype=np.int64)
    row = lm(np.array([[toks[2]]]), cache=cache).logits[0, -1]
    err = _rel_rms(row, ref[3])
    print(f"caller-owned window after a closed generator: next step rel-rms {err:.4f}")
    assert err < 2e-2, err
    seq.release()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_window_over_the_8bit_cache_is_refused(peaked):
    from mlx_vlm_amd import _lib
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = peaked
    lm = model.language_model
    ids = np.random.default_rng(9).integers(3, 1000, (1, 40))
    with pytest.raises(NotImplementedError, match="RotatingKVCache Quantization NYI"):
        next(generate_step(ids, model, None, None, max_tokens=4, max_kv_size=16, kv_bits=8, quantized_kv_start=0))
    # the engine itself: the flag without a window size is an argument error (nothing is enqueued)
    L = _lib.lib()
    st = lm.decode_state(1)
    lm._set_window_mode((0, 0, 0))
    args = st.args(flags=_lib.DECODE_WINDOW)
    assert L.vlm_llm_decode_step(lm._handle, C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 1
    lm._set_window_mode((6, 5, 0))                           # M <= keep + 1
    assert L.vlm_llm_decode_step(lm._handle, C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 1
    lm._set_window_mode((0, 0, 0))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_device_side_penalties_ride_in_the_captured_window_step(peaked, monkeypatch):
    from mlx_vlm_amd import generate as gen_mod

    cfg, W, model = peaked
    ids = G["gen.long.input_ids"]
    kw = dict(max_tokens=40, temperature=0.0, max_kv_size=MAXS, repetition_penalty=1.3, repetition_context_size=16,
              presence_penalty=0.4, frequency_penalty=0.2, logit_bias={7: 1.5, 901: -2.0})
    # the eager path: an identity Python processor cannot live in a captured step
    eager = [t for t, _ in gen_mod.generate_step(ids, model, None, None, logits_processors=[lambda tokens, logits: logits], **kw)]

    def no_eager(*a, **k):
        raise AssertionError("_generate_step_eager entered")

    monkeypatch.setattr(gen_mod, "_generate_step_eager", no_eager)
    got = [t for t, _ in gen_mod.generate_step(ids, model, None, None, **kw)]
    assert got == eager
