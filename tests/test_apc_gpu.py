"""`BatchGenerator(apc_manager=)` end to end on the GPU: a request whose prompt shares an image and its first 128 tokens with an
earlier one is admitted WARM - the matched blocks are copied into its pages, the vision tower is not called, only the suffix
is prefilled (its queries attending over the pages: csrc/attn_prefill_paged.hip) - and must give the oracle's tokens and the
cold path's first log-prob row.  The model is the peaked-head tiny Qwen2-VL of tests/test_rotating_gpu.py (greedy tokens are
decided by a margin: compared for equality, no tie allowance), in both KV pool layouts (`kv_layout=` reaches the pool through
build_product_model)."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from oracle import qwen2_vl as oq
from tests.helpers import bf16_close, build_product_model, synth_request

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_NEW = 6


def _peaked_tiny():
    cfg = oq.tiny_cfg()
    cfg.text.tie_word_embeddings = False
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * 0.5).to(BF)
    return cfg, oq.peak_head(W, cfg, gamma=4.0, stride=389, n_cycle=1000)


class CountingTower:
    """counts the calls of the vision tower it wraps"""

    def __init__(self, tower):
        self._tower, self.calls = tower, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self._tower(*a, **kw)

    def __getattr__(self, name):
        return getattr(self._tower, name)


@pytest.fixture(scope="module", params=["paged", "identity"])
def peaked(request):
    cfg, W = _peaked_tiny()
    model = build_product_model(cfg, W, kv_pool_tokens=4096, max_seqs=8, kv_layout=request.param)
    assert model.language_model.pool.identity == (request.param == "identity")
    model.vision_tower = CountingTower(model.vision_tower)
    return cfg, W, model


@pytest.fixture(scope="module")
def reqs():
    """A: one 56 x 56 image (4 placeholder tokens: the span ends at token 5) + 140 text tokens; B: A's first 128 tokens and
    another tail; C: B's text under another image; D / E: a 224 x 224 image whose span (64 tokens) ends at token 65 - inside the
    second block - and the same image under another text; F: text only"""
    cfg = oq.tiny_cfg()
    rng = np.random.default_rng(77)
    a_ids, pix, thw = synth_request(cfg, [(56, 56)], n_text=140, seed=31)
    a_ids = a_ids.reshape(-1)
    assert a_ids.size >= 140 and int(np.nonzero(a_ids == cfg.image_token_id)[0][-1]) + 1 < 128
    tail = lambda n: rng.integers(3, 1000, n)                        # noqa: E731
    b_ids = np.concatenate([a_ids[:128], tail(21)])
    b2_ids = np.concatenate([a_ids[:128], tail(9)])
    _, pix_c, thw_c = synth_request(cfg, [(56, 56)], n_text=1, seed=32)
    assert not np.array_equal(pix, pix_c)
    d_ids, pix_d, thw_d = synth_request(cfg, [(224, 224)], n_text=80, seed=33)
    d_ids = d_ids.reshape(-1)
    span_end = int(np.nonzero(d_ids == cfg.image_token_id)[0][-1]) + 1
    assert 64 < span_end < 128
    e_ids = np.concatenate([d_ids[:span_end + 1], tail(75)])
    kw = lambda p, t: dict(pixel_values=torch.from_numpy(p), image_grid_thw=t)     # noqa: E731
    return dict(A=(a_ids, kw(pix, thw)), B=(b_ids, kw(pix, thw)), B2=(b2_ids, kw(pix, thw)), C=(b_ids, kw(pix_c, thw_c)),
                D=(d_ids, kw(pix_d, thw_d)), E=(e_ids, kw(pix_d, thw_d)), F=(tail(150), {}),
                raw=dict(pix=pix, thw=thw))


def _capturing(BatchGenerator):
    class Capturing(BatchGenerator):
        """keeps the first tokens' log-prob rows of every admission and the pages of every admitted sequence"""

        def _prefill_requests(self, batch):
            out = super()._prefill_requests(batch)
            self.first_rows = getattr(self, "first_rows", {})
            self.pages_of = getattr(self, "pages_of", {})
            self.admission_sizes = getattr(self, "admission_sizes", []) + [len(batch)]
            for b, c, row in zip(batch, out[0], self._last_lp_rows.float().cpu()):
                self.first_rows[b[0]] = row.clone()
                self.pages_of[b[0]] = list(c[0]._seq.pages)
            return out

    return Capturing


def _run(gen, items, max_tokens=N_NEW):
    """insert `items` [(ids, kwargs)] at once, run to completion -> tokens per request"""
    uids = gen.insert([i for i, _ in items], max_tokens, prompt_kwargs=[k for _, k in items])
    got = {u: [] for u in uids}
    rounds = 0
    while gen.has_work:
        progress, out = gen.next()
        gen.cached_seen = {**getattr(gen, "cached_seen", {}), **{p.uid: p.cached_tokens for p in progress}}
        rounds += 1
        assert rounds < 200
        for r in out:
            got[r.uid].append(r.token)
    return uids, [got[u] for u in uids]


def _make(model, mgr=None, **kw):
    from mlx_vlm_amd.batch import BatchGenerator

    return _capturing(BatchGenerator)(model, None, max_tokens=N_NEW, completion_batch_size=4, top_logprobs_k=2,
                                      **({"apc_manager": mgr} if mgr is not None else {}), **kw)


@pytest.mark.parametrize("async_prefill", [True, False])
def test_warm_admission_equals_the_oracle_and_the_cold_path(peaked, reqs, async_prefill):
    from mlx_vlm_amd.apc import APCManager

    cfg, W, model = peaked
    lm, tower = model.language_model, model.vision_tower
    free_seqs = len(lm.pool._free_seqs)
    mgr = APCManager(num_blocks=8)
    gen = _make(model, mgr, async_prefill=async_prefill)
    (a_ids, a_kw), (b_ids, b_kw) = reqs["A"], reqs["B"]
    kvv, vvv = APCManager._pool_views(lm.pool)
    # ---- A, cold, to completion
    (ua,), _ = _run(gen, [reqs["A"]])
    torch.cuda.synchronize()
    snap = mgr.stats_snapshot()
    assert (snap["lookups_hit"], snap["lookups_miss"], snap["stores"]) == (0, 1, a_ids.size // 64)
    a_pages = gen.pages_of[ua][:2]
    a_k, a_v = kvv[:, a_pages].clone(), vvv[:, a_pages].clone()           # (decode steps write past the prompt: page 2 on)
    # ---- B, warm.  First: it WAS warm, and the tower was not called for it
    calls = tower.calls
    (ub,), (b_toks,) = _run(gen, [reqs["B"]])
    torch.cuda.synchronize()
    snap = mgr.stats_snapshot()
    assert snap["lookups_hit"] == 1 and snap["matched_tokens"] == 128
    assert tower.calls == calls
    assert snap["served_tokens"] == a_ids.size + b_ids.size - 128
    assert gen.cached_seen[ua] == 0 and gen.cached_seen[ub] == 128                 # PromptProgress.cached_tokens
    b_pages = gen.pages_of[ub][:2]
    # (in the paged layout B may have been given the very pages A released: the restore still had to rewrite them - their bytes
    #  were A's only if nothing else ran in between, which the equality with the clone does not rely on)
    assert torch.equal(kvv[:, b_pages], a_k) and torch.equal(vvv[:, b_pages], a_v)          # every layer, K and V
    ref_toks, ref_logits = oq.generate_greedy(W, cfg, b_ids[None], torch.from_numpy(reqs["raw"]["pix"]).to(BF), reqs["raw"]["thw"],
                                              max_tokens=N_NEW, return_logits=True)
    assert b_toks == ref_toks
    ok, rep = bf16_close(gen.first_rows[ub], O.logprobs_from_logits(ref_logits[0][None])[0], ulps=2, atol_rms=3e-2)
    assert ok, rep
    # ---- B warm once more: bit-equal log-probs
    (ub2,), (b_toks2,) = _run(gen, [reqs["B"]])
    assert mgr.stats_snapshot()["lookups_hit"] == 2 and tower.calls == calls
    assert b_toks2 == b_toks and torch.equal(gen.first_rows[ub2], gen.first_rows[ub])
    gen.close()
    # ---- B from a fresh generator without a manager
    plain = _make(model, async_prefill=async_prefill)
    (up,), (p_toks,) = _run(plain, [reqs["B"]])
    assert tower.calls == calls + 1 and p_toks == b_toks
    ok, rep = bf16_close(gen.first_rows[ub], plain.first_rows[up], ulps=2, atol_rms=3e-2)
    assert ok, rep
    plain.close()
    assert len(lm.pool._free_seqs) == free_seqs and all(b.ref_cnt == 0 for b in mgr.blocks)
    mgr.close()


def test_cold_cases_reject_and_mixed_admission(peaked, reqs):
    from mlx_vlm_amd.apc import APCManager

    cfg, W, model = peaked
    tower = model.vision_tower
    plain = _make(model)
    alone = {k: _run(plain, [reqs[k]])[1][0] for k in ("B", "B2", "C", "E", "F")}
    plain.close()
    mgr = APCManager(num_blocks=16)
    gen = _make(model, mgr, prefill_batch_size=3)
    _run(gen, [reqs["A"]])
    # the same text under another image: cold
    miss, calls = mgr.stats_snapshot()["lookups_miss"], tower.calls
    assert _run(gen, [reqs["C"]])[1][0] == alone["C"]
    snap = mgr.stats_snapshot()
    assert snap["lookups_miss"] == miss + 1 and snap["lookups_hit"] == 0 and tower.calls == calls + 1
    # a match that ends inside the image span: cold, one reject
    _run(gen, [reqs["D"]])
    calls = tower.calls
    assert _run(gen, [reqs["E"]])[1][0] == alone["E"]
    snap = mgr.stats_snapshot()
    assert snap["rejects"] == 1 and snap["rejects_by_reason"] == {"media_suffix": 1} and tower.calls == calls + 1
    assert snap["lookups_hit"] == 1 and snap["matched_tokens"] == 64              # (the lookup did match the first block)
    # ONE admission with one cold and two warm requests
    served, calls = snap["served_tokens"], tower.calls
    items = [reqs["B2"], reqs["F"], reqs["B"]]
    _, streams = _run(gen, items)
    assert gen.admission_sizes[-1] == 3
    assert streams == [alone["B2"], alone["F"], alone["B"]]
    snap = mgr.stats_snapshot()
    assert snap["lookups_hit"] == 3 and tower.calls == calls                      # F is text: nobody needed the tower
    assert snap["served_tokens"] == served + sum(i[0].size for i in items) - 2 * 128
    gen.close()
    mgr.close()


def test_small_store_evicts_and_everything_completes(peaked, reqs):
    from mlx_vlm_amd.apc import APCManager

    cfg, W, model = peaked
    plain = _make(model)
    alone = [_run(plain, [reqs[k]])[1][0] for k in ("A", "F", "D")]
    plain.close()
    mgr = APCManager(num_blocks=2)
    gen = _make(model, mgr)
    for k, want in zip(("A", "F", "D"), alone):
        assert _run(gen, [reqs[k]])[1][0] == want
    snap = mgr.stats_snapshot()
    assert snap["evictions"] > 0 and snap["pool_used"] == 2 and snap["stores"] == 6
    gen.close()
    mgr.close()


def test_failed_warm_prefill_returns_its_sequences(peaked, reqs, monkeypatch):
    """one admission, a cold request that succeeds and a warm one whose prefill raises: no sequence slot, page or block reference
    stays behind"""
    from mlx_vlm_amd.apc import APCManager

    cfg, W, model = peaked
    lm = model.language_model
    mgr = APCManager(num_blocks=8)
    gen = _make(model, mgr, async_prefill=False, prefill_batch_size=2)
    _run(gen, [reqs["A"]])
    free = (len(lm.pool._free_seqs), len(lm.pool._free_pages))
    real = lm.prefill

    def failing(*a, paged_attn=False, **kw):
        if paged_attn:
            raise RuntimeError("warm prefill failed")
        return real(*a, **kw)

    monkeypatch.setattr(lm, "prefill", failing)
    gen.insert([reqs["F"][0], reqs["B"][0]], N_NEW, prompt_kwargs=[reqs["F"][1], reqs["B"][1]])
    with pytest.raises(RuntimeError, match="warm prefill failed"):
        gen.next()
    assert mgr.stats_snapshot()["lookups_hit"] == 1
    assert (len(lm.pool._free_seqs), len(lm.pool._free_pages)) == free
    assert all(b.ref_cnt == 0 for b in mgr.blocks)
    monkeypatch.undo()
    assert _run(gen, [reqs["B"]])[1][0]                       # the generator and the manager go on working
    gen.close()
    mgr.close()


def test_refusals(peaked):
    from mlx_vlm_amd.apc import APCManager
    from mlx_vlm_amd.batch import BatchGenerator
    from oracle import llava_bunny as ob
    from tests.helpers import build_bunny_model

    cfg, W, model = peaked
    with pytest.raises(NotImplementedError, match="kv_bits"):
        BatchGenerator(model, None, kv_bits=8, apc_manager=APCManager(num_blocks=2))
    bcfg = ob.tiny_cfg()
    bW = {k: v.to(BF) for k, v in ob.random_weights(bcfg, seed=4321, dtype=torch.float32, **ob.TEST_WEIGHT_SCALES).items()}
    bunny = build_bunny_model(bcfg, bW, kv_pool_tokens=1024, max_seqs=4)
    with pytest.raises(NotImplementedError, match="Qwen2-VL"):
        BatchGenerator(bunny, None, apc_manager=APCManager(num_blocks=2))
