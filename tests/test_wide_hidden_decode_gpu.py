"""Decode at Qwen2-VL-72B's attention geometry: hidden 8192, 64 query heads over 8 KV heads of 128 (o_proj K = 8192, GQA
group 8), 2 layers, intermediate 2048, vocabulary 1024, a depth-1 vision tower whose merger writes 8192 columns (~0.8 GB of
bf16).  Before hidden sizes past 4096 were built, every step of up to 16 rows failed here with "unsupported shape" from
the first qkv launch.

Weights: oracle.qwen2_vl.random_weights(std=0.02, fast=True), as tests/test_full_depth_gpu.py draws its real-width models,
then scaled the way tests/helpers.py::peaked_full_depth scales (embedding x 50, every o_proj / down_proj x 0.1; no head
peak).  Unscaled, an embedding of 0.02 rms is swamped by branch outputs of ~1.8 rms per element (0.02 * sqrt(8192)) and the
oracle's own bf16 graph sits 2.0 - 2.6 % (rel-rms of a logit row) from its float32 graph - above the bar.  Scaled, that
distance is 0.6 % (measured on the B = 1 inputs below; the fixture asserts it is under half of the bar).

Bar: 2e-2 rel-rms of every logit row against oracle.qwen2_vl.decode_teacher_forced, the project's bar for two bf16 layers.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model, synth_request

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2e-2
EMBED_GAIN, BRANCH_GAIN = 50.0, 0.1


def _rel_rms(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _check_rows(got, ref, tol_rms, tag):
    """every row within tol_rms (rel-rms); argmax identical wherever the oracle's top-2 margin exceeds 0.25 rms (copied from
    tests/test_full_depth_gpu.py)"""
    errs = [_rel_rms(got[i], ref[i]) for i in range(ref.shape[0])]
    print(f"{tag}: row rel-rms " + " ".join(f"{e:.4f}" for e in errs))
    assert max(errs) < tol_rms, (tag, errs)
    for i in range(ref.shape[0]):
        r = ref[i].float()
        top2 = r.topk(2).values
        if float(top2[0] - top2[1]) > 0.25 * float(r.pow(2).mean().sqrt()):
            assert int(got[i].float().argmax()) == int(r.argmax()), (tag, i)
    return max(errs)


def _cfg():
    text = oq.TextCfg(hidden_size=8192, num_hidden_layers=2, intermediate_size=2048, num_attention_heads=64,
                      num_key_value_heads=8, vocab_size=1024, tie_word_embeddings=False)
    return oq.Cfg(text=text, vision=oq.VisionCfg(depth=1, embed_dim=160, hidden_size=8192, num_heads=2),
                  image_token_id=1001, video_token_id=1002, vision_start_token_id=1003)


@functools.lru_cache(maxsize=None)
def _weights():
    cfg = _cfg()
    W = oq.random_weights(cfg, seed=75, dtype=BF, std=0.02, fast=True)
    k = "language_model.model.embed_tokens.weight"
    W[k] = (W[k].float() * EMBED_GAIN).to(BF)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * BRANCH_GAIN).to(BF)
    return cfg, W


@functools.lru_cache(maxsize=None)
def _image_request():
    """image + text prompt, 4 forced tokens, the oracle's rows (bf16 graph): shared by the B = 1 cases"""
    cfg, W = _weights()
    ids, pix, thw = synth_request(cfg, [(56, 84)], n_text=12, seed=1)
    forced = np.random.default_rng(2).integers(3, 1000, 4)
    ref = oq.decode_teacher_forced(W, cfg, ids, torch.from_numpy(pix).to(BF), thw, forced)
    return ids, pix, thw, forced, ref


@pytest.fixture(scope="module")
def wide():
    cfg, W = _weights()
    ids, pix, thw, forced, ref = _image_request()
    # the oracle's own typed-vs-float32 distance on these inputs must leave the bar room (CPU only)
    ref32 = oq.decode_teacher_forced({k: v.float() for k, v in W.items()}, cfg, ids, torch.from_numpy(pix), thw, forced)
    d_typed = max(_rel_rms(ref[i], ref32[i]) for i in range(len(ref)))
    print(f"oracle bf16 graph vs float32 graph: {d_typed:.4f}")
    assert d_typed < TOL / 2, d_typed
    return cfg, W, build_product_model(cfg, W, kv_pool_tokens=32768, max_seqs=72)


def _teacher_forced(model, ids, pix, thw, forced):
    lm = model.language_model
    f = model.get_input_embeddings(ids, torch.from_numpy(pix), image_grid_thw=thw)
    cache = lm.make_cache()
    out = lm(ids, f.inputs_embeds, cache=cache, position_ids=f.position_ids, rope_deltas=f.rope_deltas, logits_to_keep=1)
    rows = [out.logits[0, -1].clone()]
    for y in forced:
        rows.append(lm(np.array([[int(y)]]), cache=cache).logits[0, -1].clone())
    cache[0]._seq.release()
    return torch.stack(rows)


def test_image_prefill_then_teacher_forced_decode_one_row(wide):
    cfg, W, model = wide
    ids, pix, thw, forced, ref = _image_request()
    got = _teacher_forced(model, ids, pix, thw, forced)
    assert got.shape == ref.shape == (1 + len(forced), 1024)
    worst = _check_rows(got, ref, TOL, "8192-wide B=1")
    print(f"8192-wide, image prefill + {len(forced)} forced steps: worst row rel-rms {worst:.4f}")


# ---- B rows of different context lengths: row b of every step width is the same sequence, so the oracle runs once per row
N_STEPS = 2
_LENS = [3 + (b * 7) % 20 for b in range(32)]
_LENS[1], _LENS[3] = 66, 63             # past a page boundary; the step that crosses it (slots 63 | 64)


def _prompt(b):
    rng = np.random.default_rng(7500 + b)
    return rng.integers(3, 1000, _LENS[b]).astype(np.int64), rng.integers(3, 1000, N_STEPS)


@functools.lru_cache(maxsize=None)
def _row_ref(b):
    cfg, W = _weights()
    p, f = _prompt(b)
    return oq.decode_teacher_forced(W, cfg, p[None], None, None, f)[1:]      # drop the prefill row


def _rows_vs_oracle(model, B, tag):
    """tests/test_full_depth_gpu.py::_rows_vs_oracle's method: prefill each prompt into its own cache, then every step feeds one
    token per row through ONE B-row decode forward; every row of every step vs the oracle's teacher-forced logits"""
    lm = model.language_model
    prompts = [_prompt(b) for b in range(B)]
    caches = []
    for p, _ in prompts:
        c = lm.make_cache()
        lm(p[None], cache=c, logits_to_keep=1)
        caches.append(c)
    got = []
    for s in range(N_STEPS):
        step = np.asarray([int(f[s]) for _, f in prompts], dtype=np.int64).reshape(B, 1)
        got.append(lm(step, cache=caches).logits[:, 0].clone())
    got = torch.stack(got)                                          # [steps, B, V]
    for c in caches:
        c[0]._seq.release()
    return max(_check_rows(got[:, b], _row_ref(b), TOL, f"{tag} row {b}") for b in range(B))


@pytest.mark.parametrize("B", [2, 4, 8, 9, 16, 32])
def test_rows_of_different_context_lengths_every_row_vs_oracle(wide, B):
    """2, 4 rows: RMSNorm | split-K GEMV (| rotary + KV write) on the dot-product kernels; 8, 9, 16 rows: the matrix-core forms
    (their norm prologue as one rows launch past one K segment); 32 rows: one wide step on the prefill GEMMs."""
    worst = _rows_vs_oracle(wide[2], B, f"8192-wide B={B}")
    print(f"8192-wide, {B}-row decode forward vs oracle: worst row rel-rms {worst:.4f}")


def test_one_row_over_a_4bit_language_model(wide):
    """the B = 1 case with the language model in MLX 4-bit (oracle/quant.quantize_checkpoint), against the oracle's 4-bit graph"""
    from oracle import quant as Q

    cfg, W, _ = wide
    ids, pix, thw, forced, _ = _image_request()
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    model = build_product_model(cfg, ck, kv_pool_tokens=4096, max_seqs=4)
    assert model.language_model.quantized
    ref = oq.decode_teacher_forced(ow, cfg, ids, torch.from_numpy(pix).to(BF), thw, forced)
    got = _teacher_forced(model, ids, pix, thw, forced)
    worst = _check_rows(got, ref, TOL, "8192-wide 4-bit B=1")
    print(f"8192-wide, 4-bit language model: worst row rel-rms {worst:.4f}")


def _centred(x):
    x = x.float().cpu()
    return x - x.mean(-1, keepdim=True)


def test_generate_step_over_the_8bit_kv_cache(wide):
    """generate_step(kv_bits=8, quantized_kv_start=0), 12 tokens.  Its rows are log-probs; the oracle is teacher-forced on the
    tokens the engine produced and compared as log-softmax rows with the row mean removed (a log-prob row carries a common
    offset of -log Z that would shrink any rel-rms): within 2e-2 of the quantised oracle, and nearer to it than to the bf16
    one (as tests/test_kv_quant_gpu.py)."""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = wide
    ids = np.random.default_rng(76).integers(3, 1000, (1, 40))
    out = [(int(t), lp.float().cpu()) for t, lp in generate_step(ids, model, None, None, max_tokens=12, temperature=0.0, kv_bits=8,
                                                                 quantized_kv_start=0)]
    assert model.language_model.pool.kpool8 is not None
    toks = [t for t, _ in out]
    got = torch.stack([lp for _, lp in out])
    fed = np.asarray(toks[:-1])
    ref_q = oq.decode_teacher_forced(W, cfg, ids, None, None, fed, kv_bits=8, kv_group_size=64, quantized_kv_start=0)
    ref_p = oq.decode_teacher_forced(W, cfg, ids, None, None, fed)
    lq, lp_ = torch.log_softmax(ref_q.float(), -1), torch.log_softmax(ref_p.float(), -1)
    errs = [_rel_rms(_centred(got[i]), _centred(lq[i])) for i in range(len(toks))]
    print("8192-wide kv_bits=8: row rel-rms " + " ".join(f"{e:.4f}" for e in errs))
    assert max(errs) < TOL, errs
    tail = range(2, len(toks))                                      # (row 0 is the prefill's: no quantised key yet)
    d_q = np.mean([_rel_rms(_centred(got[i]), _centred(lq[i])) for i in tail])
    d_p = np.mean([_rel_rms(_centred(got[i]), _centred(lp_[i])) for i in tail])
    print(f"    mean distance to the quantised oracle {d_q:.4f}, to the bf16 oracle {d_p:.4f}")
    assert d_q < d_p, (d_q, d_p)


def test_generate_step_captured_equals_eager(wide):
    """greedy generate_step on the captured step (hipGraph) and on the same launches enqueued step by step: equal tokens,
    bit-equal log-probs"""
    from mlx_vlm_amd.generate import generate_step

    cfg, W, model = wide
    ids = np.random.default_rng(77).integers(3, 1000, (1, 30))
    a = [(int(t), lp.float().cpu()) for t, lp in generate_step(ids, model, None, None, max_tokens=10, temperature=0.0)]
    b = [(int(t), lp.float().cpu()) for t, lp in generate_step(ids, model, None, None, max_tokens=10, temperature=0.0,
                                                               use_graph=False)]
    assert [t for t, _ in a] == [t for t, _ in b]
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert len(set(t for t, _ in a)) > 1


# ---- projections no single launch takes: the engine's slices of the weight rows and halves of the batch rows
def _one_layer(inter, vocab, seed):
    text = oq.TextCfg(hidden_size=8192, num_hidden_layers=1, intermediate_size=inter, num_attention_heads=64,
                      num_key_value_heads=8, vocab_size=vocab, tie_word_embeddings=False)
    cfg = oq.Cfg(text=text, vision=oq.VisionCfg(depth=1, embed_dim=160, hidden_size=8192, num_heads=2),
                 image_token_id=1001, video_token_id=1002, vision_start_token_id=1003)
    W = oq.random_weights(cfg, seed=seed, dtype=BF, std=0.02, fast=True)
    k = "language_model.model.embed_tokens.weight"
    W[k] = (W[k].float() * EMBED_GAIN).to(BF)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * BRANCH_GAIN).to(BF)
    return cfg, W


def _nine_rows(model, ref_of, tag, steps=N_STEPS):
    """9 rows (an odd count on the matrix-core widths; the engine's decode widths are 1, 2, 4, 8 and 9..64), every row of every
    step vs the oracle"""
    lm = model.language_model
    B = 9
    prompts = [_prompt(b) for b in range(B)]
    caches = []
    for p, _ in prompts:
        c = lm.make_cache()
        lm(p[None], cache=c, logits_to_keep=1)
        caches.append(c)
    got = torch.stack([lm(np.asarray([int(f[s]) for _, f in prompts], dtype=np.int64).reshape(B, 1), cache=caches).logits[:, 0].clone()
                       for s in range(steps)])
    for c in caches:
        c[0]._seq.release()
    return max(_check_rows(got[:, b], ref_of(prompts[b][0], prompts[b][1][:steps])[1:], TOL, f"{tag} row {b}") for b in range(B))


def test_gate_up_and_head_beyond_one_launch_run_as_slices_of_the_weight_rows():
    """intermediate 11008 (gate/up: 22016 weight rows) and vocabulary 22016 at 9 rows: 1376 row tiles x 3 K segments exceed the
    4096 units of the matrix-core workspace, so the engine cuts both projections at weight row 16384 (W, bias, y offsets; the
    SwiGLU output offset n0 / 2) - what a real 72B layer needs for gate/up (59136 rows) and the head (152064).  One layer."""
    cfg, W = _one_layer(11008, 22016, seed=76)
    model = build_product_model(cfg, W, kv_pool_tokens=4096, max_seqs=12)
    worst = _nine_rows(model, lambda p, f: oq.decode_teacher_forced(W, cfg, p[None], None, None, f), "sliced gate/up + head")
    print(f"8192-wide, sliced gate/up and head at 9 rows: worst row rel-rms {worst:.4f}")


def test_4bit_down_projection_no_kernel_takes_runs_as_halves_of_the_rows():
    """4-bit weights, intermediate 2112 (no multiple of 128: the matrix-core forms refuse that K, as they refuse the 72B's
    29568 in chunks of 256), 9 rows: the down projection runs as 4 + 5 -> 4 + (2 + 3) -> 4 + 2 + (1 + 2) rows on the 1 / 2 / 4-row
    kernels (x, residual and y row offsets; floor / ceil halves of an odd count), against the oracle's 4-bit graph.  One layer,
    one step."""
    from oracle import quant as Q

    cfg, W = _one_layer(2112, 1024, seed=77)
    ck, ow = Q.quantize_checkpoint(W, predicate=lambda p, v: p.startswith("language_model."))
    model = build_product_model(cfg, ck, kv_pool_tokens=4096, max_seqs=12)
    assert model.language_model.quantized
    worst = _nine_rows(model, lambda p, f: oq.decode_teacher_forced(ow, cfg, p[None], None, None, f), "halved 4-bit down", steps=1)
    print(f"8192-wide, 4-bit down projection in halves at 9 rows: worst row rel-rms {worst:.4f}")


def test_llm_create_refuses_a_wider_model_before_allocating():
    """the C entry itself (the Python constructor refuses first): hidden 8320 and 16384, and 4224 + 64 (no multiple of 128 above
    4096), return "unsupported shape" and leave the handle untouched; 8192 is taken"""
    import ctypes as C

    from mlx_vlm_amd import _lib

    L = _lib.lib()
    for hidden, want in ((8320, 2), (16384, 2), (4288, 2), (8192, 0)):
        cfg = _lib.LlmConfig(hidden, 1, 2048, hidden // 128, 8, 128, 1024, 1e-6, 16, 24, 0.0, 0.0, 0)
        h = C.c_void_p()
        assert L.vlm_llm_create(C.byref(cfg), C.byref(h)) == want, hidden
        if want:
            assert not h.value
        else:
            assert h.value and L.vlm_llm_destroy(h) == 0


# ---- SuScaledRoPE (two frequency tables, typed q / k scale) at hidden 8192: the long_from rule on every qkv route
def _su_model():
    from oracle import phi3_v as op

    short, long = op.su_factors(128, seed=9)
    cfg = op.Cfg(text=op.TextCfg(hidden_size=8192, num_hidden_layers=2, intermediate_size=2048, num_attention_heads=64,
                                 num_key_value_heads=8, vocab_size=1024, original_max_position_embeddings=64,
                                 short_factor=short, long_factor=long),
                 vision=op.VisionCfg(num_hidden_layers=1, intermediate_size=256))
    W = op.random_weights(cfg, seed=78, dtype=BF, std=0.02, embed_std=1.0, fast=True)
    for k in list(W):
        if k.endswith("o_proj.weight") or k.endswith("down_proj.weight"):
            W[k] = (W[k].float() * BRANCH_GAIN).to(BF)
    return cfg, W


@pytest.fixture(scope="module")
def su_wide():
    from tests.helpers import build_phi3v_model

    cfg, W = _su_model()
    return cfg, W, build_phi3v_model(cfg, W, kv_pool_tokens=8192, max_seqs=16)


@pytest.mark.parametrize("B", [1, 8])
def test_su_rope_regime_at_hidden_8192(su_wide, B):
    """tests/test_vlm_family_phi3v_gpu.py::test_su_rope_regime_of_a_batched_decode_step_follows_its_longest_row at hidden 8192
    (64 : 8 heads of 128, original_max_position_embeddings = 64 so that the crossing costs 60 tokens of context): B - 1 short
    rows and one row that runs from offset 61 across 64; from the step where ITS offset reaches 64 every row of the step rotates
    with the long factors.  B = 1: RMSNorm | split-K GEMV + bias | vlm_mrope_kvwrite_decode(long_from) (the composition of the
    narrow bf16 steps past 4096 columns); B = 8: the matrix-core qkv form at 8 rows (taken from K > 4096 on; 9..16 rows
    are the same kernel).  Every row of every step against oracle/phi3_v with the call-wide position_end, at that test's 2.5e-2; and
    the control: row 0 decoded alone stays short and must differ from its batched logits after the crossing."""
    from oracle import ops as O
    from oracle import phi3_v as op

    cfg, W, model = su_wide
    lm = model.language_model
    lim = cfg.text.original_max_position_embeddings
    rng = np.random.default_rng(920 + B)
    prompts = [rng.integers(3, 1000, 5 + 2 * r).astype(np.int64) for r in range(B - 1)] + [rng.integers(3, 1000, lim - 3).astype(np.int64)]
    n_steps = 6
    forced = rng.integers(3, 1000, (n_steps, B))
    caches, ocaches = [], []
    for p in prompts:
        c = lm.make_cache()
        lm(p[None], cache=c, logits_to_keep=1)
        caches.append(c)
        oc = [O.KVCache() for _ in range(cfg.text.num_hidden_layers)]
        op.language_model(W, cfg, op.embed_tokens(W, p[None]), oc, last_only=True)
        ocaches.append(oc)
    worst, crossed, row0 = 0.0, 0, []
    for s in range(n_steps):
        pe = max(len(p) + s for p in prompts) + 1                      # the call's position_end
        crossed += pe > lim
        got = lm(forced[s].reshape(B, 1), cache=caches).logits[:, 0]
        row0.append(got[0].float().cpu())
        for r in range(B):
            ref = op.language_model(W, cfg, op.embed_tokens(W, np.array([[int(forced[s, r])]])), ocaches[r], position_end=pe)[0, 0]
            e = _rel_rms(got[r], ref)
            worst = max(worst, e)
            assert e < 2.5e-2, (s, r, pe, e)
    assert 0 < crossed < n_steps                                        # steps on both sides of the limit
    for c in caches:
        c[0]._seq.release()
    if B > 1:
        c0 = lm.make_cache()
        lm(prompts[0][None], cache=c0, logits_to_keep=1)
        alone = [lm(np.array([[int(forced[s, 0])]]), cache=c0).logits[0, 0].float().cpu() for s in range(n_steps)]
        c0[0]._seq.release()
        first_long = n_steps - crossed
        assert _rel_rms(alone[first_long - 1], row0[first_long - 1]) < 2.5e-2      # before: the same computation
        assert _rel_rms(alone[n_steps - 1], row0[n_steps - 1]) > 5e-2               # after: another rope regime
    print(f"Su-RoPE regime at hidden 8192, B={B}: worst row rel-rms {worst:.4f}, {crossed} long steps of {n_steps}")
