"""Per-row samplers on MI355X: the row-table mode of vlm_sample_ex (ops.sample_rows), the VLM_DECODE_ROW_SAMPLER step of the
engine and `BatchGenerator.insert(..., samplers=)`.

The yardstick is the scalar sampler itself (pinned to the reference's survivor sets by tests/test_sampler_exact_*.py): row b of a
row-table call gives the token, the log-prob row and the filtered row of `ops.sample` on that row alone with the row's scalars
and step = the row's count - bit for bit, no tolerance.  Shapes: V = 8192 takes the split chain, V = 1000 the one-workgroup
filter (a multiple of 8 below the split's 8192), V = 8195 the unaligned tail."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location("make_golden_row_sampler_parent",
                                               os.path.join(HERE, "golden", "make_golden_row_sampler_parent.py"))
parent = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(parent)


def _samplers():
    from mlx_vlm_amd.sample_utils import make_sampler

    return [make_sampler(),                                                       # greedy
            make_sampler(temp=0.9, seed=101),                                     # temperature only
            make_sampler(temp=1.0, top_p=0.9, seed=202),
            make_sampler(temp=1.1, min_p=0.05, top_k=40, seed=303),
            make_sampler(temp=0.7, top_p=0.9, min_p=0.05, top_k=40, seed=404),
            make_sampler(temp=1.0, top_k=1, seed=505)]


COUNTS = [3, 0, 2_000_000_000, 1, 77, 12345]


def _logits(B, V, seed=5):
    """seeded bf16 rows with a realistic spread (tests/test_sampler_gpu.py::_rows); row 2 holds exact ties"""
    g = torch.Generator().manual_seed(seed)
    scales = (1.5, 5.0, 2.0)
    x = torch.randn(B, V, generator=g) * torch.tensor([[scales[b % 3]] for b in range(B)])
    x[2] = torch.round(x[2] * 2) / 2
    return x.to(BF).to(DEV)


def _table(samplers, counts):
    return torch.from_numpy(np.stack([s.row_line(c) for s, c in zip(samplers, counts)])).to(DEV)


def _scalar(ops, row, smp, count):
    """today's call on one row: (token, log-prob row, filtered row or None when the sampler has no filter)"""
    step = torch.tensor([count], dtype=torch.int32, device=DEV)
    tok, lp, filt = ops.sample(row, step=step, want_logprobs=True, return_filtered=True, **smp.sample_args())
    has_filter = smp.temp > 0 and (0 < smp.top_p < 1 or smp.min_p != 0 or smp.top_k > 0)
    return int(tok[0]), lp[0], (filt[0] if has_filter else None)


@pytest.mark.parametrize("V", [8192, 1000, 8195])
def test_row_equals_the_scalar_call(V):
    from mlx_vlm_amd import ops

    smps = _samplers()
    B = len(smps)
    logits = _logits(B, V)
    table = _table(smps, COUNTS)
    before = table.clone()
    tok, lp, filt = ops.sample_rows(logits, table, return_filtered=True)
    torch.cuda.synchronize()
    for b, (smp, c) in enumerate(zip(smps, COUNTS)):
        t1, lp1, f1 = _scalar(ops, logits[b:b + 1], smp, c)
        assert int(tok[b]) == t1, (V, b, int(tok[b]), t1)
        assert torch.equal(lp[b].view(torch.int16), lp1.view(torch.int16)), (V, b)
        if f1 is not None:
            assert torch.equal(filt[b].view(torch.int16), f1.view(torch.int16)), (V, b)
            assert int(torch.isfinite(f1.float()).sum()) < V           # (the filter did remove something)
    # the call advanced every row's count by exactly one and touched nothing else of the lines
    want = before.clone()
    want[:, 5] += 1
    assert torch.equal(table, want)
    # ... log-probs in: the same tokens from the rows' log-probs
    tok2, _ = ops.sample_rows(lp, before.clone(), input_is_logprobs=True)
    assert torch.equal(tok2, tok)


@pytest.mark.parametrize("V", [8192, 1000])
def test_a_rows_draw_depends_on_its_line_alone(V):
    """the (logits row, sampler, count) pairs in another row order, beside other neighbours: every pair keeps its token.  The
    scalar path keys its noise on the row index: there this fails."""
    from mlx_vlm_amd import ops
    from mlx_vlm_amd.sample_utils import make_sampler

    smps = _samplers()
    B = len(smps)
    logits = _logits(B, V)
    base, _ = ops.sample_rows(logits, _table(smps, COUNTS))
    perm = [4, 2, 5, 0, 3, 1]
    tok_p, _ = ops.sample_rows(logits[perm].contiguous(), _table([smps[i] for i in perm], [COUNTS[i] for i in perm]))
    assert tok_p.tolist() == [int(base[i]) for i in perm]
    # pair 4 in row 0, every neighbour another sampler
    other = [smps[4]] + [make_sampler(temp=1.3, top_k=7, seed=900 + i) for i in range(B - 1)]
    rows = [4, 0, 1, 2, 3, 5]
    tok_n, _ = ops.sample_rows(logits[rows].contiguous(), _table(other, [COUNTS[4]] + [9] * (B - 1)))
    assert int(tok_n[0]) == int(base[4])
    # the noise does decide these draws: the scalar call on the same row at rows 0 and 1 of a batch differs somewhere
    st = torch.tensor([COUNTS[1]], dtype=torch.int32, device=DEV)
    two = logits[[1, 1]].contiguous()
    differs = False
    for seed in range(8):
        t, _ = ops.sample(two, step=st, temperature=0.9, seed=seed)
        differs = differs or int(t[0]) != int(t[1])
    assert differs


def test_captured_call_replays_over_any_table():
    """one capture at B = 4, V = 8192; the lines are rewritten between replays (all greedy, mixed, all sampled): the launches
    do not depend on them, every replay equals the eager call with the same table"""
    from mlx_vlm_amd import ops

    smps = _samplers()
    B, V = 4, 8192
    logits = _logits(B, V, seed=9)
    ws = ops.sample_workspace(B, DEV)
    lines = ops.sample_row_table(ws)
    ops.sample_rows(logits, ws=ws)                     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tok, lp, filt = ops.sample_rows(logits, ws=ws, return_filtered=True)
    tables = [[smps[0]] * 4, [smps[0], smps[4], smps[1], smps[3]], [smps[2], smps[4], smps[5], smps[3]]]
    for i, row_smps in enumerate(tables):
        table = _table(row_smps, [5 * i + r for r in range(B)])
        lines[:B].copy_(table)
        graph.replay()
        torch.cuda.synchronize()
        tok_e, lp_e, filt_e = ops.sample_rows(logits, table.clone(), return_filtered=True)
        assert torch.equal(tok, tok_e), (i, tok.tolist(), tok_e.tolist())
        assert torch.equal(lp.view(torch.int16), lp_e.view(torch.int16))
        assert torch.equal(filt.view(torch.int16), filt_e.view(torch.int16))
        assert lines[:B, 5].tolist() == [5 * i + r + 1 for r in range(B)]
    assert tok.tolist() != [int(torch.argmax(lp[b].float())) for b in range(B)]      # (the last table did sample)


def test_extended_filters_are_refused_in_row_table_mode():
    import ctypes as C

    from mlx_vlm_amd import _lib, ops

    logits = _logits(3, 1000)
    ws = ops.sample_workspace(3, DEV)
    tok = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    lp, sc = torch.empty(3, 1000, dtype=BF, device=DEV), torch.empty(3, 1000, dtype=BF, device=DEV)
    for kw in (dict(xtc_probability=0.5), dict(typical_p=0.5), dict(top_n_sigma=1.0), dict(p_less=1)):
        sp = _lib.SamplerParams(input_is_logprobs=_lib.SAMPLE_MODE_ROW_TABLE, **{"typical_p": 1.0, **kw})
        rc = _lib.lib().vlm_sample_ex(logits.data_ptr(), 1000, 3, 1000, lp.data_ptr(), sc.data_ptr(), 1000, tok.data_ptr(),
                                      ws.data_ptr(), C.byref(sp), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0, kw
    torch.cuda.synchronize()
    assert tok.tolist() == [-7] * 3


# ------------------------------------------------------------------------------------------ engine step, generator
@pytest.fixture(scope="module")
def tiny():
    return parent.tiny_model()


def _joined(model, B, smps):
    """a generator whose B requests have joined rows 0..B-1 of its decode state (nothing stepped yet)"""
    from mlx_vlm_amd.batch import BatchGenerator

    gen = BatchGenerator(model, None, max_tokens=16, completion_batch_size=B, prefill_batch_size=B, async_prefill=False)
    ids = [np.random.default_rng(40 + i).integers(3, 1000, 4 + (i % 5)) for i in range(B)]
    gen.insert(ids, 16, samplers=smps)
    gen._admit_begin()
    gen._admit_join()
    assert len(gen._rows) == B
    return gen, [len(i) for i in ids]


@pytest.mark.parametrize("B", [1, 4, 8, 13, 20])
def test_engine_step_equals_forward_then_sample_rows(tiny, B):
    """VLM_DECODE_ROW_SAMPLER at widths 1 / 4 / 8 (v_dot2c), 13 (skinny-M MFMA) and 20 (wide): six captured steps give the tokens
    of forward + ops.sample_rows + advance run eagerly on the same state; counts, ctx and pos advance by one per step"""
    import ctypes as C

    from mlx_vlm_amd import _lib, ops

    _, model = tiny
    lm = model.language_model
    pool = _samplers()
    smps = [pool[(i + 1) % len(pool)] for i in range(B)]
    STEPS = 6
    runs = []
    for captured in (True, False):
        gen, lens = _joined(model, B, smps)
        st = gen._st
        first = st.tok[:B].clone()
        toks = []
        for _ in range(STEPS):
            if captured:
                lm.decode_step_rows(st, B, gen._table, {}, use_graph=True, row_sampler=True)
            else:
                lm.decode_forward_rows(st, B, gen._table)
                tok, lp = ops.sample_rows(st.logits[:B], ws=st.sample_ws)
                st.tok[:B].copy_(tok)
                lm.decode_advance_rows(st, B)
            toks.append(st.tok[:B].clone())
        torch.cuda.synchronize()
        lines = ops.sample_row_table(st.sample_ws)
        assert lines[:B, 5].tolist() == [1 + STEPS] * B
        want = [n + STEPS for n in sorted(lens)]        # (the queue admits the shortest prompt first)
        assert st.ctx[:B].tolist() == want and st.pos[:B].tolist() == want
        if captured and B == 1:
            # the flag beside VLM_DECODE_WINDOW: an argument error, and nothing of the state moves
            args = st.args(B=1, flags=_lib.DECODE_ROW_SAMPLER | _lib.DECODE_WINDOW)
            keep = [t.clone() for t in (st.tok, st.ctx, st.pos, st.step)]
            rc = _lib.lib().vlm_llm_decode_step(lm._handle, C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert rc != 0
            assert all(torch.equal(a, b) for a, b in zip(keep, (st.tok, st.ctx, st.pos, st.step)))
            assert lines[:1, 5].tolist() == [1 + STEPS]
        for row in gen._rows:                          # (the steps above went past the scheduler: its mirror of the offsets follows)
            row.seq.offset += STEPS
        gen.close()
        runs.append((first, torch.stack(toks)))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]), (runs[0][1].tolist(), runs[1][1].tolist())


@pytest.mark.parametrize("B", [1, 8])
def test_engine_step_with_the_fused_tail(tiny, B):
    """VLM_DECODE_ROW_SAMPLER | VLM_DECODE_FUSED_TAIL: the sampler's last launch also advances ctx / pos / step / counts and
    gathers the next step's embedding rows - the tokens of the step with the advance as a launch of its own"""
    import ctypes as C

    from mlx_vlm_amd import _lib, ops

    _, model = tiny
    lm = model.language_model
    pool = _samplers()
    smps = [pool[(i + 1) % len(pool)] for i in range(B)]
    STEPS = 6
    runs = []
    for fused in (False, True):
        gen, lens = _joined(model, B, smps)
        st = gen._st
        toks = []
        if fused:
            kp = lm.pool
            kv = _lib.KvPool(kp.kpool.data_ptr(), kp.vpool.data_ptr(), kp.layer_stride, gen._table.data_ptr(), kp.max_pages,
                             None, None, None, None, 0)
            assert _lib.lib().vlm_llm_set_kv(lm._handle, C.byref(kv)) == 0
            ops.embed_gather(st.tok[:B], lm._w["embed"], out=st.h[:B])          # the flag's promise: h == embed[tok] at entry
            args = st.args(B=B, with_logprobs=True, flags=_lib.DECODE_ROW_SAMPLER | _lib.DECODE_FUSED_TAIL)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(STEPS):
            if fused:
                assert _lib.lib().vlm_llm_decode_step(lm._handle, C.byref(args), stream) == 0
            else:
                lm.decode_step_rows(st, B, gen._table, {}, use_graph=False, row_sampler=True)
            toks.append(st.tok[:B].clone())
        torch.cuda.synchronize()
        want = [n + STEPS for n in sorted(lens)]
        assert st.ctx[:B].tolist() == want and st.pos[:B].tolist() == want
        assert ops.sample_row_table(st.sample_ws)[:B, 5].tolist() == [1 + STEPS] * B
        if fused:
            assert torch.equal(st.h[:B], lm._w["embed"][st.tok[:B].long()])
        for row in gen._rows:
            row.seq.offset += STEPS
        gen.close()
        runs.append(torch.stack(toks))
    assert torch.equal(runs[0], runs[1]), (runs[0].tolist(), runs[1].tolist())


def _gen_samplers():
    from mlx_vlm_amd.sample_utils import make_sampler

    return [make_sampler(),                              # greedy, named
            make_sampler(temp=0.9, seed=11),
            None,                                        # the generator's default: greedy
            make_sampler(temp=1.0, top_p=0.9, seed=22),
            make_sampler(temp=0.8, top_p=0.95, min_p=0.02, top_k=50, seed=33),
            make_sampler(temp=1.2, top_k=5, seed=44),
            make_sampler(temp=1.0, min_p=0.1, seed=55)]


def test_batch_generator_per_request_samplers(tiny):
    """7 requests of different lengths, 3 .. 12 tokens each, 4 rows: rows leave and others join mid-run.  Captured and
    uncaptured steps agree on every token and token_logprob; the greedy requests get the tokens of a plain greedy generator
    of the same width schedule (same kernels, same log-prob rows)."""
    from mlx_vlm_amd.batch import BatchGenerator
    from mlx_vlm_amd.sample_utils import make_sampler

    _, model = tiny
    smps = _gen_samplers()
    tok_g, lp_g, _ = parent.run(model, samplers=smps, use_graph=True)
    tok_e, lp_e, _ = parent.run(model, samplers=smps, use_graph=False)
    assert tok_g == tok_e
    assert lp_g == lp_e

    class EagerSteps(BatchGenerator):                    # the route Python callables force: forward, ops.sample_rows, advance
        def _decode_rows(self, width):
            return self._decode_rows_eager(width)

    tok_h, lp_h, _ = parent.run(model, samplers=smps, gen_cls=EagerSteps)
    assert tok_h == tok_g and lp_h == lp_g
    plain, _, _ = parent.run(model)
    for i in (0, 2):
        assert tok_g[i] == plain[i], i
    assert any(tok_g[i] != plain[i] for i in (1, 3, 4, 5, 6))          # (the others were sampled)

    gen = BatchGenerator(model, None, max_tokens=4, completion_batch_size=4)
    try:
        ids = parent.prompts(2)
        with pytest.raises(ValueError):
            gen.insert(ids, 4, samplers=[make_sampler()])
        with pytest.raises(NotImplementedError, match="top_p, min_p .* top_k"):
            gen.insert(ids, 4, samplers=[make_sampler(temp=1.0, typical_p=0.5), None])
        with pytest.raises(NotImplementedError, match="top_p, min_p .* top_k"):
            gen.insert(ids, 4, samplers=[None, lambda lp: lp.argmax(-1)])
        assert not gen.unprocessed_prompts and not gen._row_sampling
    finally:
        gen.close()


def test_generator_without_samplers_is_the_parents(tiny):
    """the tokens and the launches per step recorded from the commit before per-request samplers existed"""
    _, model = tiny
    want = json.load(open(os.path.join(HERE, "golden", "row_sampler_parent_tokens.json")))
    got = parent.workload(model)
    for name in ("sampled", "greedy"):
        assert got[name]["tokens"] == want[name]["tokens"], name
        assert got[name]["launches"] == want[name]["launches"], name
