"""Constrained decoding without a GPU: `mlx_vlm_amd/structured.py` against a stub llguidance, the scheduler's part of the
mask protocol on the mock engine of tests/test_batch_scheduler_cpu.py, and the frozen C ABI the mask travels through.

The device half - the bitmask kernel, the sampler over masked rows, the captured steps - is tests/test_token_mask_gpu.py."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from mlx_vlm_amd import structured as ST
from mlx_vlm_amd.models.qwen2_vl.language import DecodeState
from tests.test_batch_scheduler_cpu import V, MockEngineGenerator, make_pool, stream_alone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MW = (V + 31) // 32


def pack(allowed_tokens, words):
    out = np.zeros(words, dtype=np.uint32)
    for t in allowed_tokens:
        out[t >> 5] |= np.uint32(1 << (t & 31))
    return out.view(np.int32)


def unpack(words, vocab):
    w = np.asarray(words).reshape(-1).view(np.uint32)
    t = np.arange(vocab)
    ok = (t >> 5) < len(w)
    bit = np.zeros(vocab, dtype=bool)
    bit[ok] = (w[t[ok] >> 5] >> (t[ok] & 31).astype(np.uint32)) & 1 == 1
    return bit


# ------------------------------------------------------------------------------------------ structured.py on a stub llguidance
class _StubMatcher:
    """allows {consumed tokens so far} + {7}; token 666 is a grammar error"""
    made = []

    def __init__(self, tokenizer, grammar):
        self.tokenizer, self.grammar, self.consumed, self.error = tokenizer, grammar, [], ""
        _StubMatcher.made.append(self)

    def consume_token(self, t):
        self.consumed.append(int(t))
        if t == 666:
            self.error = "token 666 is not in the grammar"

    def get_error(self):
        return self.error


def _stub_fill(matcher, bitmask, row):
    assert bitmask.dtype == np.int32 and bitmask.ndim == 2
    bitmask[row] = pack([7] + matcher.consumed, bitmask.shape[1])


@pytest.fixture
def llg(monkeypatch):
    _StubMatcher.made = []
    root = types.ModuleType("llguidance")
    root.LLMatcher = _StubMatcher
    root.grammar_from = lambda kind, text: f"{kind}:{text}"
    npmod = types.ModuleType("llguidance.numpy")
    npmod.fill_next_token_bitmask = _stub_fill
    hf = types.ModuleType("llguidance.hf")
    hf.from_tokenizer = lambda tok: types.SimpleNamespace(vocab_size=tok.vocab_size, of=tok)
    root.numpy, root.hf = npmod, hf
    for name, mod in (("llguidance", root), ("llguidance.numpy", npmod), ("llguidance.hf", hf)):
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.setattr(ST, "_llg_tokenizer_cache", {})
    # the device call of the plain-callable route, restated on CPU tensors (the kernel itself: tests/test_token_mask_gpu.py)
    monkeypatch.setattr(ST, "_apply_mask", lambda logits, words: logits.masked_fill(
        ~torch.from_numpy(np.stack([unpack(w, logits.shape[-1]) for w in np.asarray(words)])), float("-inf")))
    return root


class _Tok:
    vocab_size = 100

    def encode(self, text, add_special_tokens=False):
        return {"<think>": [1, 50], "</think>": [51]}[text]


def test_llguidance_processor_sets_up_once_then_consumes(llg):
    tok = _Tok()
    proc = ST.build_json_schema_logits_processor(tok, {"type": "object"})
    assert isinstance(proc, ST.LLGuidanceLogitsProcessor) and ST.is_mask_processor(proc)
    assert proc.grammar == 'json_schema:{"type": "object"}' and proc.llg_tokenizer.of is tok
    assert ST.build_json_schema_logits_processor(tok, "x").llg_tokenizer is proc.llg_tokenizer      # one llg tokenizer per tokenizer
    assert proc.requires_immediate_decode_yield and proc.is_first_token and not _StubMatcher.made
    w0 = proc.prepare_next_token_mask(12)                     # the first call: set-up, nothing consumed
    assert w0.dtype == np.int32 and w0.shape == (1, 4) and len(_StubMatcher.made) == 1 and _StubMatcher.made[0].consumed == []
    assert unpack(w0, 100).nonzero()[0].tolist() == [7]
    w1 = proc.prepare_next_token_mask(33)
    assert _StubMatcher.made[0].consumed == [33] and unpack(w1, 100).nonzero()[0].tolist() == [7, 33]
    assert unpack(w0, 100).nonzero()[0].tolist() == [7]       # the words of the step before are still what they were
    with pytest.raises(ValueError, match="LLGuidance matcher error: token 666"):
        proc.prepare_next_token_mask(666)
    twin = proc.clone()
    assert twin is not proc and twin.is_first_token and twin.grammar == proc.grammar and twin.llg_tokenizer is proc.llg_tokenizer
    proc.reset()
    assert proc.is_first_token and proc.ll_matchers is None
    proc.prepare_next_token_mask(5)
    assert len(_StubMatcher.made) == 2 and _StubMatcher.made[1].consumed == []


def test_llguidance_processor_as_a_plain_callable(llg):
    proc = ST.LLGuidanceLogitsProcessor("g", types.SimpleNamespace(vocab_size=100))
    logits = torch.arange(200, dtype=torch.float32).reshape(2, 100)
    ids = torch.tensor([[3, 4], [5, 6]])
    out = proc(ids, logits)                                   # a batch: one matcher per row, nothing consumed at the first call
    assert len(_StubMatcher.made) == 2 and torch.isfinite(out).nonzero().tolist() == [[0, 7], [1, 7]]
    out = proc(torch.tensor([[3, 4, 9], [5, 6, 11]]), logits)
    assert [m.consumed for m in _StubMatcher.made] == [[9], [11]]
    assert torch.isfinite(out).nonzero().tolist() == [[0, 7], [0, 9], [1, 7], [1, 11]]
    assert torch.equal(logits, torch.arange(200, dtype=torch.float32).reshape(2, 100))      # the caller's logits are not edited
    one = ST.LLGuidanceLogitsProcessor("g", types.SimpleNamespace(vocab_size=100))
    row = one.process_last_token(1, logits[0])                # [V] in, [V] out
    assert row.shape == (100,) and torch.isfinite(row).nonzero().reshape(-1).tolist() == [7]
    row = one.process_last_token(21, logits[:1])
    assert row.shape == (1, 100) and torch.isfinite(row).nonzero()[:, 1].tolist() == [7, 21]


def test_thinking_aware_processor_waits_for_the_end_of_thinking(llg):
    inner = ST.LLGuidanceLogitsProcessor("g", types.SimpleNamespace(vocab_size=100))
    proc = ST.ThinkingAwareLogitsProcessor(inner, _Tok(), enable_thinking=True)
    assert (proc.thinking_start_token_id, proc.thinking_end_token_id) == (50, 51) and ST.is_mask_processor(proc)
    assert proc.requires_immediate_decode_yield
    for t in (50, 3, 4):
        assert proc.prepare_next_token_mask(t) is None        # thinking is open: no constraint, the matcher does not exist yet
    assert not _StubMatcher.made
    w = proc.prepare_next_token_mask(51)                      # </think>: the next token is the first of the answer
    assert unpack(w, 100).nonzero()[0].tolist() == [7] and _StubMatcher.made[0].consumed == []
    w = proc.prepare_next_token_mask(7)
    assert _StubMatcher.made[0].consumed == [7]
    logits = torch.zeros(1, 100)
    twin = proc.clone()
    assert twin.processor is not inner and twin.enable_thinking and twin.prepare_next_token_mask(9) is None
    assert twin.process_last_token(3, logits) is logits and twin(torch.tensor([3, 4]), logits) is logits
    assert torch.isfinite(twin.process_last_token(51, logits)).sum() == 1
    proc.reset()
    assert inner.is_first_token and proc.prepare_next_token_mask(7) is None
    now = ST.ThinkingAwareLogitsProcessor(inner.clone(), _Tok(), enable_thinking=False)
    assert now.prepare_next_token_mask(3) is not None          # no thinking: active from the first token
    # a wrapper around a plain callable does not speak the mask protocol
    assert not ST.is_mask_processor(ST.ThinkingAwareLogitsProcessor(lambda ids, logits: logits, _Tok()))


def test_without_llguidance_the_builder_raises_the_references_import_error(monkeypatch):
    monkeypatch.setitem(sys.modules, "llguidance", None)
    with pytest.raises(ImportError, match="llguidance is required for structured response_format generation"):
        ST.build_json_schema_logits_processor(_Tok(), {"type": "object"})


def test_mask_word_helpers():
    w = pack([0, 31, 32, 99], 4)
    assert ST.mask_words_of(w[None]).tolist() == w.tolist() and ST.mask_words_of(w.view(np.uint32), 2).tolist() == w[:2].tolist()
    assert ST.mask_words_of(torch.from_numpy(w)).dtype == np.int32
    with pytest.raises(TypeError):
        ST.mask_words_of(np.zeros(4, dtype=np.int64))
    assert ST.mask_allows_any(w, 100) and ST.mask_allows_any(w, 32) and not ST.mask_allows_any(pack([99], 4), 99)
    assert ST.mask_allows_any(pack([98], 4), 99) and not ST.mask_allows_any(pack([40], 4), 32) and not ST.mask_allows_any(w[:0], 100)
    # the tables: the words sit at the END of the row's bias_idx entries, their count in slot 7, the bias list in front
    from mlx_vlm_amd.sample_utils import make_logits_processors
    spec = make_logits_processors(logit_bias={3: 1.0, 9: -2.0}, repetition_penalty=1.5)
    params, bidx, bval = DecodeState.pack_row_penalties([spec, None, None], 64, 4, [w[:3], None, w])
    S = DecodeState.MAX_ROW_BIAS + 4
    assert params.shape == (3, 8) and bidx.shape == bval.shape == (3, S)
    assert params[:, 7].tolist() == [3, 0, 4] and params[:, 6].tolist() == [2, 0, 0] and params[0, 0] == 1.5
    assert bidx[0, :2].tolist() == [3, 9] and bidx[0, S - 3:].tolist() == w[:3].tolist() and bidx[2, S - 4:].tolist() == w.tolist()
    assert not bidx[1].any() and not bidx[0, 2:S - 3].any()
    old = DecodeState.pack_row_penalties([spec], 64)          # callers without masks: today's widths, zero in slot 7
    assert old[1].shape == (1, DecodeState.MAX_ROW_BIAS) and old[0][0, 7] == 0


# ------------------------------------------------------------------------------------------ the scheduler on the mock engine
class StandIn:
    """A stand-in matcher: at every step a seeded set of about 30 allowed tokens that depends on the step index and on the
    token it was last handed; `fed` is every token it consumed.  short: masks of MW - 5 words."""

    def __init__(self, seed, short=False):
        self.seed, self.short, self.is_first_token, self.step, self.fed, self.words = seed, short, True, 0, [], None

    def prepare_next_token_mask(self, last_token):
        if not self.is_first_token:
            self.fed.append(int(last_token))
        key = 0 if self.is_first_token else int(last_token) + 1
        self.is_first_token = False
        n = MW - 5 if self.short else MW
        rng = np.random.default_rng([self.seed, self.step, key])
        self.words = pack(rng.integers(0, min(V, 32 * n), 30).tolist(), n)
        self.step += 1
        return self.words[None]

    def __call__(self, tokens, logits):
        raise AssertionError("a mask processor is never handed the logits")


class _SpyEvent:
    def __init__(self):
        self.synced = False

    def record(self, *a):
        pass

    def query(self):
        return True

    def synchronize(self):
        self.synced = True


class MaskMock(MockEngineGenerator):
    """the mock engine + the state's per-row tables on the host: `_decode_rows` checks, at every step, that each live row's
    slot 7 and words are what its own processor last returned, and records whether the step waited for its tokens first"""

    def __init__(self, pool, **kw):
        self.waited = []           # per step: (the step's event was synchronised before the launch, a mask row was live)
        super().__init__(pool, **kw)

    def _event(self):
        self._last_event = _SpyEvent()
        return self._last_event

    def _vocab_size(self):
        return V

    def _new_decode_state(self, cap):
        st = super()._new_decode_state(cap)
        S = DecodeState.MAX_ROW_BIAS + MW
        st.hist, st.hist_len = torch.zeros(cap, 8, dtype=torch.int32), torch.zeros(cap, dtype=torch.int32)
        st.row_params = torch.zeros(cap, 8)
        st.row_bias_idx, st.row_bias_val = torch.zeros(cap, S, dtype=torch.int32), torch.zeros(cap, S)
        st.row_penalty_tables = lambda: None
        return st

    def _prefill_requests(self, batch):
        from mlx_vlm_amd.batch import _MASKPROC_KEY, _PROCS_KEY

        out = super()._prefill_requests(batch)
        masks = self._first_masks(batch)
        self.first_masks = getattr(self, "first_masks", {})
        self.first_masks.update({b[0]: m for b, m in zip(batch, masks)})
        specs = [b[3].get(_PROCS_KEY) for b in batch]
        if any(specs) or any(b[3].get(_MASKPROC_KEY) is not None for b in batch):
            n = len(batch)
            params, bidx, bval = DecodeState.pack_row_penalties(specs, 8, MW, masks)
            self._last_pen = (torch.zeros(n, 8, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), torch.from_numpy(params),
                              torch.from_numpy(bidx), torch.from_numpy(bval))
        return out

    def _decode_rows(self, width):
        st, live = self._st, len(self._rows)
        mask_live = any(row.mask_proc is not None for row in self._rows)
        self.waited.append((self._last_event.synced, mask_live))
        for r, row in enumerate(self._rows):
            W = int(st.row_params[r, 7])
            if row.mask_proc is None or (row.mask_proc.words is None):
                assert W == 0, (r, row.uid, W)
            elif mask_live and row.mask_w == 0:                 # its token ends the request: this step's output is dropped
                assert W == 0 and row.num_tokens + 1 >= row.max_tokens
            else:
                want = row.mask_proc.words
                assert W == len(want) and st.row_bias_idx[r, st.row_bias_idx.shape[1] - W:].numpy().tolist() == want.tolist(), (r, row.uid)
            assert float(st.row_params[r, 0]) == (row.procs.repetition_penalty if row.procs else 0.0)
        assert not st.row_params[live:, 7].any()
        super()._decode_rows(width)


def _drain(gen):
    got = {}
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            got.setdefault(r.uid, []).append(r.token)
    return got


def test_mask_rows_keep_their_words_through_compaction_and_disable_the_pipelining():
    from mlx_vlm_amd.sample_utils import make_logits_processors

    gen = MaskMock(make_pool(), completion_batch_size=4, prefill_batch_size=4, async_prefill=False)
    prompts = [np.arange(3 + i) + 5 for i in range(7)]
    lens = [3, 9, 4, 7, 5, 6, 8]
    procs = [StandIn(1), None, [StandIn(3, short=True), make_logits_processors(repetition_penalty=1.25)], None, StandIn(5), None, None]
    uids = gen.insert(prompts, lens, logits_processors=procs)
    got = _drain(gen)
    for u, p, m, pr in zip(uids, prompts, lens, procs):
        want = stream_alone(p, m)
        assert got[u] == want                                 # (the mock engine's tokens do not depend on the masks)
        pr = pr[0] if isinstance(pr, list) else pr
        if pr is not None:
            # the matcher saw the first-token call and then every token that was fed back, in order - not the last one
            assert pr.fed == want[:-1] and pr.step == m, (u, pr.fed, want)
            assert gen.first_masks[u] is not None
    # rows moved into holes and rows re-used by later requests happened, with and without masks
    assert len(gen.decode_widths) > 9 and {w for w, _ in gen.decode_widths} >= {1, 2, 4}
    # a step waits for its tokens on the host exactly while a mask row is live; the steps after run one ahead again
    assert all(synced == live for synced, live in gen.waited)
    flags = [live for _, live in gen.waited]
    assert True in flags and False in flags and flags.index(False) > flags.index(True)
    assert gen._unpipelined_steps == sum(flags)
    assert set(vars(gen.stats())) >= {"prompt_tokens", "prompt_tps", "generation_tokens", "generation_tps", "peak_memory"}
    gen.close()


def test_free_rows_alone_stay_pipelined_and_tables_untouched():
    gen = MaskMock(make_pool(), completion_batch_size=2, prefill_batch_size=2, async_prefill=False)
    uids = gen.insert([np.arange(4) + 5, np.arange(6) + 5], [5, 4])
    got = _drain(gen)
    assert [len(got[u]) for u in uids] == [5, 4] and gen._unpipelined_steps == 0 and not any(s for s, _ in gen.waited)
    assert getattr(gen, "_pin_mask", None) is None and not gen._st.row_params.any()
    gen.close()


def test_an_all_zero_mask_is_refused_on_the_host_naming_the_request():
    class Dead(StandIn):
        def prepare_next_token_mask(self, last_token):
            super().prepare_next_token_mask(last_token)
            if self.step == 3:
                return np.zeros((1, MW), dtype=np.int32)
            return self.words[None]

    gen = MaskMock(make_pool(), completion_batch_size=2, prefill_batch_size=2, async_prefill=False)
    uids = gen.insert([np.arange(4) + 5, np.arange(6) + 5], [9, 9], logits_processors=[None, Dead(2)])
    with pytest.raises(ValueError, match=f"request {uids[1]}: .*allows no token"):
        _drain(gen)
    gen.close()
    # ... at the first token too, and bits past the vocabulary do not count
    gen = MaskMock(make_pool(), completion_batch_size=2, prefill_batch_size=2, async_prefill=False)
    first = types.SimpleNamespace(prepare_next_token_mask=lambda t: pack([V, V + 3], MW)[None])
    (uid,) = gen.insert([np.arange(4) + 5], [3], logits_processors=[first])
    with pytest.raises(ValueError, match=f"request {uid}: "):
        gen.next()
    gen.close()


def test_two_mask_processors_on_one_request_are_refused():
    gen = MaskMock(make_pool(), completion_batch_size=2, prefill_batch_size=2, async_prefill=False)
    with pytest.raises(NotImplementedError, match="one mask processor"):
        gen.insert([np.arange(4) + 5], [3], logits_processors=[[StandIn(1), StandIn(2)]])
    assert not gen.has_work
    gen.close()


# ------------------------------------------------------------------------------------------ the frozen C ABI
def test_the_mask_travels_through_the_frozen_abi():
    from mlx_vlm_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    src = "".join(open(os.path.join(ROOT, "mlx-vlm_amd", "csrc", f)).read()
                  for f in sorted(os.listdir(os.path.join(ROOT, "mlx-vlm_amd", "csrc"))) if f.endswith(".hip"))
    assert re.search(r"vlm_abi_version\(void\)\s*\{\s*return 8;", src)
    body = re.search(r"typedef struct vlm_penalty_args \{(.*?)\} vlm_penalty_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [n for n, _ in _lib.PenaltyArgs._fields_] == [
        "hist", "hist_len", "hist_cap", "rep_penalty", "rep_ctx", "pres_penalty", "pres_ctx", "freq_penalty", "freq_ctx", "bias_idx",
        "bias_val", "n_bias", "row_params", "bias_stride"]
    assert [t for _, t in _lib.PenaltyArgs._fields_] == [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int,
                                                         C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert "W (slot 7" in hdr                                   # the encoding is documented next to row_params
