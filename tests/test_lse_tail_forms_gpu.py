"""Bits 13 and 14 of VLM_TUNE_GEMV_VARIANT (include/vlm_hip.h): the greedy tail's two launches in their lean forms -
lse_partial_kernel_regs loads a thread's elements once and keeps them across the max pass, the barrier and the sum pass;
logprob_argmax_tail_kernel_lean issues its logits loads ahead of the partials' and, with one row, takes one ticket level.
They change when things happen, never what is computed: bits on are held to the BYTES of bits off, in the same library,
through vlm_sample_greedy_advance (the off side is held to the exact result by tests/test_sampler_exact_gpu.py).

Compared, all as integers: the (max, sum exp) partial words and the candidates of every row's workspace block, the whole
log-prob buffer (pad columns included), tok, ctx, pos, step, the token ring and the gathered h rows; both tickets read zero
after every launch.

    V = 8          63 empty blocks, partial (-inf, 0)
    V = 520        per = 16, the last non-empty block is half full
    V = 32,003     at pitch 32,008: 16-byte trips and a ragged scalar end of three
    V = 151,936    ten values per thread in the one-pass form, two vector trips in the tail
    V = 163,848    per = 2568 > 2560: past the register-resident bound, the loop form runs under bit 13 too
    B = 1, 2, 16   the one-level and the two-level ticket

Rows: bf16 of a seeded N(0, 4); the same with -inf holes; all elements equal (token 0); the maximum twice, at per - 1 and
per, across a block boundary (token per - 1); all NaN (token 0, ops.bad_argmax_rows + 1).  With logprobs = nullptr the
token and the state are the same and a canary-filled buffer stays untouched.  Twenty launches back to back on changing
inputs leave the state of twenty launches of the off form."""
import pytest
import torch

from oracle import qwen2_vl as oq
from tests.helpers import build_product_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LSE, TAIL = 1 << 13, 1 << 14
NBLK, ROW_W, ROW_CTL, CTL_ROW_TICKET = 64, 65920, 4 * 64 + 65536, 120
DM, RING = 64, 4
KINDS = ["plain", "holes", "equal", "dupmax", "nan"]
SHAPES = [(8, 8), (520, 520), (32003, 32008), (151936, 151936), (163848, 163848)]      # (V, pitch)


@pytest.fixture(scope="module")
def variant():
    """set(bits): the process-wide variant (travels through vlm_llm_set_tuning: the module builds a tiny model for its handle)"""
    cfg = oq.tiny_cfg()
    W = oq.random_weights(cfg, seed=1234, dtype=BF, std=0.05, embed_std=0.2)
    lm = build_product_model(cfg, W, kv_pool_tokens=1024, max_seqs=2).language_model
    base = lm.TUNING_DEFAULTS["gemv_variant"] & ~(LSE | TAIL)
    yield lambda bits: lm.apply_tuning(gemv_variant=base | bits)
    lm.apply_tuning()


def per_of(V):
    return ((V + NBLK - 1) // NBLK + 7) & ~7


def make_rows(V, kinds, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(len(kinds), V, generator=g, device="cuda") * 2.0).to(BF)
    per = per_of(V)
    for r, kind in enumerate(kinds):
        if kind == "holes":
            x[r, torch.rand(V, generator=g, device="cuda") < 0.3] = float("-inf")
            x[r, V // 2] = 1.0                                     # (one finite element whatever the draw)
        elif kind == "equal":
            x[r] = 0.75
        elif kind == "dupmax":
            x[r, min(per, V - 1)] = 60.0
            x[r, min(per, V - 1) - 1] = 60.0
        elif kind == "nan":
            x[r] = float("nan")
    return x


def expected_token(V, kind):
    return {"equal": 0, "nan": 0, "dupmax": min(per_of(V), V - 1) - 1}.get(kind)


class State:
    def __init__(self, B, V, pitch, embed):
        from mlx_vlm_amd import ops

        self.B, self.V, self.pitch, self.embed = B, V, pitch, embed
        self.logits = torch.full((B, pitch), float("nan"), dtype=BF, device="cuda")
        self.lp = torch.full((B, pitch), -7.0, dtype=BF, device="cuda")        # canary: -7.0 in every word
        self.ws = ops.sample_workspace(B, "cuda")
        self.tok = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        self.ctx = torch.arange(10, 10 + B, dtype=torch.int32, device="cuda")
        self.pos = torch.arange(100, 100 + B, dtype=torch.int32, device="cuda")
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ring = torch.full((RING, B), -1, dtype=torch.int32, device="cuda")
        self.h = torch.zeros(B, DM, dtype=BF, device="cuda")

    def launch(self, x, with_lp=True):
        from mlx_vlm_amd import _lib, ops

        self.logits[:, :self.V] = x
        rc = _lib.lib().vlm_sample_greedy_advance(ops._p(self.logits), self.pitch, self.B, self.V, ops._p(self.lp) if with_lp else None,
                                                  self.pitch, ops._p(self.tok), ops._p(self.ws), ops._p(self.ctx), ops._p(self.pos),
                                                  ops._p(self.ring), RING, ops._p(self.step), ops._p(self.embed), ops._p(self.h), DM, DM,
                                                  ops._stream())
        assert rc == 0, rc

    def words(self):
        return self.ws.view(torch.int32)

    def snapshot(self):
        """everything the two launches leave behind, as integers; the tickets must be back at zero"""
        torch.cuda.synchronize()
        w = self.words()
        rows = w[64:64 + self.B * ROW_W].view(self.B, ROW_W)
        assert int(w[0]) == 0, "launch ticket"
        assert rows[:, ROW_CTL + CTL_ROW_TICKET].tolist() == [0] * self.B, "row tickets"
        return dict(partials=rows[:, :2 * NBLK].clone(), cands=rows[:, 2 * NBLK:4 * NBLK].clone(), bad=int(w[1]),
                    lp=self.lp.view(torch.int16).clone(), tok=self.tok.clone(), ctx=self.ctx.clone(), pos=self.pos.clone(),
                    step=self.step.clone(), ring=self.ring.clone(), h=self.h.view(torch.int16).clone())


def same(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        eq = a[k] == b[k] if isinstance(a[k], int) else torch.equal(a[k], b[k])
        assert eq, (what, k)


_EMBED = {}


def embed_of(V):
    if V not in _EMBED:
        g = torch.Generator(device="cuda").manual_seed(V)
        _EMBED[V] = torch.randn(V, DM, generator=g, device="cuda").to(BF)
    return _EMBED[V]


def batches(B):
    if B == 1:
        return [[k] for k in KINDS]
    if B == 2:
        return [["plain", "dupmax"], ["nan", "holes"], ["equal", "plain"]]
    return [[KINDS[r % len(KINDS)] for r in range(B)]]


@pytest.mark.parametrize("B", [1, 2, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%d" % s[0])
def test_lean_forms_give_the_bytes_of_the_two_pass_forms(variant, shape, B):
    V, pitch = shape
    embed = embed_of(V)
    for n, kinds in enumerate(batches(B)):
        x = make_rows(V, kinds, seed=1000 * n + V % 997 + B)
        got = {}
        for bits in (0, LSE, TAIL, LSE | TAIL):
            variant(bits)
            st = State(B, V, pitch, embed)
            st.launch(x)
            got[bits] = st.snapshot()
        off = got[0]
        for bits in (LSE, TAIL, LSE | TAIL):
            same(got[bits], off, (V, B, kinds, bits))
        # the off side itself, where the row names its token: lowest index on ties, token 0 and one count for a row without a candidate
        for r, kind in enumerate(kinds):
            want = expected_token(V, kind)
            if want is not None:
                assert int(off["tok"][r]) == want, (V, B, kind)
        assert off["bad"] == kinds.count("nan")
        assert torch.equal(off["h"], embed[off["tok"].long()].view(torch.int16))
        assert off["ctx"].tolist() == list(range(11, 11 + B)) and off["pos"].tolist() == list(range(101, 101 + B))
        assert off["ring"][0].tolist() == off["tok"].tolist() and int(off["step"]) == 1
        assert bool((off["lp"].view(BF)[:, V:] == -7.0).all())                   # nothing at or past V is written
        if V == 8:
            p = off["partials"].view(torch.float32).view(B, NBLK, 2)
            assert bool((p[:, 1:, 0] == float("-inf")).all()) and bool((p[:, 1:, 1] == 0).all())
        # no log-prob pointer: the same token and state, in both forms, and the buffer of the call before is not touched
        for bits in (0, LSE | TAIL):
            variant(bits)
            st = State(B, V, pitch, embed)
            st.launch(x, with_lp=False)
            snap = st.snapshot()
            same(snap, off, (V, B, kinds, bits, "nullptr"), skip=("lp",))
            assert bool((snap["lp"].view(BF) == -7.0).all())


@pytest.mark.parametrize("V,B", [(520, 1), (520, 16), (151936, 1)])
def test_twenty_replays_back_to_back_leave_the_tickets_at_zero(variant, V, B):
    embed = embed_of(V)
    kinds = [KINDS[r % len(KINDS)] for r in range(B)]
    xs = [make_rows(V, kinds if i % 4 == 3 else ["plain"] * B, seed=77 * i + V % 997 + B) for i in range(20)]
    got = {}
    for bits in (0, LSE | TAIL):
        variant(bits)
        st = State(B, V, V, embed)
        toks = torch.full((20, B), -1, dtype=torch.int32, device="cuda")
        for i, x in enumerate(xs):                      # no synchronisation between the launches
            st.launch(x)
            toks[i].copy_(st.tok)
        got[bits] = (st.snapshot(), toks)
    same(got[LSE | TAIL][0], got[0][0], (V, B, "replays"))
    assert torch.equal(got[LSE | TAIL][1], got[0][1])
    assert int(got[0][0]["step"]) == 20 and got[0][0]["ctx"].tolist() == list(range(30, 30 + B))
    assert got[0][0]["bad"] == 5 * kinds.count("nan")
