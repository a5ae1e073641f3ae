"""max_kv_size as a device-resident window, host side (no GPU): the rule a decode step's tail applies on the device
(csrc/internal.h vlm_window_advance; include/vlm_hip.h VLM_DECODE_WINDOW) has ONE host mirror, models/cache.py
window_start / window_step.  Replaying the mirror on a slot -> token table must leave, after every step, exactly the tokens the
reference's RotatingKVCache holds, and read the same `_idx` before every update - against oracle.ops.RotatingKVCache, the
restatement pinned bit for bit to the reference class by tests/golden/rotating_ref.npz (test_oracle_ref_golden_rotating).

Also pinned here: the window travels through the frozen C ABI (a flag bit and three keys of vlm_llm_set_tuning - no new symbol,
version 8)."""
import os
import re

import pytest
import torch

from mlx_vlm_amd import _lib
from mlx_vlm_amd.models import cache as C
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(24, 4), (20, 4), (7, 4), (64, 4), (10, 0)]


def _tag(a, b):
    return torch.arange(a, b, dtype=torch.float32).reshape(1, 1, b - a, 1)


@pytest.mark.parametrize("M,K", WINDOWS)
def test_mirror_holds_the_references_tokens_and_reads_its_idx(M, K):
    for L in range(1, 3 * M + 2):
        oc = O.RotatingKVCache(M, keep=K)
        oc.update_and_fetch(_tag(0, L), _tag(0, L))
        slots = {i: i for i in range(L)}                     # slot -> token index, as the prefill writes a first prompt
        n, w, src, dst = C.window_start(L, M, K)
        # the one move call: sources beyond the window, destinations inside it, the two sets disjoint, no destination twice and
        # none that holds a survivor which stays
        assert len(src) == len(dst) == len(set(src)) == len(set(dst))
        assert not (set(src) & set(dst))
        assert all(M <= a < L for a in src) and all(K <= d < M for d in dst)
        stay = {t for t in range(max(K, L - (M - K) + 1), L) if t < M}
        assert not (stay & set(dst)) and w not in dst and (L < M or w not in stay)
        slots.update({d: slots[a] for a, d in zip(src, dst)})
        if L >= M:
            survivors = list(range(K)) + list(range(L - (M - K) + 1, L))
            assert sorted(slots[i] for i in range(M) if i != w) == survivors, (M, K, L)
        r = L
        assert 0 <= n <= M - 1 and 0 <= w < M
        for t in range(L, L + 3 * M):
            assert r == oc._idx, (M, K, L, t)                # what the forward of this step reads as the cache offset
            assert (K <= w < M or w == n) and w < M          # the write never leaves the window's slots
            slots[w] = t
            seen = sorted(slots[i] for i in range(n + 1))
            k, _ = oc.update_and_fetch(_tag(t, t + 1), _tag(t, t + 1))
            assert seen == sorted(int(x) for x in k.reshape(-1)), (M, K, L, t)
            n, w, r = C.window_step(n, w, r, M, K)


def test_paged_sequence_follows_the_mirror_and_keeps_the_facade():
    pool = C.KVPool(n_layers=1, n_kv_heads=1, head_dim=8, max_tokens=4096, max_seqs=4, device="cpu", layout="paged")
    s = C.PagedSequence(pool)
    c = C.KVCache(s, 0)
    s.set_rotating(24, keep=4)
    s.offset += 41
    s.note_prefill(41)
    src, dst = s.window_enter()
    assert (s.held, s.win_w) == C.window_start(41, 24, 4)[:2] and (src, dst) == tuple(C.window_start(41, 24, 4)[2:])
    assert s.window_enter() == ([], [])                      # already there: nothing moves twice
    st = s.window_state()
    s.window_advance(50)
    n, w, r = st
    for _ in range(50):
        n, w, r = C.window_step(n, w, r, 24, 4)
    assert s.window_state() == (n, w, r) and s.kv_entries == 23
    s.offset += 50
    assert c.size() == 24 and not c.is_trimmable()
    with pytest.raises(NotImplementedError):
        c.trim(1)                                            # a wrapped window
    with pytest.raises(RuntimeError):
        s.rotate_plan()                                      # one arrangement per sequence
    # not wrapped yet: trim moves all of the state
    s2 = C.PagedSequence(pool)
    s2.set_rotating(24, keep=4)
    s2.offset += 10
    s2.note_prefill(10)
    s2.window_enter()
    s2.window_advance(3)
    s2.offset += 3
    assert C.KVCache(s2, 0).trim(2) == 2 and (s2.offset,) + s2.window_state() == (11, 11, 11, 11)
    # a window that wrapped on the host-planned arrangement stays there
    s3 = C.PagedSequence(pool)
    s3.set_rotating(24, keep=4)
    s3.offset += 30
    s3.note_prefill(30)
    s3.rotate_plan()
    with pytest.raises(NotImplementedError):
        s3.window_enter()


def test_the_window_travels_through_the_frozen_abi():
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    defs = dict(re.findall(r"#define\s+(VLM_[A-Z0-9_]+)\s+(\d+)\b", hdr))
    assert int(defs["VLM_DECODE_WINDOW"]) == 4 == _lib.DECODE_WINDOW
    assert (_lib.MODE_WINDOW_SIZE, _lib.MODE_WINDOW_KEEP, _lib.MODE_WINDOW_RING_POS) == (16, 17, 18)
    assert [int(defs[k]) for k in ("VLM_MODE_WINDOW_SIZE", "VLM_MODE_WINDOW_KEEP", "VLM_MODE_WINDOW_RING_POS")] == [16, 17, 18]
    assert not (_lib.DECODE_WINDOW & (_lib.DECODE_FUSED_TAIL | _lib.DECODE_ACT16))
    L = _lib.lib()
    assert L.vlm_abi_version() == 8
    # the keys on a handle (host-side construction; no device needed): defaults, round trip, refusals
    import ctypes as ct

    cfg = _lib.LlmConfig(64, 1, 128, 2, 1, 32, 256, 1e-6, 4, 6, 0.0, 0.0, 0)
    h = ct.c_void_p()
    assert L.vlm_llm_create(ct.byref(cfg), ct.byref(h)) == 0
    try:
        keys = (_lib.MODE_WINDOW_SIZE, _lib.MODE_WINDOW_KEEP, _lib.MODE_WINDOW_RING_POS)
        assert [L.vlm_llm_get_tuning(h, k) for k in keys] == [0, 0, 0]
        for k, v in zip(keys, (24, 4, 1)):
            assert L.vlm_llm_set_tuning(h, k, v) == 0
        assert [L.vlm_llm_get_tuning(h, k) for k in keys] == [24, 4, 1]
        assert L.vlm_llm_set_tuning(h, _lib.MODE_WINDOW_SIZE, -1) != 0 and L.vlm_llm_set_tuning(h, _lib.MODE_WINDOW_RING_POS, 2) != 0
        assert L.vlm_llm_set_tuning(h, _lib.MODE_WINDOW_SIZE, 0) == 0          # 0 switches the window off
    finally:
        L.vlm_llm_destroy(h)
