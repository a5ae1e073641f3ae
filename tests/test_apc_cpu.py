"""Automatic prefix caching without a GPU: the manager's rules (mlx_vlm_amd/apc.py - chain hash, image salt, LRU eviction with
reference counts, stats), the media rule and the length cap, the store / restore round trip on CPU pools of both layouts, and
`BatchGenerator(apc_manager=)` driven by the mock engine of tests/test_batch_scheduler_cpu.py."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mlx_vlm_amd import apc
from mlx_vlm_amd.apc import APCManager
from mlx_vlm_amd.models.cache import KVPool, PagedSequence
from tests.test_batch_scheduler_cpu import MockEngineGenerator, V, drain, first_token, make_pool, stream_alone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the keys of the reference's APCStats.snapshot (mlx_vlm/apc.py:614-637) + what its stats_snapshot adds without a disk tier
SNAPSHOT_KEYS = {"block_size", "num_blocks", "pool_used", "lookups_hit", "lookups_miss", "matched_tokens", "served_tokens",
                 "token_hit_rate", "evictions", "stores", "disk_hits", "disk_writes", "exact_hits", "exact_stores", "rejects",
                 "rejects_by_reason", "last_reject", "resident_bytes"}


def small_pool(layout="paged", n_layers=3, Hkv=2, D=128, max_seqs=6):
    return KVPool(n_layers=n_layers, n_kv_heads=Hkv, head_dim=D, max_tokens=64 * 24, max_seqs=max_seqs, max_pages_per_seq=4,
                  device="cpu", layout=layout)


def seq_with_pattern(pool, n_tokens, seed):
    """a sequence whose pages hold a seeded pattern in every layer (K and V)"""
    seq = PagedSequence(pool)
    seq.reserve(n_tokens)
    g = torch.Generator().manual_seed(seed)
    kv, vv = APCManager._pool_views(pool)
    for p in seq.pages:
        kv[:, p] = torch.randn(pool.n_layers, kv.shape[2], generator=g).to(torch.bfloat16)
        vv[:, p] = torch.randn(pool.n_layers, vv.shape[2], generator=g).to(torch.bfloat16)
    return seq


# ---------------------------------------------------------------------------------------------------------------- manager
def test_constructor_refusals():
    with pytest.raises(ValueError, match="page"):
        APCManager(num_blocks=4, block_size=16)
    with pytest.raises(NotImplementedError):
        APCManager(num_blocks=4, disk=object())
    assert APCManager().block_size == 64 and APCManager().num_blocks == 2048


def test_chain_lookup_salt_and_stats():
    pool = small_pool()
    rng = np.random.default_rng(0)
    p1 = rng.integers(1, 900, 200)
    p2 = np.concatenate([p1[:150], rng.integers(1, 900, 50)])
    p3 = p1.copy()
    p3[70] += 1
    mgr = APCManager(num_blocks=4)
    assert mgr.lookup_prefix(p1) == ([], 0)                        # before any store: a miss
    s1 = seq_with_pattern(pool, 200, 1)
    assert mgr.store_pages(p1, s1.pages, pool) == 3                # 200 // 64 full blocks
    b, m = mgr.lookup_prefix(p2)
    assert m == 128 and len(b) == 2 and all(x.ref_cnt == 1 for x in b)
    mgr.release(b)
    b, m = mgr.lookup_prefix(p3)
    assert m == 64
    mgr.release(b)
    b, m = mgr.lookup_prefix(p1)
    assert m == 192
    mgr.release(b)
    assert mgr.lookup_prefix(p1, extra_hash=77) == ([], 0)         # the same tokens under another image
    assert all(x.ref_cnt == 0 for x in mgr.blocks)
    mgr.record_served(200 + 72 + 136)
    snap = mgr.stats_snapshot()
    assert set(snap) == SNAPSHOT_KEYS
    assert (snap["lookups_hit"], snap["lookups_miss"], snap["matched_tokens"], snap["stores"], snap["evictions"]) == (3, 2, 384, 3, 0)
    assert snap["token_hit_rate"] == pytest.approx(384 / (384 + 408))
    assert snap["pool_used"] == 3 and snap["block_size"] == 64 and snap["num_blocks"] == 4
    assert all(snap[k] == 0 for k in ("disk_hits", "disk_writes", "exact_hits", "exact_stores"))
    assert snap["resident_bytes"] == mgr.resident_bytes() == 3 * 2 * 3 * (2 * 64 * 128) * 2
    mgr.reset_stats()
    assert mgr.stats_snapshot()["lookups_hit"] == 0 and mgr.stats_snapshot()["pool_used"] == 3
    mgr.clear()
    assert mgr.lookup_prefix(p1) == ([], 0) and mgr.stats_snapshot()["pool_used"] == 0
    mgr.close()
    assert mgr.store_k is None and mgr.resident_bytes() == 0


def test_eviction_is_lru_and_spares_acquired_blocks():
    pool = small_pool()
    mgr = APCManager(num_blocks=4)
    prompts = [np.full(64, 10 + i) for i in range(6)]
    seqs = [seq_with_pattern(pool, 64, 20 + i) for i in range(4)]
    for p, s in zip(prompts[:4], seqs):
        assert mgr.store_pages(p, s.pages, pool) == 1
    # touch them in the order 2, 0, 3 and keep 1 acquired: 2 is the least recently released of the free ones
    held, _ = mgr.lookup_prefix(prompts[1])
    for i in (2, 0, 3):
        b, m = mgr.lookup_prefix(prompts[i])
        assert m == 64
        mgr.release(b)
    assert mgr.store_pages(prompts[4], seqs[0].pages, pool) == 1              # the fifth block
    assert mgr.stats_snapshot()["evictions"] == 1
    assert mgr.lookup_prefix(prompts[2]) == ([], 0)                           # ... evicted the LRU one
    for i in (0, 3, 4):
        b, m = mgr.lookup_prefix(prompts[i])
        assert m == 64, i
        mgr.release(b)
    assert held[0].ref_cnt == 1 and held[0].key is not None           # never the acquired one
    # with all four acquired a store stores nothing and does not raise
    hold = [mgr.lookup_prefix(prompts[i])[0] for i in (0, 3, 4)]
    assert all(len(h) == 1 for h in hold)
    before = mgr.stats_snapshot()
    assert mgr.store_pages(prompts[5], seqs[1].pages, pool) == 0
    after = mgr.stats_snapshot()
    assert (after["stores"], after["evictions"], after["pool_used"]) == (before["stores"], before["evictions"], 4)
    for h in hold + [held]:
        mgr.release(h)
    assert all(x.ref_cnt == 0 for x in mgr.blocks)


def test_a_chain_never_evicts_its_own_head():
    """3 blocks into a 2-block store: the first two are kept, the third finds no free slot (its parents are held)"""
    pool = small_pool()
    mgr = APCManager(num_blocks=2)
    p = np.arange(1, 201)
    s = seq_with_pattern(pool, 200, 3)
    assert mgr.store_pages(p, s.pages, pool) == 2
    b, m = mgr.lookup_prefix(p)
    assert m == 128
    mgr.release(b)


# ---------------------------------------------------------------------------------------------------------------- rules
def test_media_rule_truth_table():
    I, W = 1001, 1002                      # noqa: E741
    media = apc.media_token_ids(SimpleNamespace(image_token_id=I, video_token_id=W))
    assert media == {I, W} and apc.media_token_ids(SimpleNamespace()) == frozenset()
    ids = [5, 6] + [I] * 70 + list(range(10, 210))           # [t t I .. I t t ...]: the span ends at 72
    n = len(ids)
    assert apc.media_safe_prefix_min(ids, media) == 72
    assert apc.usable_prefix_len(n, 64, 72) == (0, "media_suffix")          # ends inside the span
    assert apc.usable_prefix_len(n, 128, 72) == (128, None)                 # after it
    assert apc.usable_prefix_len(n, 0, 72) == (0, None)                     # nothing matched: no reject
    short = [5] * 70 + [I] * 4 + [7] * 100                                  # the span starts after the first block
    assert apc.media_safe_prefix_min(short, media) == 74
    assert apc.usable_prefix_len(len(short), 64, 74) == (0, "media_suffix")   # ends before the span: the suffix holds the image
    assert apc.usable_prefix_len(len(short), 128, 74) == (128, None)
    text = list(range(300))
    assert apc.media_safe_prefix_min(text, media) == 0 and apc.usable_prefix_len(300, 256, 0) == (256, None)
    two = [5] * 10 + [I] * 20 + [6] * 50 + [W] * 60 + [7] * 100             # two spans: the LAST one's end counts (140)
    assert apc.media_safe_prefix_min(two, media) == 140
    assert apc.usable_prefix_len(len(two), 128, 140) == (0, "media_suffix")
    assert apc.usable_prefix_len(len(two), 192, 140) == (192, None)


def test_length_cap():
    assert apc.usable_prefix_len(128, 128) == (64, None)        # fully cached: the last token still needs a forward
    assert apc.usable_prefix_len(129, 128) == (128, None)
    assert apc.usable_prefix_len(64, 64) == (0, None)
    assert apc.usable_prefix_len(1, 0) == (0, None)


def test_image_salt():
    pix = np.arange(24, dtype=np.float32).reshape(4, 6)
    grid = np.asarray([[1, 2, 2]])
    h = apc.hash_image_payload(pix, grid)
    assert h != 0 and apc.hash_image_payload(None, None) == 0
    assert h == apc.hash_image_payload(pix.copy(), grid.copy()) == apc.hash_image_payload(torch.from_numpy(pix), grid)
    other = pix.copy()
    other[3, 5] += 1
    assert len({h, apc.hash_image_payload(other, grid), apc.hash_image_payload(pix.reshape(6, 4), grid),
                apc.hash_image_payload(pix.astype(np.float64), grid), apc.hash_image_payload(pix, np.asarray([[1, 4, 1]]))}) == 5


def test_image_salt_of_a_large_buffer_sees_every_bit():
    """a patch matrix larger than one chunk of the two-level hash: single-bit changes anywhere, and PAIRS of sign flips (which cancel in any sum of words
    modulo 2^64), give other salts"""
    rng = np.random.default_rng(3)
    pix = rng.standard_normal((160, 1176)).astype(np.float32)
    grid = np.asarray([[1, 8, 8]])
    assert pix.nbytes > apc._SALT_CHUNK and pix.nbytes % apc._SALT_CHUNK          # two chunks, the second one ragged
    h = apc.hash_image_payload(pix, grid)
    assert h == apc.hash_image_payload(pix.copy(), grid) == apc.hash_image_payload(torch.from_numpy(pix.copy()), grid)
    seen = {h}
    for i, j in ((0, 1), (0, 2), (5, 175263), (1000, 140001)):          # sign flips of two elements (same and different 64-bit words)
        other = pix.copy().reshape(-1)
        other[i], other[j] = -other[i], -other[j]
        assert not np.array_equal(other, pix.reshape(-1))
        seen.add(apc.hash_image_payload(other.reshape(pix.shape), grid))
    for pos, bit in ((0, 0), (12345, 31), (pix.size - 1, 30), (pix.size // 2, 7)):
        raw = pix.copy().reshape(-1).view(np.uint32)
        raw[pos] ^= np.uint32(1 << bit)
        seen.add(apc.hash_image_payload(raw.view(np.float32).reshape(pix.shape), grid))
    swapped = pix.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                                   # the same bytes in another order
    seen.add(apc.hash_image_payload(swapped, grid))
    assert len(seen) == 1 + 4 + 4 + 1


# ---------------------------------------------------------------------------------------------------------------- device store
@pytest.mark.parametrize("layout", ["paged", "identity"])
def test_store_restore_round_trip(layout):
    pool = small_pool(layout)
    assert pool.identity == (layout == "identity")
    mgr = APCManager(num_blocks=4)
    ids = np.arange(1, 201)
    src = seq_with_pattern(pool, 200, 40)
    left, right = seq_with_pattern(pool, 64, 41), seq_with_pattern(pool, 64, 42)          # neighbours of the destination
    dst = seq_with_pattern(pool, 200, 43)
    assert mgr.store_pages(ids, src.pages, pool) == 3
    assert tuple(mgr.store_k.shape) == (3, 4, 2 * 64 * 128) and mgr.store_k.dtype == torch.bfloat16
    kv, vv = APCManager._pool_views(pool)
    before_k, before_v = kv.clone(), vv.clone()
    blocks, m = mgr.lookup_prefix(ids)
    assert m == 192
    mgr.restore(blocks[:2], dst.pages[:2], pool)
    mgr.release(blocks)
    for t, b4 in ((kv, before_k), (vv, before_v)):
        for i in range(2):
            assert torch.equal(t[:, dst.pages[i]], b4[:, src.pages[i]])                  # every layer
        untouched = [p for p in range(pool.n_pages) if p not in dst.pages[:2]]
        assert torch.equal(t[:, untouched], b4[:, untouched])                            # the third page, the neighbours, the rest
    with pytest.raises(ValueError):
        mgr.restore(blocks[:1], dst.pages[:1], pool)                                      # released: not acquired any more
    with pytest.raises(ValueError):
        mgr.store_pages(ids + 1, src.pages, small_pool(layout))                           # one manager, one pool
    for s in (src, left, right, dst):
        s.release()


# ---------------------------------------------------------------------------------------------------------------- scheduler
class MockAPCGenerator(MockEngineGenerator):
    """the mock engine with the prefix cache's host side left in: plan, restore copies, store"""

    def __init__(self, pool, **kw):
        self.admitted = []                      # (uid, prefix_len, suffix tokens) per admitted request
        super().__init__(pool, **kw)

    def _apc_check_engine(self, model):
        pass

    def _prefill_requests(self, batch):
        self.prefill_sizes.append(len(batch))
        plans = self._apc_plan(batch)
        caches, lens, toks = [], [], []
        for (uid, ids, max_tokens, kw), pl in zip(batch, plans):
            seq = PagedSequence(self.lm.pool)
            seq.reserve(len(ids) + max_tokens + 2)
            prefix = 0
            if pl is not None and pl.prefix_len:
                prefix = pl.prefix_len
                self._apc_restore(seq, pl)
                assert seq.offset == prefix and not pl.blocks
            self.admitted.append((uid, prefix, len(ids) - prefix))
            seq.offset = len(ids)
            caches.append([SimpleNamespace(_seq=seq)])
            lens.append(len(ids))
            toks.append(first_token(ids))
        self._apc_commit(batch, caches, plans)
        tok0 = torch.tensor(toks, dtype=torch.int32)
        lp0 = -tok0.float() / V if self.compute_logprobs else None
        ctx = np.asarray(lens, dtype=np.int32)
        delta = np.asarray([b[3].get("delta", 0) for b in batch], dtype=np.int32)
        return caches, lens, tok0, lp0, torch.from_numpy(np.stack([ctx + delta, ctx]))


@pytest.mark.parametrize("paged", [True, False])
def test_scheduler_with_a_manager(paged):
    rng = np.random.default_rng(5)
    pool = make_pool(paged=paged)
    free_pages, free_seqs = len(pool._free_pages), len(pool._free_seqs)
    common = rng.integers(1, 999, 130)
    a = np.concatenate([common, rng.integers(1, 999, 30)])
    b = np.concatenate([common, rng.integers(1, 999, 47)])
    others = [rng.integers(1, 999, int(rng.integers(3, 150))) for _ in range(9)]
    mgr = APCManager(num_blocks=16)
    gen = MockAPCGenerator(pool, completion_batch_size=4, prefill_batch_size=1, prefill_ahead=0, apc_manager=mgr)
    prompts = [a, b] + others
    max_tokens = [int(rng.integers(1, 12)) for _ in prompts]
    uids = gen.insert(prompts, max_tokens)
    got, reasons, seen, _ = drain(gen)
    for u, p, m in zip(uids, prompts, max_tokens):
        assert [t for t, _ in got[u]] == stream_alone(p, m), u                 # the stream it emits alone
        assert reasons[u] == "length" and seen[u] == len(p)
    adm = {u: (pre, sfx) for u, pre, sfx in gen.admitted}
    assert adm[uids[0]] == (0, len(a))                                         # (a is shorter: admitted first, cold)
    assert adm[uids[1]] == (128, len(b) - 128)                                 # b is admitted warm
    snap = mgr.stats_snapshot()
    assert snap["lookups_hit"] == 1 and snap["matched_tokens"] == 128
    assert snap["lookups_miss"] == len(prompts) - 1
    assert snap["served_tokens"] == sum(len(p) for p in prompts) - 128
    assert snap["stores"] == sum(len(p) // 64 for p in prompts) - 2            # b's first two blocks were held already
    assert all(x.ref_cnt == 0 for x in mgr.blocks)
    gen.close()
    assert len(pool._free_pages) == free_pages and len(pool._free_seqs) == free_seqs
    assert mgr.stats_snapshot()["pool_used"] == snap["pool_used"] > 0          # close() leaves the manager it was handed open


def test_generator_refusals_and_stats_keys():
    pool = make_pool()
    plain = MockEngineGenerator(pool)
    keys = set(vars(plain.stats()))
    plain.close()
    gen = MockAPCGenerator(pool, apc_manager=APCManager(num_blocks=2))
    assert set(vars(gen.stats())) == keys                                      # stats() keeps its keys
    gen.close()
    with pytest.raises(NotImplementedError, match="kv_bits"):
        MockAPCGenerator(pool, apc_manager=APCManager(num_blocks=2), kv_bits=8)
    with pytest.raises(NotImplementedError, match="Qwen2-VL"):
        MockEngineGenerator(pool, apc_manager=APCManager(num_blocks=2))        # a model without the Qwen2-VL embedding path


def test_header_facts():
    """the bf16 form travels through an existing symbol: still 60 names, still v8"""
    hdr = open(os.path.join(ROOT, "include", "vlm_hip.h")).read()
    assert len(set(re.findall(r"\b(vlm_[a-z0-9_]+)\s*\(", hdr))) == 60
    src = open(os.path.join(ROOT, "mlx-vlm_amd", "csrc", "engine.hip")).read()
    assert re.search(r"vlm_abi_version\(void\)\s*\{\s*return 8;", src)
    from mlx_vlm_amd import _lib

    assert len(_lib.SIGNATURES["vlm_attn_prefill_paged_q8"][1]) == 20
