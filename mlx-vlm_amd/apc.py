"""Automatic prefix caching (APC) over the paged KV pool: hash-chained, block-level KV reuse across requests, with the
public names of the reference's manager (mlx_vlm/apc.py:2856-3513: `APCManager(num_blocks, block_size)`, `lookup_prefix`,
`release`, `stats_snapshot`, `reset_stats`, `clear`, `close`, `resident_bytes`), so that a server written against it binds
unchanged.  `BatchGenerator(apc_manager=mgr)` (batch.py) is its user here.

The rules are the reference's:

  * chain hash - block_hash[i] = H(block_hash[i - 1], tokens of block i, extra_hash), parent of block 0 = 0.  A lookup walks the
    full blocks of a prompt from the start and stops at the first miss or token mismatch (apc.py:3288-3319); it ACQUIRES what
    it matched (ref_cnt += 1) and the caller releases it;
  * eviction - a block with ref_cnt > 0 is never evicted; the blocks with ref_cnt == 0 form an LRU queue and a store takes its
    slots from the queue's head;
  * stats - hits / misses / matched_tokens are counted by the lookup, stores / evictions by the store, served_tokens by the
    generator for the tokens it really prefilled; `stats_snapshot()` has the reference's keys (the disk and exact-snapshot
    tiers are not built: their counters are present and 0);
  * image salt - `extra_hash` of a request is a content hash of its pixel_values (shape, dtype, bytes) and image_grid_thw, 0 for
    a text-only request (ar.py:2290-2315): the same tokens under another image are another chain;
  * media rule - a prefix is usable only if the suffix is text-only, i.e. it reaches the end of the last run of image / video
    placeholder tokens (apc.py:420-464).

Where this differs from the reference, on purpose:

  * a prefix that covers every media span WHOLE is used.  The reference's block mode drops any prefix that contains media tokens
    and leaves such prompts to its exact-snapshot tier; here the image is in the salt and the K / V of a causal model depend on
    nothing after the prefix, so the blocks of [text | image | text] are as good as those of text alone.  (M-RoPE positions are
    a function of the prompt's tokens and grid up to each position: equal prefixes and equal grids give equal positions.)
  * `block_size` is 64, the pool's page, and nothing else: one page of one layer is ONE contiguous run of bytes in kpool /
    vpool (K [page][Hkv][D/8][64][8], V [page][Hkv][D][64 key slots]), so a cached block is a page-sized copy per layer; a
    16-token block (the reference's default) is 16 strided slivers of a page in K and a permuted subset of key slots in V.
  * the store call takes PAGE IDS of a sequence (`store_pages`) instead of per-layer arrays (the reference's `store_kv_blocks`
    takes MLX arrays, which do not exist here), and `restore` copies blocks back into pages.
  * the prefix is copied in, not shared: the identity pool layout, which the decode kernels use without a block-table load,
    gives every sequence slot its own fixed pages, so two sequences cannot name one page.

Device store: `store_k` / `store_v` [n_layers, num_blocks, Hkv * 64 * D] bf16, allocated on first use next to the pool they
serve (device="cpu" pools too).  Both directions are indexed copies on views of the pools - torch as plumbing, no kernel - and
go through page ids (`seq.pages`), never through the block table, so both pool layouts work.

STREAM INVARIANT.  The manager's bookkeeping (hash table, LRU queue, ref counts) is host state and is final when a call
returns; the copies are only ENQUEUED.  Every copy of a manager - store, restore, and therefore the overwrite of an evicted
slot - must be enqueued on ONE stream: the stream its generators' admissions run on (`batch._admission_stream`, or the current
stream with async_prefill=False; generators that share a manager share that choice).  Stream order is then the only
synchronisation needed: a restore enqueued before the store that evicts its block reads the old bytes, one enqueued after a
store reads the new ones.  That is also why a generator may release the blocks it acquired as soon as its restore copies are
enqueued - a later eviction can only be enqueued behind them.

Not built: the disk tier (`disk=` other than None raises NotImplementedError), the exact-snapshot tier, tenants, `from_env`.
"""
from __future__ import annotations

import hashlib
import threading
from collections import Counter, OrderedDict
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import h2d
from .models.cache import PAGE

DEFAULT_NUM_BLOCKS = 2048
DEFAULT_BLOCK_SIZE = PAGE
_ROOT_KEY = bytes(16)          # the parent of a prompt's first block ("seed parent 0")
_MASK128 = (1 << 128) - 1


def _salt_bytes(extra_hash: int) -> bytes:
    return (int(extra_hash) & _MASK128).to_bytes(16, "little")


def _block_key(parent: bytes, salt: bytes, tokens: bytes) -> bytes:
    """H(parent key, tokens of the block, salt): 128 bits of BLAKE2b"""
    return hashlib.blake2b(parent + salt + tokens, digest_size=16).digest()


_SALT_CHUNK = 1 << 19          # bytes per leaf of the two-level hash of a large buffer (fixed: the digest depends on the bytes alone)
_salt_workers = None
_salt_workers_lock = threading.Lock()


def _workers():
    global _salt_workers
    with _salt_workers_lock:
        if _salt_workers is None:
            from concurrent.futures import ThreadPoolExecutor

            _salt_workers = ThreadPoolExecutor(max_workers=8, thread_name_prefix="apc-salt")
        return _salt_workers


def _sha256_of(raw: np.ndarray) -> bytes:
    """SHA-256 of a byte buffer.  Above one chunk: SHA-256 over (length, the SHA-256 of every 512 KiB chunk in order) - still a
    collision-resistant hash of all the bytes - with the chunks hashed on worker threads (hashlib releases the GIL)."""
    view = memoryview(raw)
    if raw.size <= _SALT_CHUNK:
        return hashlib.sha256(view).digest()
    leaves = _workers().map(lambda part: hashlib.sha256(part).digest(),
                            [view[o:o + _SALT_CHUNK] for o in range(0, raw.size, _SALT_CHUNK)])
    return hashlib.sha256(b"chunks" + int(raw.size).to_bytes(8, "little") + b"".join(leaves)).digest()


def hash_image_payload(pixel_values=None, image_grid_thw=None) -> int:
    """The image salt of a request: a content hash (SHA-256, 128 bits kept) of pixel_values - shape, dtype and every byte - and
    of image_grid_thw; 0 without pixels.  It is the only thing that separates the K / V of two images under equal tokens, so it
    is a real hash of all the bytes (large buffers chunk by chunk on worker threads: 0.5 ms for the 4.8 MB patch matrix of a
    448 x 448 image, profiles/apc_warm_admission.txt).  Pixels that already live on the device are
    read back for it."""
    if pixel_values is None:
        return 0
    h = hashlib.sha256()
    for x in (pixel_values, image_grid_thw):
        if x is None:
            h.update(b"<none>")
            continue
        if isinstance(x, torch.Tensor):
            t = x.detach().to("cpu").contiguous()
            shape, dtype = tuple(t.shape), str(t.dtype).replace("torch.", "")      # (the numpy spelling: one salt either way)
            raw = t.reshape(-1).view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)
        else:
            a = np.ascontiguousarray(np.asarray(x))
            shape, dtype = tuple(a.shape), str(a.dtype)
            raw = a.reshape(-1).view(np.uint8)
        h.update(f"<{shape}|{dtype}|{raw.size}>".encode())
        h.update(_sha256_of(raw))
    return int.from_bytes(h.digest()[:16], "little") or 1


def media_token_ids(config: Any) -> frozenset:
    """ids of the image / video placeholder tokens of a model config (missing attributes: none)"""
    ids = (getattr(config, "image_token_id", None), getattr(config, "video_token_id", None))
    return frozenset(int(i) for i in ids if i is not None)


def media_safe_prefix_min(token_ids: Sequence[int], media_ids: Iterable[int]) -> int:
    """end (exclusive) of the LAST run of media placeholder tokens: the shortest prefix that leaves a text-only suffix;
    0 for a text-only prompt"""
    ids = np.asarray(token_ids, dtype=np.int64).reshape(-1)
    media = list(media_ids)
    if not media or ids.size == 0:
        return 0
    at = np.nonzero(np.isin(ids, np.asarray(media, dtype=np.int64)))[0]
    return int(at[-1]) + 1 if at.size else 0


def usable_prefix_len(n_tokens: int, matched_tokens: int, safe_min: int = 0, block_size: int = DEFAULT_BLOCK_SIZE) -> Tuple[int, Optional[str]]:
    """What a generator may reuse of `matched_tokens` -> (prefix_len, reject reason or None).
    Length cap: prefix_len < n_tokens always - the last token's logits must come from a forward - so whole blocks of the first
    n_tokens - 1.  Media rule: the prefix must reach `safe_min` (media_safe_prefix_min), or nothing of it is used."""
    prefix = min(int(matched_tokens), block_size * ((int(n_tokens) - 1) // block_size))
    prefix = max(prefix, 0)
    if prefix and prefix < int(safe_min):
        return 0, "media_suffix"
    return prefix, None


class CachedBlock:
    """One slot of the store: which block of which chain it holds, and how many holders it has."""
    __slots__ = ("slot", "key", "tokens", "salt", "ref_cnt")

    def __init__(self, slot: int):
        self.slot = slot
        self.ref_cnt = 0
        self.forget()

    def forget(self):
        self.key: Optional[bytes] = None       # chain key of the block held (None: the slot is empty)
        self.tokens: bytes = b""               # its 64 token ids (int64 bytes): compared on every match, whatever the key says
        self.salt: bytes = b""

    def holds(self, key: bytes, salt: bytes, tokens: bytes) -> bool:
        return self.key == key and self.salt == salt and self.tokens == tokens


_COUNTERS = ("lookups_hit", "lookups_miss", "matched_tokens", "served_tokens", "evictions", "stores", "rejects")
_UNBUILT_TIERS = ("disk_hits", "disk_writes", "exact_hits", "exact_stores")      # present in the snapshot, always 0


class APCManager:
    """The table of cached blocks, their LRU order, the counters and the device store (module docstring)."""

    def __init__(self, num_blocks: int = DEFAULT_NUM_BLOCKS, block_size: int = DEFAULT_BLOCK_SIZE, disk=None):
        if int(block_size) != PAGE:
            raise ValueError(f"APCManager: block_size = {block_size}: a cached block is one {PAGE}-token page of the KV pool (one "
                             f"contiguous run of bytes per layer); a block of another size is not contiguous in the pool's layouts")
        if disk is not None:
            raise NotImplementedError("APCManager: the disk tier is not built (disk=None)")
        if int(num_blocks) < 1:
            raise ValueError(f"APCManager: num_blocks = {num_blocks}")
        self.block_size = int(block_size)
        self.num_blocks = int(num_blocks)
        self.disk = None
        self.lock = threading.RLock()
        self.blocks: List[CachedBlock] = [CachedBlock(i) for i in range(self.num_blocks)]
        # the device store, bound to ONE KV pool at first use
        self._kv_pool = None
        self.store_k: Optional[torch.Tensor] = None
        self.store_v: Optional[torch.Tensor] = None
        self._reset_table()
        self._reset_counters()

    def _reset_table(self):
        for blk in self.blocks:
            blk.forget()
            blk.ref_cnt = 0
        self._by_key: Dict[bytes, CachedBlock] = {}
        # blocks nobody holds, least recently released first: where a store takes its slots from
        self._idle: "OrderedDict[int, CachedBlock]" = OrderedDict((blk.slot, blk) for blk in self.blocks)

    def _reset_counters(self):
        self._n = Counter()
        self._reject_reasons = Counter()
        self._last_reject: Optional[dict] = None

    # ------------------------------------------------------------------ the chain and the LRU order (host state)
    def _chain(self, token_ids, extra_hash: int) -> Iterator[Tuple[bytes, bytes, bytes]]:
        """(key, salt, token bytes) of every FULL block of a prompt, in order: key_i = H(key_(i-1), tokens_i, salt)"""
        ids = np.ascontiguousarray(np.asarray(token_ids, dtype=np.int64).reshape(-1))
        salt, key = _salt_bytes(extra_hash), _ROOT_KEY
        for start in range(0, ids.size - self.block_size + 1, self.block_size):
            tokens = ids[start:start + self.block_size].tobytes()
            key = _block_key(key, salt, tokens)
            yield key, salt, tokens

    def _hold(self, blk: CachedBlock) -> CachedBlock:
        self._idle.pop(blk.slot, None)
        blk.ref_cnt += 1
        return blk

    def _drop(self, blk: CachedBlock):
        blk.ref_cnt = max(0, blk.ref_cnt - 1)
        if blk.ref_cnt == 0:
            self._idle[blk.slot] = blk
            self._idle.move_to_end(blk.slot)

    def _take_idle_slot(self) -> Optional[CachedBlock]:
        """the least recently released block nobody holds, emptied (an eviction if it held something); None: all are held"""
        if not self._idle:
            return None
        _, blk = self._idle.popitem(last=False)
        if blk.key is not None:
            self._by_key.pop(blk.key, None)
            self._n["evictions"] += 1
        blk.forget()
        return blk

    def release(self, blocks: Iterable[CachedBlock]) -> None:
        """Give back what a lookup acquired.  The blocks of one call join the LRU order last block first, so that a chain loses
        its TAIL first: a chain without its head matches nothing."""
        with self.lock:
            for blk in reversed(list(blocks)):
                self._drop(blk)

    # ------------------------------------------------------------------ lookup
    def lookup_prefix(self, token_ids: Sequence[int], extra_hash: int = 0) -> Tuple[List[CachedBlock], int]:
        """-> (blocks, matched_tokens): the blocks held for the longest run of full blocks from the start of `token_ids` under
        this salt - the walk ends at the first block that is not held or whose tokens differ.  The blocks come ACQUIRED
        (ref_cnt + 1 each); hand them to `release` when their copies are enqueued or they are not wanted."""
        with self.lock:
            found: List[CachedBlock] = []
            for key, salt, tokens in self._chain(token_ids, extra_hash):
                blk = self._by_key.get(key)
                if blk is None or not blk.holds(key, salt, tokens):
                    break
                found.append(self._hold(blk))
            n_tokens = len(found) * self.block_size
            self._n["lookups_hit" if found else "lookups_miss"] += 1
            self._n["matched_tokens"] += n_tokens
            return found, n_tokens

    def record_served(self, n_tokens: int) -> None:
        """tokens a generator really prefilled (the other half of token_hit_rate's denominator)"""
        with self.lock:
            self._n["served_tokens"] += int(n_tokens)

    def record_reject(self, reason: str, **details: Any) -> None:
        """a hit the generator could not use (the media rule), by reason"""
        with self.lock:
            self._n["rejects"] += 1
            self._reject_reasons[reason] += 1
            self._last_reject = dict(details, reason=reason)

    # ------------------------------------------------------------------ device store
    def _bind(self, kv_pool):
        if self._kv_pool is kv_pool:
            return
        if self._kv_pool is not None:
            raise ValueError("APCManager: this manager already serves another KV pool (one manager per language model: its blocks "
                             "are that model's K / V)")
        if kv_pool.kpool.dtype != torch.bfloat16:
            raise NotImplementedError("APCManager: bf16 KV pools")
        page_elems = kv_pool.n_kv_heads * PAGE * kv_pool.head_dim
        dev = kv_pool.kpool.device
        self.store_k = torch.zeros(kv_pool.n_layers, self.num_blocks, page_elems, dtype=torch.bfloat16, device=dev)
        self.store_v = torch.zeros(kv_pool.n_layers, self.num_blocks, page_elems, dtype=torch.bfloat16, device=dev)
        self._kv_pool = kv_pool

    @staticmethod
    def _pool_views(kv_pool):
        return (kv_pool.kpool.view(kv_pool.n_layers, kv_pool.n_pages, -1), kv_pool.vpool.view(kv_pool.n_layers, kv_pool.n_pages, -1))

    def store_pages(self, token_ids: Sequence[int], pages: Sequence[int], kv_pool, *, extra_hash: int = 0) -> int:
        """Cache the full blocks of a PROMPT whose K / V sit in `pages` (page i = tokens 64 i .. 64 i + 63 of the sequence, as
        `PagedSequence.pages` lists them): every block the table does not hold yet gets the least recently released idle slot and
        page pages[i] of every layer is copied into it (enqueued on the current stream: the stream invariant of the module
        docstring).  Stops at the first block that cannot get a slot (every slot held).  -> blocks stored."""
        fresh_slots, fresh_pages, pinned = [], [], []
        with self.lock:
            # every block of the chain passed so far stays held while the chain grows: a later block must not evict its own parent
            for i, (key, salt, tokens) in enumerate(self._chain(token_ids, extra_hash)):
                if i >= len(pages):
                    break
                blk = self._by_key.get(key)
                if blk is None or not blk.holds(key, salt, tokens):
                    blk = self._take_idle_slot()
                    if blk is None:
                        break
                    blk.key, blk.salt, blk.tokens = key, salt, tokens
                    self._by_key[key] = blk
                    self._n["stores"] += 1
                    fresh_slots.append(blk.slot)
                    fresh_pages.append(int(pages[i]))
                pinned.append(self._hold(blk))
            if fresh_slots:
                self._bind(kv_pool)
                self._copy(fresh_slots, fresh_pages, kv_pool, to_store=True)
            for blk in reversed(pinned):
                self._drop(blk)
        return len(fresh_slots)

    def restore(self, blocks: Sequence[CachedBlock], pages: Sequence[int], kv_pool) -> None:
        """block i -> page pages[i] of every layer (enqueued on the current stream).  `blocks` are acquired (a lookup's)."""
        if len(blocks) != len(pages):
            raise ValueError(f"APCManager.restore: {len(blocks)} blocks for {len(pages)} pages")
        if not blocks:
            return
        with self.lock:
            if self._kv_pool is not kv_pool or self.store_k is None:
                raise ValueError("APCManager.restore: these blocks were not stored from this KV pool")
            if any(blk.ref_cnt <= 0 or blk.key is None for blk in blocks):
                raise ValueError("APCManager.restore: blocks must be acquired (lookup_prefix) until their copies are enqueued")
            self._copy([blk.slot for blk in blocks], [int(p) for p in pages], kv_pool, to_store=False)

    def _copy(self, slots, pages, kv_pool, to_store: bool):
        dev = kv_pool.kpool.device
        si = h2d(np.asarray(slots, dtype=np.int64), dev)
        pi = h2d(np.asarray(pages, dtype=np.int64), dev)
        kv, vv = self._pool_views(kv_pool)
        if to_store:
            self.store_k.index_copy_(1, si, kv.index_select(1, pi))
            self.store_v.index_copy_(1, si, vv.index_select(1, pi))
        else:
            kv.index_copy_(1, pi, self.store_k.index_select(1, si))
            vv.index_copy_(1, pi, self.store_v.index_select(1, si))

    # ------------------------------------------------------------------ reporting / lifetime
    def _used(self) -> int:
        return sum(1 for blk in self.blocks if blk.key is not None)

    def resident_bytes(self) -> int:
        """bytes of K / V the table currently names (the store itself is allocated whole at first use)"""
        with self.lock:
            if self.store_k is None:
                return 0
            return 2 * self.store_k.shape[0] * self.store_k.shape[2] * self.store_k.element_size() * self._used()

    def stats_snapshot(self) -> dict:
        """the counters under the reference's key names.  matched_tokens (and so token_hit_rate) counts what LOOKUPS matched:
        tokens a generator then dropped under the length cap or the media rule are in it (see rejects_by_reason)."""
        with self.lock:
            snap = {name: int(self._n[name]) for name in _COUNTERS}
            snap.update((name, 0) for name in _UNBUILT_TIERS)
            seen = snap["matched_tokens"] + snap["served_tokens"]
            snap.update(block_size=self.block_size, num_blocks=self.num_blocks, pool_used=self._used(),
                        token_hit_rate=snap["matched_tokens"] / seen if seen else 0.0,
                        rejects_by_reason=dict(self._reject_reasons),
                        last_reject=None if self._last_reject is None else dict(self._last_reject),
                        resident_bytes=self.resident_bytes())
            return snap

    def reset_stats(self) -> None:
        with self.lock:
            self._reset_counters()

    def clear(self) -> None:
        """forget every block (ref counts included) and the counters; the device store stays allocated"""
        with self.lock:
            self._reset_table()
            self._reset_counters()

    def close(self) -> None:
        """drop the table and free the device store"""
        with self.lock:
            self.clear()
            self.store_k = self.store_v = None
            self._kv_pool = None
