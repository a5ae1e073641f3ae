"""Continuous batching over the paged KV pool: `BatchGenerator` with the reference's interface
(mlx_vlm/generate/ar.py:2178-2887: insert / next / remove / stats / has_work, `GenerationBatch.Response` 937-943,
`PromptProgress` 906-913, finish rules 1313-1316).

What differs from the reference is the mechanism, not the contract.  The reference keeps one left-padded contiguous
KV tensor per layer for the whole batch and re-packs it whenever the membership changes (`filter` / `extend`,
cache.py:1100-1201).  Here every sequence owns pages of the pool; the batch owns a small block table with one row
per batch row, so

  * a finished request leaves by releasing its pages and, if it was not the last row, the last row takes its place:
    one table row and three 4-byte state words are copied - no KV bytes move and nothing is padded;
  * a new request joins after ONE varlen prefill launch over all admitted prompts (one ViT call over all their
    images), by writing its first sampled token / position / context length into the next free row.  That admission
    (ViT + prefill + first sample) is enqueued on a SECOND HIP stream: the running rows keep decoding underneath it
    and the new rows join at the first `next()` that finds its event complete (the reference alternates decode and
    prefill on one stream, ar.py:2705-2887, so every admission stalls the running rows).  Admissions run AHEAD of
    the free rows: up to `prefill_ahead` prefilled requests wait with their pages, so a row that finishes is refilled
    in the same `next()` call instead of idling for the length of a prefill;
  * a decode step is one hipGraph replay over the first 1, 2, 4 or 8 rows (the widths the weight-streaming kernels
    are built for); rows past the live ones point at a scratch page.  The engine keeps one graph per width.

The host never waits for the step in flight: `next()` returns the tokens that were the INPUTS of the step launched
by the previous call (their copy to pinned memory was enqueued before that step), then enqueues the next step - the
reference's `mx.async_eval` double buffering (ar.py:1044-1141), with the stop decision one step behind as there.
"""
from __future__ import annotations

import contextlib
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import h2d
from .models.cache import PAGE, PagedSequence
from .models.qwen2_vl.language import DecodeState
from .sample_utils import Sampler, make_sampler

_PROCS_KEY = "__logits_processors__"     # a request's LogitsProcessors spec inside its keyword arguments
_PYPROCS_KEY = "__py_logits_processors__"   # ... its Python callables (tokens, logits) -> logits (eager steps)
_BUDGET_KEY = "__thinking_budget_criteria__"   # ... its ThinkingBudgetCriteria
_MASKPROC_KEY = "__mask_logits_processor__"    # ... its mask processor (structured.py: prepare_next_token_mask), captured steps
_SAMPLER_KEY = "__sampler__"                   # ... its own sample_utils.Sampler (insert(..., samplers=)); absent: the generator's
MAX_ROWS = 16         # default widest decode step: one N tile of the skinny-M MFMA GEMM (csrc/gemv_mfma.hip), bf16 or 4-bit weights
WIDE_ROWS = 64        # on request (completion_batch_size > 16): WIDE steps of 32 / 64 rows on the prefill GEMMs (engine.hip decode_impl:
                      # 192.6 us per Qwen2-VL-7B layer at 32 rows, 210 at 64, against 120 per 16-row step - profiles/r03_mfma_shapes.txt)
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
MAX_TOP_LOGPROBS = 64  # top_logprobs_k: the selection kernel's cap (csrc/top_logprobs.hip)


class _NullEvent:
    """What the scheduler sees of a device event when no device is involved (the mock-engine tests on CPU, in the manner
    of the reference's scheduler tests with mock models, tests/test_generate.py:50-166, 529-1170)."""

    def record(self, *a):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


@dataclass
class PromptProgress:
    """reference ar.py:906-913"""
    uid: int
    prompt_tokens: int
    prompt_tps: float = 0.0
    prompt_time: float = 0.0
    cached_tokens: int = 0


@dataclass
class _Row:
    uid: int
    seq: PagedSequence
    max_tokens: int
    prompt_tokens: int
    num_tokens: int = 0
    procs: Any = None              # this request's sample_utils.LogitsProcessors (None: none)
    py_procs: Any = None           # its Python callables (tokens, logits) -> logits, in order (None: none)
    tokens: Any = None             # device int32 [n]: prompt + every token fed back (kept only for rows with py_procs)
    budget: Any = None             # its ThinkingBudgetCriteria (None: none)
    mask_proc: Any = None          # its mask processor (structured.is_mask_processor; None: none)
    mask_w: int = -1               # words of its token bitmask in slot 7 of its row of the device tables (-1: not written yet)


@dataclass
class _Admission:
    """A prefill in flight on the side stream: everything the join needs, kept alive until then."""
    batch: list
    caches: list
    lens: List[int]
    tok0: torch.Tensor
    lp0: Optional[torch.Tensor]
    state: torch.Tensor            # int32 [2, n]: rope position, context length
    event: torch.cuda.Event
    tic: float
    removed: set = field(default_factory=set)
    joined: int = 0                # requests of `batch` already given a row (a join takes as many as there are free rows)
    done_t: Optional[float] = None # host clock when the prefill's event was first seen fired (it may WAIT for a row after that)
    pen: Any = None                # device (hist, hist_len, params, bias_idx, bias_val) of the admitted requests, or None
    top0: Any = None               # top_logprobs_k > 0: (indices [n, k], values [n, k]) of the first tokens
    cached: Any = None             # apc_manager: tokens of each request restored from the prefix cache (PromptProgress.cached_tokens)

    def waiting(self) -> int:
        return sum(1 for b in self.batch[self.joined:] if b[0] not in self.removed)


@dataclass
class _APCPlan:
    """What an admission reuses of one request's prompt (apc.py)."""
    prefix_len: int                # tokens restored from the prefix cache (a multiple of PAGE; 0 = a cold request)
    blocks: list                   # the acquired blocks of that prefix, emptied when they are released
    extra_hash: int                # the request's image salt
    matched_tokens: int = 0        # what the lookup matched before the length cap and the media rule


_ADMISSION_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def _admission_stream(dev) -> "torch.cuda.Stream":
    """ONE side stream per device for the life of the process: the caching allocator keeps a pool per stream, so a fresh
    stream per generator would find no cached blocks and pay ~13 hipMalloc calls (tens of ms each) in its first admissions
    (profiles/r02_continuous_diag.txt)."""
    idx = torch.device(dev).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _ADMISSION_STREAMS:
        _ADMISSION_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return _ADMISSION_STREAMS[idx]


class BatchGenerator:
    """`insert(prompts)` queues token-id prompts (shortest first, ar.py:2620-2623); every `next()` reports one token
    per running request and advances the batch by one step.  `model` is the full `Model` (vision tower + language
    model): per-request `prompt_kwargs` carry `pixel_values` / `image_grid_thw` and the ViT runs inside the admission
    prefill.  Per-request logits processors (`insert(..., logits_processors=)`, ar.py:2584-2606): the reference's own
    four - logit_bias, repetition / presence / frequency penalty, as `make_logits_processors` specs - are applied by the
    device pass inside the captured step from per-row parameter tables; any other callable `(tokens, logits) -> logits`
    (and a Python `sampler(logprobs) -> tokens`) makes the steps EAGER while such a row is live: forward, the callables on
    the rows' logits as device tensors, sampling, advance - four host calls instead of one graph replay
    (ar.py:1044-1141).  `thinking_budget_criteria` per request (ar.py:1303-1350).  `kv_bits=8`: the uniform 8-bit KV
    cache with the reference's batch policy (every layer but the last of a stack deeper than 2, models/cache.py:8-21);
    as in the reference's batch path `quantized_kv_start` has no effect on the uniform scheme (ar.py:776-812: the batch
    caches are quantised from the first token).  `top_logprobs_k=k` (ar.py:2209; k <= 64): every Response carries the k best
    (token, log-prob) pairs of its token's log-prob row - after the logits processors, before the sampler's filters - in the
    reference's order (ops.top_logprobs), selected by one HIP launch behind every step.  `apc_manager=mgr` (ar.py:2214-2250;
    an `apc.APCManager`): automatic prefix caching for the Qwen2-VL family - at admission every request looks up the full 64-token
    blocks of its prompt (salted with its image); a request whose match leaves a text-only suffix is admitted WARM: the matched
    blocks are copied into its pages, only the suffix is embedded (no ViT call) and prefilled onto them, its queries attending
    straight over the pages (ops.attn_prefill_paged); after every admission the prompts' new full blocks are stored.  One manager
    may serve several generators of one model; `close()` leaves it open.  Not with kv_bits.  Speculative drafts are outside the
    built path and are rejected.

    Per-request samplers (`insert(..., samplers=)`; the reference's server hands the whole batch the sampler of whichever
    request opened it): from the first insert that names one, every step samples in ROW-TABLE mode - row r draws with its own
    line of the state's sampler workspace (temperature, top-p, min-p, top-k, seed and a draw counter; ops.sample_row_table),
    written when the request takes the row, moved with it, zeroed when it leaves - inside the captured step, whose launches
    do not depend on the lines.  What a seeded request can rely on: its n-th draw is keyed by (its seed, n, token index) -
    neither its row nor the generator's step counter enters - so GIVEN THE SAME LOG-PROB ROWS its tokens do not depend on the
    row it was given or on its neighbours, and a greedy request stays greedy whoever shares the batch.  The log-prob rows
    themselves come from different GEMV forms at different batch widths, so token equality of a whole run across widths (or
    against the request run alone) is not promised.  A generator that never sees `samplers` keeps the one shared sampler, its
    (seed, step, row, index) key and the launches it always had."""

    @dataclass
    class Response:
        uid: int
        token: int
        token_logprob: float
        finish_reason: Optional[str]
        top_logprobs: Optional[List[Tuple[int, float]]] = None

    def __init__(self, model, processor=None, *, max_tokens: int = 128, stop_tokens=None,
                 sampler: Optional[Sampler] = None, completion_batch_size: int = MAX_ROWS,
                 prefill_batch_size: int = MAX_ROWS, compute_logprobs: bool = True, use_graph: bool = True,
                 async_prefill: bool = True, prefill_ahead: int = 2, **kwargs):
        # uniform 8-bit KV cache (reference ar.py:2200-2230: BatchGenerator(kv_bits=, kv_group_size=, quantized_kv_start=)):
        # every admitted request's cache is quantised right after its prefill
        self.kv_bits = kwargs.pop("kv_bits", None)
        kv_group_size = kwargs.pop("kv_group_size", None) or 64
        kv_start = kwargs.pop("quantized_kv_start", None)
        kv_scheme = kwargs.pop("kv_quant_scheme", None)
        if self.kv_bits is not None:
            if float(self.kv_bits) != 8 or int(kv_group_size) != 64 or kv_scheme not in (None, "uniform"):
                raise NotImplementedError(f"BatchGenerator: kv_bits={self.kv_bits} kv_group_size={kv_group_size} "
                                          f"kv_quant_scheme={kv_scheme}: the uniform 8-bit / group-64 quantized KV cache is built")
            # quantized_kv_start: the reference's batch path builds BatchQuantizedKVCache for the uniform scheme whatever
            # the value (ar.py:776-812 - only the TurboQuant scheme defers on it), i.e. rows are quantised from their first
            # token; accepted and, as there, without effect
            if getattr(self.lm if hasattr(self, "lm") else model.language_model, "head_dim", 128) != 128:
                raise NotImplementedError("BatchGenerator(kv_bits=8): the 8-bit KV kernels are built for 128-wide heads")
        # top_logprobs_k (reference ar.py:2209): every Response carries the k best (token, log-prob) pairs of its token's row
        k = kwargs.pop("top_logprobs_k", None)
        k = 0 if k is None else k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"BatchGenerator: top_logprobs_k = {k!r}: an int >= 0")
        if k < 0:
            raise ValueError(f"BatchGenerator: top_logprobs_k = {k}: an int >= 0")
        if k > MAX_TOP_LOGPROBS:
            raise NotImplementedError(f"BatchGenerator: top_logprobs_k = {k}: at most {MAX_TOP_LOGPROBS} entries per token are built")
        self.top_logprobs_k = int(k)
        # automatic prefix caching (reference ar.py:2214-2250): an apc.APCManager, possibly shared with other generators
        self.apc_manager = kwargs.pop("apc_manager", None)
        if self.apc_manager is not None:
            if self.kv_bits is not None:
                raise NotImplementedError("BatchGenerator(apc_manager=, kv_bits=): the prefix cache holds bf16 pages; cached blocks "
                                          "of the 8-bit KV cache are not built")
            if int(getattr(self.apc_manager, "block_size", 0)) != PAGE:
                raise ValueError(f"BatchGenerator(apc_manager=): block_size must be {PAGE}, the KV pool's page")
            self._apc_check_engine(model)
        if kwargs.get("max_kv_size"):
            # reference ar.py:831-834 (to_batch_cache): make_prompt_cache's RotatingKVCache has keep = 4
            raise ValueError("RotatingKVCache with keep tokens is not supported.")
        unsupported = {k: v for k, v in kwargs.items() if v not in (None, False, 0, [], ())
                       and k not in ("prefill_step_size", "greedy_sampling", "stream")}
        if unsupported:
            raise NotImplementedError(f"BatchGenerator: outside the built path: {sorted(unsupported)}")
        self.model = model
        self.lm = model.language_model
        self.lm._batch_users = getattr(self.lm, "_batch_users", 0) + 1      # models with per-call global state (phi3_v's RoPE regime)
        self.processor = processor
        self.tokenizer = getattr(processor, "tokenizer", processor)
        self.max_tokens = max_tokens
        self.compute_logprobs = compute_logprobs
        self.use_graph = use_graph
        self.async_prefill = async_prefill
        self.prefill_ahead = max(0, int(prefill_ahead)) if async_prefill else 0
        max_rows = MAX_ROWS
        if int(completion_batch_size) > MAX_ROWS:      # wide steps: where the language model's engine has them
            max_rows = max(MAX_ROWS, min(WIDE_ROWS, int(getattr(self.lm, "MAX_DECODE_ROWS", MAX_ROWS))))
        pool_seqs = getattr(getattr(self.lm, "pool", None), "max_seqs", 64)
        while max_rows > 8 and pool_seqs < 2 * max_rows + 2:      # rows + admissions prefilled ahead + the scratch page each hold a sequence slot
            max_rows //= 2
        self.completion_batch_size = max(1, min(int(completion_batch_size), max_rows))
        self.prefill_batch_size = max(1, int(prefill_batch_size))
        # a sample_utils.Sampler samples on the device inside the captured step; any other callable is the reference's
        # `sampler(logprobs [n, V]) -> tokens [n]` contract and makes every step eager
        self._py_sampler = None
        if sampler is not None and (not isinstance(sampler, Sampler) or sampler.extended):
            # (a Sampler with the filters the captured step does not carry - sample_utils.Sampler.extended - is called on the
            # rows' log-probs like any callable: the same HIP kernel through vlm_sample_ex)
            if not callable(sampler):
                raise TypeError("sampler must be a mlx_vlm_amd.sample_utils.Sampler or a callable logprobs -> tokens")
            if isinstance(sampler, Sampler) and sampler.xtc_probability > 0.0:
                # the reference's apply_xtc takes its minimum over the WHOLE [rows, V] array and draws once per call
                # (sample_utils.py:371-376): across requests that is not a per-request filter; vlm_sample_ex serves one row
                raise NotImplementedError("xtc in the batch generator: the reference's filter mixes the rows of a batch; one row per call is built")
            self._py_sampler, sampler = sampler, None
        self.sampler = sampler or make_sampler()
        self._sargs = self.sampler.engine_args()
        self._row_sampling = False                    # row-table steps: set by the first insert(..., samplers=) that names a sampler
        crit = getattr(self.tokenizer, "stopping_criteria", None)
        self._stop = set(getattr(crit, "eos_token_ids", ()) or ())
        self._stop.update(int(t) for t in (stop_tokens or ()))
        self.uid_count = 0
        self._unprocessed_sequences: List[tuple] = []
        self._rows: List[_Row] = []
        self._closed = False

        # buffers are sized for the widest step that can run: 3 live rows decode inside a 4-wide step
        lm, dev, cap = self.lm, self.lm.device, next(w for w in WIDTHS if w >= self.completion_batch_size)
        self._cuda = torch.device(dev).type == "cuda"
        self._st = self._new_decode_state(cap)
        pool = lm.pool
        self._table = torch.zeros(cap, pool.max_pages, dtype=torch.int32, device=dev)
        self._scratch_seq = PagedSequence(pool)          # one page nobody reads: where idle rows write their k / v
        self._scratch_seq.reserve(1)
        self._idle_row = torch.full((pool.max_pages,), self._scratch_seq.pages[0], dtype=torch.int32, device=dev)
        self._table[:] = self._idle_row
        self._lp = torch.zeros(cap, dtype=torch.float32, device=dev)      # logprob of the token sitting in st.tok
        self._pin_tok = torch.empty(2, cap, dtype=torch.int32)
        self._pin_lp = torch.empty(2, cap, dtype=torch.float32)
        if self._cuda:
            self._pin_tok, self._pin_lp = self._pin_tok.pin_memory(), self._pin_lp.pin_memory()
        if self.top_logprobs_k:
            # the k best (index, log-prob) of the token sitting in st.tok, beside self._lp, and their two pinned slots
            self._top_idx, self._top_val = self._new_top_buffers(cap, self.top_logprobs_k)
            self._pin_top_idx = torch.empty(2, cap, self.top_logprobs_k, dtype=self._top_idx.dtype)
            self._pin_top_val = torch.empty(2, cap, self.top_logprobs_k, dtype=self._top_val.dtype)
            if self._cuda:
                self._pin_top_idx, self._pin_top_val = self._pin_top_idx.pin_memory(), self._pin_top_val.pin_memory()
        self._inflight: Optional[Tuple[int, torch.cuda.Event, List[int], float]] = None
        self._pending: List[_Admission] = []         # oldest first
        self._side = _admission_stream(dev) if (async_prefill and self._cuda) else None
        self._calls = 0
        self._unpipelined_steps = 0                   # steps that waited for their input tokens on the host (a mask row was live)
        self._idle_steps = 0
        self._width = 0

        self._prompt_tokens_counter = 0
        self._prompt_time_counter = 0.0
        self._gen_tokens_counter = 0
        self._gen_time_counter = 0.0
        self._steps_counter = 0
        # decode time = wall time with a step in flight: [launch, results back] of every step PLUS the host's share of the loop up
        # to the next launch (the steps are pipelined one ahead, so that share is hidden behind the GPU but it is decode time),
        # minus what a round spent blocked on a prefill
        self._t_results: Optional[float] = None
        self._blocked = 0.0

    # ------------------------------------------------------------------ engine hooks
    # (top_logprobs_k > 0 adds three, called only then: _new_top_buffers, _prefill_top_logprobs, _step_top_logprobs.)
    # Everything that touches the device sits behind these five methods; the scheduler (queue, admission, joins,
    # compaction, finish rules, stats) never looks past them, so it is driven by a mock engine in the CPU tests.
    def _event(self):
        return torch.cuda.Event() if self._cuda else _NullEvent()

    def _new_decode_state(self, cap: int):
        return self._borrow_state(self.lm, cap)

    def _sampler_lines(self) -> torch.Tensor:
        """int32 [cap, 8]: the rows' sampler lines of the row-table steps (engine hook: a view of the state's sampler workspace;
        a state without one - a mock engine - gets a host table)"""
        ws = getattr(self._st, "sample_ws", None)
        if ws is not None:
            return ops.sample_row_table(ws)
        if getattr(self, "_host_lines", None) is None:
            self._host_lines = torch.zeros(self._st.B, 8, dtype=torch.int32)
        return self._host_lines

    def _prefill_cold(self, batch):
        """One ViT call over all images of `batch`, one varlen prefill launch onto empty caches.
        -> (caches, lengths, logits of the last rows [n, V], rope deltas)"""
        from .generate import embed_requests

        lm = self.lm
        ids_l = [b[1] for b in batch]
        pix_l = [b[3].get("pixel_values") for b in batch]
        grid_l = [b[3].get("image_grid_thw") for b in batch]
        extras = [{k: v for k, v in b[3].items() if k not in ("pixel_values", "image_grid_thw", _PROCS_KEY, _PYPROCS_KEY, _BUDGET_KEY, _MASKPROC_KEY, _SAMPLER_KEY)}
                  for b in batch]
        ds = []                   # Qwen3-VL: the DeepStack rows of all requests, concatenated like their prompts
        emb, pos, lens, deltas = embed_requests(self.model, ids_l, pix_l, grid_l, extras, deepstack_out=ds)
        caches = []
        try:
            for L, b in zip(lens, batch):
                caches.append(lm.make_cache())
                caches[-1][0]._seq.reserve(L + b[2] + 2)          # prompt + every token it may generate + the step in flight
            logits = lm.prefill(emb, pos, caches, lens, "last", **({"deepstack": ds[0]} if ds else {}))
        except BaseException:
            self._release_caches(caches)             # (no sequence slot or page stays with a failed admission)
            raise
        return caches, list(lens), logits, list(deltas)

    @staticmethod
    def _release_caches(caches):
        for c in caches:
            if c is not None:
                c[0]._seq.release()

    def _prefill_warm(self, batch, plans):
        """Requests with a cached prefix (plans[i].prefix_len > 0): the matched blocks are copied into the first pages of each
        sequence, only the SUFFIX tokens are embedded - no ViT call, no pixel upload: a usable prefix covers every image span
        whole - and prefilled onto the pages in one launch chain, their queries attending straight over the pages
        (ops.attn_prefill_paged).  M-RoPE positions and the rope delta come from the FULL prompt and its grid.
        -> (caches, full prompt lengths, logits of the last rows [n, V], rope deltas)"""
        lm = self.lm
        caches, lens, deltas, embs, poss, sfx = [], [], [], [], [], []
        try:
            for b, pl in zip(batch, plans):
                ids = np.asarray(b[1]).reshape(1, -1)
                L, P = ids.shape[1], pl.prefix_len
                cache = lm.make_cache()
                seq = cache[0]._seq
                caches.append(cache)
                seq.reserve(L + b[2] + 2)
                self._apc_restore(seq, pl)
                grid = b[3].get("image_grid_thw")
                if b[3].get("pixel_values") is not None:
                    p, d = lm.get_rope_index(ids, np.asarray(grid), None, None)
                else:
                    p, d = lm.get_rope_index(ids)
                    p = np.broadcast_to(p[None], (3,) + p.shape)
                embs.append(lm.embed_tokens(ids[:, P:]).reshape(L - P, -1))
                poss.append(np.asarray(p).reshape(3, -1)[:, P:])
                sfx.append(L - P)
                lens.append(L)
                deltas.append(int(np.asarray(d).reshape(-1)[0]))
            logits = lm.prefill(torch.cat(embs, dim=0), np.concatenate(poss, axis=1), caches, sfx, "last", paged_attn=True)
        except BaseException:
            self._release_caches(caches)
            raise
        return caches, lens, logits, deltas

    def _prefill_logits(self, batch, plans):
        """-> (caches, lengths, last-row logits [n, V], rope deltas) of `batch` in request order.  Without a prefix-cache hit
        this is `_prefill_cold(batch)` - the calls and the launch of a generator without a manager; otherwise the cold and the
        warm requests run as two prefill calls and their rows are put back in request order."""
        warm = [i for i, pl in enumerate(plans) if pl is not None and pl.prefix_len > 0]
        if not warm:
            return self._prefill_cold(batch)
        cold = [i for i in range(len(batch)) if i not in set(warm)]
        n = len(batch)
        caches, lens, deltas, logits = [None] * n, [0] * n, [0] * n, None
        for idx, warm_part in ((cold, False), (warm, True)):
            if not idx:
                continue
            try:
                part = (self._prefill_warm([batch[i] for i in idx], [plans[i] for i in idx]) if warm_part
                        else self._prefill_cold([batch[i] for i in idx]))
            except BaseException:
                self._release_caches(caches)         # the half that had succeeded (each half releases its own on failure)
                raise
            c, l, lg, d = part
            if logits is None:
                V = lg.shape[1]
                logits = torch.empty(n, (V + 7) & ~7, dtype=lg.dtype, device=lg.device)[:, :V]      # pitch: see DecodeState
            logits[h2d(np.asarray(idx, dtype=np.int64), lg.device)] = lg
            for j, i in enumerate(idx):
                caches[i], lens[i], deltas[i] = c[j], l[j], d[j]
        return caches, lens, logits, deltas

    def _prefill_requests(self, batch):
        """One ViT call over all images of `batch`, one varlen prefill launch, first tokens sampled on the device (with a prefix
        cache: see `_prefill_logits`).
        -> (caches, lengths, first tokens int32 [n], their log-probs f32 [n] or None, int32 [2, n] rope position /
        context length of each request's first decode step)"""
        lm = self.lm
        masks = self._first_masks(batch)             # (host only, and first: a refused mask leaves no pages behind)
        plans = self._apc_plan(batch)
        self._last_cached = [pl.prefix_len for pl in plans] if self.apc_manager is not None else None
        try:
            caches, lens, logits, deltas = self._prefill_logits(batch, plans)
        finally:
            self._apc_release(plans)                 # (whatever a failed prefill left acquired)
        self._apc_commit(batch, caches, plans)
        # per-request logits processors on the FIRST token (ar.py:360-364: `tokens` is the prompt there): a history of each
        # admitted prompt + its parameter rows, applied by the device pass; the same rows move into the decode state at the join
        # a request's mask processor (structured.py) constrains the first token too: nothing consumed yet (`is_first_token`),
        # its mask rides in the same tables (slot 7 + the words behind the bias entries) and the same launch
        self._last_pen = None
        specs = [b[3].get(_PROCS_KEY) for b in batch]
        if any(specs) or any(b[3].get(_MASKPROC_KEY) is not None for b in batch):
            cap = self._st.hist.shape[1]
            host_h = np.zeros((len(batch), cap), dtype=np.int32)
            host_n = np.zeros(len(batch), dtype=np.int32)
            for r, b in enumerate(batch):
                t = np.asarray(b[1], dtype=np.int64).reshape(-1)[-cap:]
                host_h[r, :len(t)] = t
                host_n[r] = len(t)
            params, bidx, bval = DecodeState.pack_row_penalties(specs, cap, self._mask_words(), masks)
            dev = lm.device
            pen = tuple(h2d(x, dev) for x in (host_h, host_n, params, bidx, bval))
            from . import _lib
            pa = _lib.PenaltyArgs(pen[0].data_ptr(), pen[1].data_ptr(), cap, 0.0, 0, 0.0, 0, 0.0, 0, pen[3].data_ptr(),
                                  pen[4].data_ptr(), 0, pen[2].data_ptr(), bidx.shape[1])
            ops.apply_logit_penalties(logits, pa)
            self._last_pen = pen
        # RNG stream of the first tokens: the sampler keys its noise on (seed, step, row, index).  Decode steps count up
        # from 1 (see _borrow_state); every admission takes its own step value from a range they never reach, so no
        # (step, row) pair is used twice - neither between an admission and a decode step nor between two admissions
        self._admissions = getattr(self, "_admissions", 0) + 1
        step0 = torch.full((1,), 0x40000000 + (self._admissions & 0x3FFFFFFF), dtype=torch.int32, device=logits.device)
        for r, b in enumerate(batch):                   # Python callables on the first token: `tokens` = the prompt (ar.py:1959-1970)
            for proc in b[3].get(_PYPROCS_KEY) or ():
                tk = h2d(np.asarray(b[1], dtype=np.int32).reshape(-1), logits.device)
                logits[r:r + 1].copy_(self._call_proc(proc, tk, logits[r:r + 1], last_token=int(np.asarray(b[1]).reshape(-1)[-1])))
        if self._py_sampler is not None:
            _, lp = ops.sample(logits, want_logprobs=True, temperature=0.0)
            tok0 = self._call_sampler(lp)
        elif self._row_sampling:
            # every request's first token with its own line at count 0; the steps of its row go on from count 1 (_admit_join)
            lines = np.stack([self._sampler_of(b).row_line(0) for b in batch])
            tok0, lp = ops.sample_rows(logits, h2d(lines, logits.device), want_logprobs=True)
        else:
            tok0, lp = ops.sample(logits, step=step0, want_logprobs=self._want_rows(), **self._sargs)
        # top_logprobs_k > 0: the first tokens' log-prob rows stay here for `_prefill_top_logprobs`, which `_admit_begin` calls
        # right after this hook on the same stream (the 5-tuple below keeps its shape: the mock engines return it)
        self._last_lp_rows = lp if self.top_logprobs_k else None
        lp0 = lp.gather(1, tok0.long()[:, None]).reshape(-1).float() if self.compute_logprobs else None
        ctx = np.asarray(lens, dtype=np.int32)
        state = h2d(np.stack([ctx + np.asarray(deltas, dtype=np.int32), ctx]), lm.device)
        return caches, list(lens), tok0, lp0, state

    # ---- automatic prefix caching (apc.py).  `_apc_plan` / `_apc_restore` / `_apc_commit` are host logic + indexed copies on the
    # pool (they run on CPU pools under a mock engine); `_apc_check_engine` is the engine's part.  Every copy they enqueue lands
    # on the stream the admission runs on (`_admit_begin`: the side stream, or the current one) - the manager's stream invariant.
    def _apc_check_engine(self, model):
        """what the warm admission is built for: the Qwen2-VL family (suffix-only embedding, M-RoPE from the full prompt) on the
        128-wide heads of ops.attn_prefill_paged"""
        if not hasattr(model, "merge_input_ids_with_image_features"):
            raise NotImplementedError("BatchGenerator(apc_manager=): automatic prefix caching is built for the Qwen2-VL family; "
                                      f"{type(model).__module__} embeds its prompts through its own get_input_embeddings")
        lm = model.language_model
        if getattr(lm, "DEEPSTACK", False):
            raise NotImplementedError("BatchGenerator(apc_manager=): a warm admission skips the vision tower, and the DeepStack "
                                      "features of Qwen3-VL's image rows are not cached")
        if getattr(lm, "head_dim", 128) != 128:
            raise NotImplementedError("BatchGenerator(apc_manager=): the paged prefill attention is built for 128-wide heads")

    def _apc_plan(self, batch):
        """Per request: look its prompt up, apply the length cap and the media rule, release what is not used.
        -> one `_APCPlan` per request (None without a manager); the blocks of a plan with prefix_len > 0 stay acquired until
        `_apc_restore` has enqueued their copies."""
        mgr = self.apc_manager
        if mgr is None:
            return [None] * len(batch)
        from . import apc

        media = apc.media_token_ids(getattr(self.model, "config", None))
        plans = []
        for b in batch:
            ids = np.asarray(b[1], dtype=np.int64).reshape(-1)
            extra = apc.hash_image_payload(b[3].get("pixel_values"), b[3].get("image_grid_thw"))
            blocks, matched = mgr.lookup_prefix(ids, extra)
            prefix, why = apc.usable_prefix_len(len(ids), matched, apc.media_safe_prefix_min(ids, media), PAGE)
            if why is not None:
                mgr.record_reject(why, uid=b[0], matched_tokens=matched)
            keep = prefix // PAGE
            mgr.release(blocks[keep:])
            plans.append(_APCPlan(prefix, list(blocks[:keep]), extra, matched))
        return plans

    def _apc_restore(self, seq, plan):
        """the plan's blocks -> the first pages of `seq` (reserved by the caller), offset = prefix_len; the blocks are released:
        their copies are enqueued, and an eviction can only be enqueued behind them"""
        n = plan.prefix_len // PAGE
        self.apc_manager.restore(plan.blocks, seq.pages[:n], self.lm.pool)
        seq.set_offset(plan.prefix_len)
        self._apc_release([plan])

    def _apc_release(self, plans):
        for pl in plans:
            if pl is not None and pl.blocks:
                self.apc_manager.release(pl.blocks)
                pl.blocks = []

    def _apc_commit(self, batch, caches, plans):
        """after the admission's prefill is enqueued: count what was really prefilled and store every full block of the PROMPTS
        the manager does not hold yet (generated tokens are never stored)"""
        mgr = self.apc_manager
        if mgr is None:
            return
        for b, c, pl in zip(batch, caches, plans):
            ids = np.asarray(b[1], dtype=np.int64).reshape(-1)
            mgr.record_served(len(ids) - pl.prefix_len)
            mgr.store_pages(ids, c[0]._seq.pages, self.lm.pool, extra_hash=pl.extra_hash)

    def _decode_rows(self, width: int):
        """One decode step over rows 0..width-1 of the state: tok <- sampled token, pos and ctx advanced by one."""
        if self._py_sampler is not None or any(row.py_procs for row in self._rows):
            return self._decode_rows_eager(width)
        self.lm.decode_step_rows(self._st, width, self._table, self._sargs, use_graph=self.use_graph,
                                 with_logprobs=self._want_rows(),
                                 row_penalties=any(row.procs or row.mask_proc is not None for row in self._rows),
                                 q8=self.kv_bits is not None, **({"row_sampler": True} if self._row_sampling else {}))

    @staticmethod
    def _call_proc(proc, tokens, logits_row, last_token=None):
        """a Python callable on one logits row.  One that has the reference's `process_last_token(last_token, logits)` is called
        through it, as the reference's batch step does (ar.py:1081): it keeps its own state and wants the new token only."""
        from .structured import call_processor, is_mask_processor

        if last_token is None and (hasattr(proc, "process_last_token") or is_mask_processor(proc)):
            last_token = int(tokens[-1])
        out = call_processor(proc, tokens, logits_row, last_token)
        if not isinstance(out, torch.Tensor):
            out = torch.as_tensor(np.asarray(out), device=logits_row.device)
        return out.to(device=logits_row.device, dtype=logits_row.dtype).reshape(1, -1)

    def _call_sampler(self, logprobs):
        tok = self._py_sampler(logprobs)
        if not isinstance(tok, torch.Tensor):
            tok = torch.as_tensor(np.asarray(tok), device=logprobs.device)
        return tok.to(device=logprobs.device, dtype=torch.int32).reshape(-1).contiguous()

    def _decode_rows_eager(self, width: int):
        """The same step with the host in the middle (reference GenerationBatch._step, ar.py:1044-1141): forward of the rows
        (logits only), each row's device-side spec, then its Python callables on its logits row with its token context
        (prompt + every token fed, the one of this step included), log-probs, sampler (device or Python), advance."""
        lm, st, n = self.lm, self._st, len(self._rows)
        lm.decode_forward_rows(st, width, self._table, q8=self.kv_bits is not None)
        logits = st.logits[:width]
        if any(row.procs or row.mask_proc is not None for row in self._rows):
            ops.apply_logit_penalties(logits, st.row_penalty_tables(), push_tok=st.tok[:width])
        for r, row in enumerate(self._rows):
            if row.py_procs:
                row.tokens = torch.cat([row.tokens, st.tok[r:r + 1]])
                for proc in row.py_procs:
                    logits[r:r + 1].copy_(self._call_proc(proc, row.tokens, logits[r:r + 1]))
        if self._py_sampler is not None:
            _, lp = ops.sample(logits, want_logprobs=True, temperature=0.0)
            tok = torch.zeros(width, dtype=torch.int32, device=logits.device)
            tok[:n].copy_(self._call_sampler(lp[:n]))
        elif self._row_sampling:
            tok, lp = ops.sample_rows(logits, ws=st.sample_ws)      # the rows' lines where the captured step reads them; counts advance
        else:
            tok, lp = ops.sample(logits, step=st.step, want_logprobs=self._want_rows(), **self._sargs)
        st.tok[:width].copy_(tok)
        if lp is not None:
            st.logprobs[:width].copy_(lp)
        lm.decode_advance_rows(st, width)

    def _force_next_token(self, r: int, token: int):
        self._st.tok[r:r + 1].copy_(h2d(np.asarray([token], dtype=np.int32), self._st.tok.device))

    def _quantize_joined(self, seq):
        """the joined request's cached prompt becomes a QuantizedKVCache (engine hook: a mock engine has nothing to convert)"""
        self.lm.quantize_kv([seq], bits=int(self.kv_bits), group_size=64)
        seq.q8_batch_policy = True      # (the batch step keeps the last layer of a deep stack bf16: vlm_kv_pool.q8_skip_last)

    def _row_logprobs(self, n: int) -> torch.Tensor:
        """log-prob of the token each of the first n rows has just sampled (f32 [n])"""
        st = self._st
        return st.logprobs[:n].gather(1, st.tok[:n].long()[:, None]).reshape(-1).float()

    def _want_rows(self) -> bool:
        """the steps write the log-prob rows: for token_logprob, or for the top_logprobs selection"""
        return bool(self.compute_logprobs or self.top_logprobs_k)

    # ---- top_logprobs_k > 0 only (reference ar.py:1092-1122, 2051-2058: logprobs after the logits processors, before the
    # sampler's filters, no temperature; argsort ascending, the last k, reversed - ops.top_logprobs states the order)
    def _new_top_buffers(self, cap: int, k: int):
        """-> (int32 [cap, k], bf16 [cap, k]) on the engine's device: the list of the token sitting in st.tok of every row"""
        dev = self.lm.device
        return (torch.zeros(cap, k, dtype=torch.int32, device=dev), torch.zeros(cap, k, dtype=torch.bfloat16, device=dev))

    def _prefill_top_logprobs(self, batch):
        """-> (indices [n, k], values [n, k]) of the first tokens `_prefill_requests(batch)` has just sampled: the selection
        over the prefill's last-row log-probs, on the stream of the prefill.  Contract: called once, right after
        `_prefill_requests(batch)`, which leaves those rows (after the requests' processors) in `self._last_lp_rows`; an engine
        that replaces `_prefill_requests` replaces this hook too."""
        lp, self._last_lp_rows = getattr(self, "_last_lp_rows", None), None
        if lp is None or lp.shape[0] != len(batch):
            raise RuntimeError("BatchGenerator._prefill_top_logprobs: no log-prob rows of this batch - _prefill_requests leaves them "
                               "in self._last_lp_rows; an engine that overrides it overrides this hook as well")
        return ops.top_logprobs(lp, self.top_logprobs_k)

    def _step_top_logprobs(self, n: int):
        """rows 0..n-1 of the list buffers <- the selection over the log-prob rows of the step just enqueued (captured or
        eager): one launch behind it on the same stream, before the next step overwrites the rows"""
        ops.top_logprobs(self._st.logprobs[:n], self.top_logprobs_k, out=(self._top_idx[:n], self._top_val[:n]))

    @staticmethod
    def _borrow_state(lm, cap: int) -> DecodeState:
        """Decode states are carved from the model's bump arena (never returned): generators re-use a parked one."""
        parked = lm.__dict__.setdefault("_batch_states", [])
        for st in parked:
            if st.B == cap and not getattr(st, "in_use", False):
                break
        else:
            st = DecodeState(lm, cap)
            parked.append(st)
        st.in_use = True
        for buf in (st.tok, st.pos, st.ctx, st.step):
            buf.zero_()
        st.step.fill_(1)          # sampling step counter of the decode steps (0 is never used: see _prefill_requests)
        return st

    # ------------------------------------------------------------------ queue (reference ar.py:2584-2670)
    def insert(self, prompts, max_tokens=None, prompt_kwargs: Optional[List[dict]] = None, logits_processors=None,
               thinking_budget_criteria=None, samplers=None) -> List[int]:
        """logits_processors: one entry per prompt (reference ar.py:2584-2606) - None, a `sample_utils.LogitsProcessors`
        (what `make_logits_processors` returns here) or a list holding one; they run on the device inside the step, each
        row with its own parameters and token history.
        samplers: one entry per prompt - None (the generator's sampler) or a `sample_utils.Sampler` (`make_sampler`) with
        temperature, top_p, min_p, top_k and seed of its own; see the class docstring for what a seeded request can rely on."""
        if max_tokens is None or isinstance(max_tokens, int):
            max_tokens = [max_tokens or self.max_tokens] * len(prompts)
        if prompt_kwargs is None:
            prompt_kwargs = [{}] * len(prompts)
        if logits_processors is None:
            logits_processors = [None] * len(prompts)
        if thinking_budget_criteria is None:
            thinking_budget_criteria = [None] * len(prompts)
        if len(thinking_budget_criteria) != len(prompts):
            raise ValueError("Insufficient number of thinking_budget_criteria provided")
        if len(max_tokens) != len(prompts) or len(prompt_kwargs) != len(prompts) or len(logits_processors) != len(prompts):
            raise ValueError("max_tokens / prompt_kwargs / logits_processors must have one entry per prompt")
        if samplers is None:
            samplers = [None] * len(prompts)
        if len(samplers) != len(prompts):
            raise ValueError("samplers must have one entry per prompt")
        for s in samplers:
            if s is not None and (not isinstance(s, Sampler) or s.extended):
                raise NotImplementedError("insert(samplers=): a per-request sampler is a sample_utils.Sampler with top_p, min_p "
                                          "(min_tokens_to_keep = 1) and top_k - the three filters a row-table line carries; the "
                                          "extended filters and Python callables go to BatchGenerator(sampler=)")
        if any(s is not None for s in samplers) and self._py_sampler is not None:
            raise NotImplementedError("insert(samplers=) on a generator whose sampler is a Python callable or an extended Sampler")
        from .sample_utils import HIST_CAP, LogitsProcessors
        from .structured import is_mask_processor
        specs, pys, mps = [], [], []
        for lp in logits_processors:
            items = [x for x in (lp if isinstance(lp, (list, tuple)) else [lp]) if x]
            sp = [x for x in items if isinstance(x, LogitsProcessors)]
            py = [x for x in items if not isinstance(x, LogitsProcessors)]
            if len(sp) > 1:
                raise NotImplementedError("one make_logits_processors spec per request")
            # a mask processor (structured.py: prepare_next_token_mask) never sees the logits: its masks go into the row's
            # device tables and the steps stay captured.  Beside other Python callables of the same request it is one of them
            # (the eager step calls them in the caller's order); with a Python sampler the steps are eager anyway
            mp = [x for x in py if is_mask_processor(x)]
            if len(mp) > 1:
                raise NotImplementedError("one mask processor (prepare_next_token_mask) per request")
            if mp and len(py) == 1 and self._py_sampler is None:
                py = []
            else:
                mp = []
            mps.append(mp[0] if mp else None)
            for f in py:
                if not callable(f) and not is_mask_processor(f):
                    raise TypeError("logits_processors entries must be make_logits_processors specs or callables (tokens, logits) -> logits")
            if sp:
                DecodeState.pack_row_penalties(sp, HIST_CAP)                      # validates (bias list length) before queueing
            specs.append(sp[0] if sp else None)
            pys.append(py or None)
        uids = []
        if any(s is not None for s in samplers) and not self._row_sampling:
            self._begin_row_sampling()
        for p, m, kw, sp, py, crit, mp, smp in zip(prompts, max_tokens, prompt_kwargs, specs, pys, thinking_budget_criteria, mps,
                                                   samplers):
            ids = np.asarray(p, dtype=np.int64).reshape(-1)
            if ids.size == 0:
                raise ValueError("empty prompt")
            kw = dict(kw or {})
            if sp:
                kw[_PROCS_KEY] = sp               # travels with the request's keyword arguments (the queue item keeps its shape)
            if py:
                kw[_PYPROCS_KEY] = py
            if mp is not None:
                kw[_MASKPROC_KEY] = mp
            if crit is not None:
                kw[_BUDGET_KEY] = crit
            if smp is not None:
                kw[_SAMPLER_KEY] = smp
            self._unprocessed_sequences.append((self.uid_count, ids, int(m), kw))
            uids.append(self.uid_count)
            self.uid_count += 1
        self._unprocessed_sequences.sort(key=lambda x: len(x[1]))
        return uids

    def remove(self, uid) -> bool:
        for i, item in enumerate(self._unprocessed_sequences):
            if item[0] == uid:
                self._unprocessed_sequences.pop(i)
                return True
        for r, row in enumerate(self._rows):
            if row.uid == uid:
                self._drop_rows([r])
                return True
        for p in self._pending:                      # being prefilled / waiting for a row: dropped at the join
            if uid not in p.removed and any(b[0] == uid for b in p.batch[p.joined:]):
                p.removed.add(uid)
                return True
        return False

    @property
    def unprocessed_prompts(self):
        return self._unprocessed_sequences

    @property
    def has_pending_prompts(self) -> bool:
        return len(self._unprocessed_sequences) > 0 or bool(self._pending)

    @property
    def has_work(self) -> bool:
        return (bool(self._rows) or bool(self._unprocessed_sequences) or self._inflight is not None
                or any(p.waiting() for p in self._pending))

    def __len__(self):
        return len(self._rows)

    def stats(self):
        from .generate import BatchStats, _peak_gb

        s = BatchStats()
        s.prompt_tokens = self._prompt_tokens_counter
        s.prompt_time = self._prompt_time_counter
        s.prompt_tps = self._prompt_tokens_counter / self._prompt_time_counter if self._prompt_time_counter > 0 else 0
        s.generation_tokens = self._gen_tokens_counter
        s.generation_time = self._gen_time_counter
        s.generation_tps = self._gen_tokens_counter / self._gen_time_counter if self._gen_time_counter > 0 else 0
        s.peak_memory = _peak_gb()
        s.decode_steps = self._steps_counter       # (not a reference field: graph replays so far, for the roofline of a job)
        return s

    def close(self):
        if self._closed:
            return
        self._closed = True
        self.lm._batch_users = max(0, getattr(self.lm, "_batch_users", 1) - 1)
        if self._cuda:
            torch.cuda.synchronize()
        for p in self._pending:
            for c in p.caches[p.joined:]:
                c[0]._seq.release()
        self._pending = []
        for row in self._rows:
            row.seq.release()
        self._rows = []
        self._scratch_seq.release()
        self._inflight = None
        self._st.in_use = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ per-row logits processors (device tables of the state)
    def _set_row_penalties(self, r: int, pen, i: int, spec):
        """row r of the decode state <- request i of an admission (history of its prompt + its parameters; with a mask
        processor also slot 7 and the words of its first mask, which every later step replaces), or cleared"""
        st = self._st
        if spec and pen is not None:
            st.row_penalty_tables()
            st.hist[r].copy_(pen[0][i])
            st.hist_len[r:r + 1].copy_(pen[1][i:i + 1])
            st.row_params[r].copy_(pen[2][i])
            st.row_bias_idx[r].copy_(pen[3][i])
            st.row_bias_val[r].copy_(pen[4][i])
        elif getattr(st, "row_params", None) is not None:
            st.row_params[r].zero_()                  # the previous occupant's processors must not apply to this request
            st.hist_len[r:r + 1].zero_()

    def _move_row_penalties(self, dst: int, src: int):
        st = self._st
        if getattr(st, "row_params", None) is not None:
            for buf in (st.hist, st.row_params, st.row_bias_idx, st.row_bias_val):
                buf[dst].copy_(buf[src])
            st.hist_len[dst:dst + 1].copy_(st.hist_len[src:src + 1])

    # ------------------------------------------------------------------ per-row samplers (the lines of the row-table steps)
    def _sampler_of(self, item) -> Sampler:
        """the sampler of a queued request: its own, or the generator's"""
        return item[3].get(_SAMPLER_KEY) or self.sampler

    def _begin_row_sampling(self):
        """From here on the steps draw every row with its own line.  Rows already running get the generator's sampler with a
        fresh counter (written stream-ordered behind the step in flight, which still drew with the shared sampler)."""
        self._row_sampling = True
        lines = self._sampler_lines()
        lines.zero_()
        for r in range(len(self._rows)):
            self._set_row_line(r, self.sampler, 0)

    def _set_row_line(self, r: int, sampler: Sampler, count: int):
        lines = self._sampler_lines()
        lines[r].copy_(h2d(sampler.row_line(count), lines.device))

    # ------------------------------------------------------------------ token bitmasks of the mask rows (structured.py)
    def _finish_reason(self, row: _Row, tok: int, ahead: int = 0) -> Optional[str]:
        """the reference's finish rules (ar.py:1313-1316) for `tok` as token number row.num_tokens + ahead of its request"""
        return "stop" if tok in self._stop else "length" if row.num_tokens + ahead >= row.max_tokens else None

    def _vocab_size(self) -> int:
        """width of a logits row (engine hook)"""
        return int(self._st.logits.shape[1])

    def _mask_words(self) -> int:
        return DecodeState.mask_words_of(self._vocab_size())

    def _next_mask(self, proc, uid: int, token: int):
        """the matcher of request `uid` advanced by `token` -> the int32 words of its next mask, or None: no constraint"""
        from .structured import mask_allows_any, mask_words_of

        words = proc.prepare_next_token_mask(int(token))
        if words is None:
            return None
        words = mask_words_of(words, self._mask_words())
        if not mask_allows_any(words, self._vocab_size()):
            # the device would turn the whole row into -inf and its log-probs into NaN; the host has the words
            raise ValueError(f"request {uid}: its mask processor allows no token for the next step (an all-zero mask)")
        return words

    def _first_masks(self, batch):
        """per request of an admission: the words of its FIRST token's mask (nothing consumed: the processor's is_first_token
        call; it is handed the prompt's last token), or None"""
        out = []
        for b in batch:
            proc = b[3].get(_MASKPROC_KEY)
            out.append(None if proc is None else self._next_mask(proc, b[0], int(np.asarray(b[1]).reshape(-1)[-1])))
        return out

    def _stage_masks(self, n: int, toks):
        """toks[r]: the token row r feeds into the step about to be enqueued (host).  Every mask row's matcher consumes its
        token; the words go right-aligned into the row's line of a pinned buffer, one stream-ordered upload puts the lines
        into the bias_idx table behind the bias entries, and slot 7 of the rows whose word count changed is rewritten.  (The
        pinned lines are free again: the event this step waited on was recorded behind the previous upload.)  A row whose
        token ends its request is not advanced - the step's output for it is dropped - and runs unconstrained."""
        st, MW = self._st, self._mask_words()
        if getattr(self, "_pin_mask", None) is None:
            st.row_penalty_tables()
            self._pin_mask = torch.zeros(st.B, MW, dtype=torch.int32)
            self._pin_w = torch.zeros(st.B, dtype=torch.float32)
            if self._cuda:
                self._pin_mask, self._pin_w = self._pin_mask.pin_memory(), self._pin_w.pin_memory()
        lo, hi, changed = n, 0, False
        for r, row in enumerate(self._rows[:n]):
            w = 0
            if row.mask_proc is not None:
                words = None
                if self._finish_reason(row, int(toks[r]), ahead=1) is None:
                    words = self._next_mask(row.mask_proc, row.uid, int(toks[r]))
                if words is not None:
                    w = len(words)
                    self._pin_mask[r, MW - w:] = torch.from_numpy(words)
                    lo, hi = min(lo, r), r + 1
            changed = changed or w != row.mask_w
            row.mask_w = w
            self._pin_w[r] = w
        self._upload_masks(lo, hi, n if changed else 0)

    def _upload_masks(self, lo: int, hi: int, n_w: int):
        """lines lo..hi-1 of the pinned masks -> the rows' words in the device table; slot 7 of rows 0..n_w-1 (engine hook only
        in that it touches the state's tables: it runs on CPU tensors under a mock engine)"""
        st = self._st
        if hi > lo:
            st.row_bias_idx[lo:hi, st.row_bias_idx.shape[1] - self._pin_mask.shape[1]:].copy_(self._pin_mask[lo:hi], non_blocking=True)
        if n_w:
            st.row_params[:n_w, 7].copy_(self._pin_w[:n_w], non_blocking=True)

    # ------------------------------------------------------------------ membership
    def _drop_rows(self, gone: List[int]):
        """Release the sequences in batch rows `gone`; keep the live rows dense by moving rows from the end into the
        holes (stream-ordered after the step in flight)."""
        st = self._st
        gone_set = set(gone)
        for r in gone:
            self._rows[r].seq.release()
        live_after = len(self._rows) - len(gone)
        movers = [r for r in range(live_after, len(self._rows)) if r not in gone_set]
        holes = sorted(r for r in gone if r < live_after)
        for dst, src in zip(holes, movers):
            for buf in (st.tok, st.pos, st.ctx, self._lp) + ((self._top_idx, self._top_val) if self.top_logprobs_k else ()):
                buf[dst:dst + 1].copy_(buf[src:src + 1])
            self._table[dst].copy_(self._table[src])
            self._move_row_penalties(dst, src)
            if self._row_sampling:
                lines = self._sampler_lines()
                lines[dst].copy_(lines[src])
            self._rows[dst] = self._rows[src]
        del self._rows[live_after:]
        self._table[live_after:] = self._idle_row
        self._park_idle_rows()

    def _park_idle_rows(self):
        """Rows past the live ones keep running inside a 2/4/8-wide step: context 0 on the scratch page."""
        n = len(self._rows)
        if n < self._st.B:
            self._st.ctx[n:].zero_()
            self._st.pos[n:].zero_()
            self._st.tok[n:].zero_()
            if getattr(self._st, "row_params", None) is not None:
                self._st.row_params[n:].zero_()
            if self._row_sampling:
                self._sampler_lines()[n:].zero_()      # an idle row is a greedy row
        self._idle_steps = 0

    def _admit_begin(self):
        """Enqueue the prefill of as many queued prompts as there are free rows (one ViT call over all their images, one
        varlen prefill launch, first tokens sampled on the device) - on the side stream when async_prefill."""
        free = self.completion_batch_size - len(self._rows)
        ahead = sum(p.waiting() for p in self._pending)
        n = min(free + self.prefill_ahead - ahead, self.prefill_batch_size, len(self._unprocessed_sequences))
        if n <= 0:
            return
        batch, self._unprocessed_sequences = self._unprocessed_sequences[:n], self._unprocessed_sequences[n:]
        tic = time.perf_counter()
        where = contextlib.nullcontext()
        if self._side is not None:
            # pages released so far may still be written by steps already enqueued on the main stream
            gate = torch.cuda.Event()
            gate.record()
            self._side.wait_event(gate)
            where = torch.cuda.stream(self._side)
        with where:
            caches, lens, tok0, lp0, state = self._prefill_requests(batch)
            top0 = self._prefill_top_logprobs(batch) if self.top_logprobs_k else None
            ev = self._event()
            ev.record()
        self._pending.append(_Admission(batch, caches, lens, tok0, lp0, state, ev, tic, pen=getattr(self, "_last_pen", None),
                                        top0=top0, cached=getattr(self, "_last_cached", None)))
        self._last_pen = self._last_cached = None

    def _admit_join(self) -> List[PromptProgress]:
        """Give free rows to prefilled requests, oldest admission first; an admission whose event has not fired is
        waited for only when there is nothing to decode meanwhile."""
        st, lm = self._st, self.lm
        out: List[PromptProgress] = []
        while self._pending and len(self._rows) < self.completion_batch_size:
            p = self._pending[0]
            if not p.event.query():
                if self._side is not None and (self._rows or out):
                    break                             # keep decoding; it joins at a later round
                t_w = time.perf_counter()
                p.event.synchronize()                 # synchronous mode, or nothing to decode meanwhile
                self._blocked += time.perf_counter() - t_w
            if p.done_t is None:
                p.done_t = time.perf_counter()
            if self._cuda:
                torch.cuda.current_stream().wait_event(p.event)
            # wall time to the first token, as the reference reports it - up to the moment the prefill was seen complete: an
            # admission prefilled AHEAD under the decode steps then waits for rows, which is not prompt time
            dt = p.done_t - p.tic
            if p.joined == 0:
                self._prompt_tokens_counter += int(sum(p.lens))
                self._prompt_time_counter += dt
            while p.joined < len(p.batch) and len(self._rows) < self.completion_batch_size:
                i = p.joined
                p.joined += 1
                b, L, seq = p.batch[i], p.lens[i], p.caches[i][0]._seq
                if b[0] in p.removed:
                    seq.release()
                    continue
                r = len(self._rows)
                st.tok[r:r + 1].copy_(p.tok0[i:i + 1])
                st.pos[r:r + 1].copy_(p.state[0, i:i + 1])
                st.ctx[r:r + 1].copy_(p.state[1, i:i + 1])
                if p.lp0 is not None:
                    self._lp[r:r + 1].copy_(p.lp0[i:i + 1])
                if p.top0 is not None:
                    self._top_idx[r:r + 1].copy_(p.top0[0][i:i + 1])
                    self._top_val[r:r + 1].copy_(p.top0[1][i:i + 1])
                self._table[r].copy_(lm.pool.block_table[seq.seq])
                if self.kv_bits is not None:
                    self._quantize_joined(seq)          # KVCache.to_quantized right after the prefill (stream-ordered)
                spec = b[3].get(_PROCS_KEY)
                mproc = b[3].get(_MASKPROC_KEY)
                self._set_row_penalties(r, p.pen, i, spec or mproc is not None)
                if self._row_sampling:
                    self._set_row_line(r, self._sampler_of(b), 1)      # (draw 0 was the first token, _prefill_requests)
                py = b[3].get(_PYPROCS_KEY)
                self._rows.append(_Row(uid=b[0], seq=seq, max_tokens=b[2], prompt_tokens=L, procs=spec, py_procs=py,
                                       tokens=h2d(np.asarray(b[1], dtype=np.int32).reshape(-1), lm.device) if py else None,
                                       budget=b[3].get(_BUDGET_KEY), mask_proc=mproc))
                out.append(PromptProgress(uid=b[0], prompt_tokens=L, prompt_tps=L / dt if dt > 0 else 0.0, prompt_time=dt,
                                          cached_tokens=int(p.cached[i]) if p.cached else 0))
            if p.joined >= len(p.batch):
                self._pending.pop(0)
            elif not p.waiting():                     # only removed requests left
                for c in p.caches[p.joined:]:
                    c[0]._seq.release()
                self._pending.pop(0)
        return out

    # ------------------------------------------------------------------ one scheduling round
    def next(self):
        """-> (prompt_responses, generation_responses), reference ar.py:2705-2887."""
        responses: List[BatchGenerator.Response] = []
        if self._inflight is not None:
            slot, ev, uids, t_launch = self._inflight
            self._inflight = None
            ev.synchronize()
            self._t_results = time.perf_counter()
            self._gen_time_counter += self._t_results - t_launch
            toks, lps = self._pin_tok[slot].numpy(), self._pin_lp[slot].numpy()
            if self.top_logprobs_k:
                top_i, top_v = self._pin_top_idx[slot].numpy(), self._pin_top_val[slot].float().numpy()
            live = {row.uid: r for r, row in enumerate(self._rows)}
            gone = []
            for i, uid in enumerate(uids):
                r = live.get(uid)
                if r is None:                      # removed by the caller since the snapshot
                    continue
                row = self._rows[r]
                row.num_tokens += 1
                tok = int(toks[i])
                reason = self._finish_reason(row, tok)
                if row.budget is not None:
                    # ar.py:1306-1314,1338-1347: the criteria sees the reported token; a pending forced id REPLACES the next
                    # token of the row - already sampled by the step in flight, so the write is stream-ordered behind it
                    row.budget(tok)
                    forced = row.budget.pop_forced_token_id()
                    if forced is not None and reason is None:
                        self._force_next_token(r, int(forced))
                if reason is not None:
                    gone.append(r)
                top = list(zip(top_i[i].tolist(), top_v[i].tolist())) if self.top_logprobs_k else None
                responses.append(self.Response(uid, tok, float(lps[i]) if self.compute_logprobs else 0.0, reason, top))
            self._gen_tokens_counter += len(responses)
            if gone:
                self._drop_rows(gone)
        now = time.perf_counter()
        for p in self._pending:                      # (polled once per round: the granularity of prompt_time is one decode step)
            if p.done_t is None and p.event.query():
                p.done_t = now
        if self._side is None:
            self._admit_begin()                      # synchronous mode: prefill, join, then decode (the reference's order)
            self._blocked += time.perf_counter() - now
        prompt_responses = self._admit_join()
        if self._rows:
            self._launch_step()
        self._t_results, self._blocked = None, 0.0
        if self._side is not None:
            self._admit_begin()                      # under the step just enqueued
        return prompt_responses, responses

    def _launch_step(self):
        st, n = self._st, len(self._rows)
        width = next(w for w in WIDTHS if w >= n)
        if width != self._width or self._idle_steps >= 4 * PAGE:
            self._width = width
            self._park_idle_rows()
        slot = self._calls & 1
        self._calls += 1
        self._pin_tok[slot, :n].copy_(st.tok[:n], non_blocking=True)
        if self.compute_logprobs:
            self._pin_lp[slot, :n].copy_(self._lp[:n], non_blocking=True)
        if self.top_logprobs_k:
            self._pin_top_idx[slot, :n].copy_(self._top_idx[:n], non_blocking=True)
            self._pin_top_val[slot, :n].copy_(self._top_val[:n], non_blocking=True)
        ev = self._event()
        ev.record()
        if any(row.mask_proc is not None for row in self._rows):
            # a mask row is live: this step is NOT enqueued behind the one in flight.  Its mask depends on the token that step
            # is sampling, so: results back (the copy above), every mask row's matcher advanced on the host, the masks staged
            # and uploaded, then the replay - the host round trip the reference pays too (its processors carry
            # requires_immediate_decode_yield, ar.py:2709-2730).  The next next() finds the event fired and reports the tokens
            ev.synchronize()
            self._unpipelined_steps += 1
            self._stage_masks(n, self._pin_tok[slot].numpy())
        t_launch = time.perf_counter()
        if self._t_results is not None:              # the loop went straight from the last step's results to this launch
            self._gen_time_counter += max(0.0, t_launch - self._t_results - self._blocked)
        self._inflight = (slot, ev, [row.uid for row in self._rows], t_launch)
        longest = max(row.prompt_tokens + row.max_tokens for row in self._rows) + 2
        # (16-row steps keep the single-pass attention: the split merge lives in the o_proj prologue of the <= 8-row GEMV)
        st.nsplit = 1 if longest <= 2048 or width > 8 else max(2, min(32, (longest + 16 * PAGE - 1) // (16 * PAGE)))
        self._decode_rows(width)
        if self.compute_logprobs:
            self._lp[:n].copy_(self._row_logprobs(n))
        if self.top_logprobs_k:
            self._step_top_logprobs(n)
        for row in self._rows:
            row.seq.offset += 1
        self._idle_steps += 1
        self._steps_counter += 1


def generate_batch_continuous(model, input_ids_list, pixel_values_list, grids, *, max_tokens=128, stop_ids=(),
                              sampler: Optional[Sampler] = None, batch_size: int = MAX_ROWS, use_graph: bool = True,
                              extras: Optional[List[Optional[dict]]] = None, logits_processors=None, kv_bits=None,
                              samplers=None):
    """The reference's `_generate_batch` loop (ar.py:3212-3232) over the continuous generator: every request is queued
    at once, the generator keeps up to `batch_size` of them decoding and admits the next ones as rows free up.
    extras: per-request keyword arguments of the model's `get_input_embeddings` besides pixels / grid (phi3_v: image_sizes).
    logits_processors: one `make_logits_processors` spec (or None) per request, or ONE spec for all of them.
    kv_bits: 8 = every request's cache is a QuantizedKVCache from its first decode step on (BatchGenerator(kv_bits=8)).
    samplers: one `make_sampler` spec (or None: `sampler`) per request - BatchGenerator.insert(..., samplers=).
    -> (tokens per request without the stop token, BatchStats)"""
    gen = BatchGenerator(model, None, max_tokens=max(max_tokens) if isinstance(max_tokens, (list, tuple)) else max_tokens,
                         stop_tokens=set(stop_ids), sampler=sampler,
                         completion_batch_size=batch_size, prefill_batch_size=batch_size, compute_logprobs=False,
                         use_graph=use_graph, kv_bits=kv_bits)
    kw: List[Dict[str, Any]] = [dict(pixel_values=p, image_grid_thw=g) if p is not None else {}
                                for p, g in zip(pixel_values_list, grids)]
    for k, e in zip(kw, extras or []):
        if e and "pixel_values" in k:
            k.update(e)
            if k.get("image_grid_thw") is None:
                del k["image_grid_thw"]
    if logits_processors is not None and not isinstance(logits_processors, (list, tuple)):
        logits_processors = [logits_processors] * len(input_ids_list)
    uids = gen.insert([np.asarray(i).reshape(-1) for i in input_ids_list], max_tokens, prompt_kwargs=kw,
                      logits_processors=logits_processors, **({"samplers": samplers} if samplers is not None else {}))
    results = {u: [] for u in uids}
    tic = time.perf_counter()
    while gen.has_work:
        _, out = gen.next()
        for r in out:
            if r.finish_reason != "stop":
                results[r.uid].append(r.token)
    total = time.perf_counter() - tic
    stats = gen.stats()               # generation_time: wall time with decode steps in flight (prefills admitted under them included)
    gen.close()
    stats.wall_time = total
    return [results[u] for u in uids], stats
