"""Grammar-constrained generation (reference mlx_vlm/structured.py): a CPU matcher (llguidance) fills a packed bitmask of
the tokens its grammar allows next, and the device writes -inf over every other logit before the sampler runs.

The device half is `ops.apply_token_mask` (csrc/sample.hip::token_mask_kernel, the reference's `mlx_vlm_llguidance_mask`).
Masks are numpy `int32 [rows, ceil(V / 32)]`: bit `t & 31` of word `t >> 5` is token `t`, tokens past the mask are disallowed.

The MASK PROTOCOL: a logits processor with a method `prepare_next_token_mask(last_token) -> words | None` (the reference's
name, structured.py:113) is a *mask processor*.  `BatchGenerator` and `generate_step` never hand such a processor the
logits: after every step they call the method with the token just produced, stage the words into the device tables of the
captured step (vlm_penalty_args: slot 7 of row_params) and replay the graph - `None` means "no constraint this step".
Used as plain callables (`__call__`, `process_last_token`) the classes below work on device logits tensors through
`ops.apply_token_mask`.
"""
from __future__ import annotations

import json
from typing import Any, Optional

import numpy as np


def is_mask_processor(proc) -> bool:
    """the protocol above: the processor hands out packed token masks instead of editing logits"""
    return callable(getattr(proc, "prepare_next_token_mask", None))


def mask_words_of(words, max_words: Optional[int] = None) -> np.ndarray:
    """What a mask processor returned -> contiguous int32 [W] for ONE row (a [1, W] array, a [W] array, a tensor on either
    side; 32-bit integers of either signedness), cut to `max_words`: bits past the logits row select nothing."""
    if hasattr(words, "detach"):
        words = words.detach().cpu().numpy()
    w = np.asarray(words)
    if w.dtype.kind not in "iu" or w.dtype.itemsize != 4:
        raise TypeError(f"a token mask holds 32-bit words, not {w.dtype}")
    if w.ndim == 2 and w.shape[0] == 1:
        w = w[0]
    if w.ndim != 1:
        raise ValueError(f"a token mask of one row is [W] or [1, W] words, not {tuple(w.shape)}")
    w = np.ascontiguousarray(w).view(np.int32)
    return w if max_words is None else w[: int(max_words)]


def mask_allows_any(words: np.ndarray, vocab: int) -> bool:
    """does the mask leave at least one of the first `vocab` tokens?  (an all-zero mask would make the whole row -inf and its
    log-probs NaN: the host, which has the words, refuses it)"""
    full, rest = int(vocab) // 32, int(vocab) % 32
    w = words[:full + (1 if rest else 0)].view(np.uint32)
    if len(w) > full:
        return bool(w[:full].any()) or bool(int(w[full]) & ((1 << rest) - 1))
    return bool(w.any())


def call_processor(proc, tokens, logits, last_token: int):
    """One Python logits processor on the eager routes: through the reference's `process_last_token(last_token, logits)` where
    it has one (ar.py:1081: it keeps its own state and takes the new token only); a mask processor that is no callable through
    its mask; anything else as `proc(tokens, logits)`."""
    if hasattr(proc, "process_last_token"):
        return proc.process_last_token(int(last_token), logits)
    if not callable(proc) and is_mask_processor(proc):
        words = proc.prepare_next_token_mask(int(last_token))
        return logits if words is None else _apply_mask(logits, mask_words_of(words)[None])
    return proc(tokens, logits)


def _new_bitmask(rows: int, vocab: int) -> np.ndarray:
    """every token allowed until a matcher says otherwise"""
    return np.full((rows, (vocab + 31) // 32), -1, dtype=np.int32)


def _apply_mask(logits, words):
    """out of place, like the reference's kernel call: the caller's logits stay as they were"""
    from . import ops

    return ops.apply_token_mask(logits.clone(), words)


class LLGuidanceLogitsProcessor:
    """Logits processor backed by llguidance (reference structured.py:53-147), for one sequence or a batch: input_ids
    [seq] or [rows, seq], logits [V], [1, V] or [rows, V] (device tensors)."""

    # a constrained token is not held behind unrelated prefill work once it is decoded (reference structured.py:61-63)
    requires_immediate_decode_yield = True

    def __init__(self, grammar: str, llg_tokenizer) -> None:
        self.grammar = grammar
        self.llg_tokenizer = llg_tokenizer
        self.reset()

    def clone(self) -> "LLGuidanceLogitsProcessor":
        return LLGuidanceLogitsProcessor(self.grammar, self.llg_tokenizer)

    def reset(self):
        self.is_first_token = True
        self.ll_matchers = None
        self.bitmask = None
        self._mask_buffers = None
        self._mask_cursor = -1

    def _setup(self, batch_size: int) -> None:
        from llguidance import LLMatcher

        self.ll_matchers = [LLMatcher(self.llg_tokenizer, self.grammar) for _ in range(batch_size)]
        # two buffers in turn: the words handed out for one step stay as they are while the next step's are filled
        self._mask_buffers = [_new_bitmask(batch_size, self.llg_tokenizer.vocab_size) for _ in range(2)]
        self._mask_cursor = -1

    def _consume_tokens(self, last_tokens) -> None:
        for matcher, tok in zip(self.ll_matchers, last_tokens):
            matcher.consume_token(int(tok))
            err = matcher.get_error()
            if err:
                raise ValueError(f"LLGuidance matcher error: {err}")

    def _advance(self, batch_size: int, last_tokens) -> None:
        if self.is_first_token:
            self._setup(batch_size)
            self.is_first_token = False
        else:
            self._consume_tokens(last_tokens)

    def _fill_next_token_mask(self) -> np.ndarray:
        import llguidance.numpy

        self._mask_cursor = (self._mask_cursor + 1) % len(self._mask_buffers)
        self.bitmask = self._mask_buffers[self._mask_cursor]
        for i, matcher in enumerate(self.ll_matchers):
            llguidance.numpy.fill_next_token_bitmask(matcher, self.bitmask, i)
        return self.bitmask

    def prepare_next_token_mask(self, last_token: int) -> np.ndarray:
        """Advance the matcher of one sequence by the token just produced (nothing is consumed before the first token) and
        return the packed mask of the next one: int32 [1, ceil(vocab_size / 32)]."""
        self._advance(1, [last_token])
        return self._fill_next_token_mask()

    def process_last_token(self, last_token: int, logits):
        if logits.dim() == 1:
            return self.process_last_token(last_token, logits[None])[0]
        self._advance(logits.shape[0], [last_token])
        return _apply_mask(logits, self._fill_next_token_mask())

    def __call__(self, input_ids, logits):
        if logits.dim() == 1:
            return self(input_ids[None], logits[None])[0]
        if input_ids.dim() == 1 and logits.shape[0] == 1:
            input_ids = input_ids[None]
        self._advance(input_ids.shape[0], [] if self.is_first_token else input_ids[:, -1].tolist())
        return _apply_mask(logits, self._fill_next_token_mask())


class ThinkingAwareLogitsProcessor:
    """Keeps the wrapped processor out of the way while the model thinks (reference structured.py:150-248): a grammar
    constrains the answer, not the thinking tokens.  The wrapper stays inactive until it is shown the end-of-thinking token;
    the token sampled right after it is the first one the wrapped processor constrains."""

    def __init__(self, processor, tokenizer, thinking_start_token: str = "<think>", thinking_end_token: str = "</think>",
                 enable_thinking: bool = False) -> None:
        self.processor = processor
        self.tokenizer = tokenizer
        self.thinking_start_token = thinking_start_token
        self.thinking_end_token = thinking_end_token
        self.enable_thinking = enable_thinking
        self._active = not enable_thinking
        self._active_context: list = []
        self.thinking_start_token_id = tokenizer.encode(thinking_start_token, add_special_tokens=False)[-1]
        self.thinking_end_token_id = tokenizer.encode(thinking_end_token, add_special_tokens=False)[-1]
        if not is_mask_processor(processor):
            # the mask protocol is offered only over a processor that speaks it: a wrapper around a plain callable stays one
            self.prepare_next_token_mask = None

    @property
    def requires_immediate_decode_yield(self) -> bool:
        return bool(getattr(self.processor, "requires_immediate_decode_yield", False))

    def clone(self) -> "ThinkingAwareLogitsProcessor":
        inner = self.processor.clone() if hasattr(self.processor, "clone") else self.processor
        return ThinkingAwareLogitsProcessor(inner, self.tokenizer, self.thinking_start_token, self.thinking_end_token,
                                            self.enable_thinking)

    def reset(self):
        self._active = not self.enable_thinking
        self._active_context = []
        if hasattr(self.processor, "reset"):
            self.processor.reset()

    def _activate_if_thinking_done(self, token_id: int) -> bool:
        if self._active or token_id != self.thinking_end_token_id:
            return False
        self._active = True
        self._active_context = []
        return True

    def prepare_next_token_mask(self, last_token: int):
        """None ("no constraint this step") while thinking is open; from the end-of-thinking token on, the wrapped
        processor's mask - that token is the first one it is shown, and as its first call consumes nothing, the answer starts
        at the grammar's start."""
        if not self._active and not self._activate_if_thinking_done(int(last_token)):
            return None
        return self.processor.prepare_next_token_mask(last_token)

    def _delegate(self, last_token: int, logits):
        if hasattr(self.processor, "process_last_token"):
            return self.processor.process_last_token(last_token, logits)
        import torch

        self._active_context.append(int(last_token))
        return self.processor(torch.as_tensor(self._active_context, dtype=torch.int32, device=logits.device), logits)

    def process_last_token(self, last_token: int, logits):
        if not self._active and not self._activate_if_thinking_done(int(last_token)):
            return logits
        return self._delegate(last_token, logits)

    @staticmethod
    def _last_token_of(input_ids) -> Optional[int]:
        if input_ids.dim() == 0:
            return int(input_ids.item())
        if input_ids.shape[-1] == 0:
            return None
        return int(input_ids.reshape(-1, input_ids.shape[-1])[0, -1].item())

    def __call__(self, input_ids, logits):
        if not self._active:
            tok = self._last_token_of(input_ids)
            if tok is None or not self._activate_if_thinking_done(tok):
                return logits
        return self.processor(input_ids, logits)


def _serialize_schema(schema) -> str:
    return schema if isinstance(schema, str) else json.dumps(schema)


# an llguidance tokenizer walks the whole vocabulary when it is built (seconds for a 150k-token model): one per tokenizer
# object for the life of the process
_llg_tokenizer_cache: dict = {}


def build_json_schema_logits_processor(tokenizer, schema: "str | dict[str, Any]"):
    try:
        import llguidance as llg
        import llguidance.hf
    except ImportError as exc:
        raise ImportError("llguidance is required for structured response_format generation. "
                          "Install mlx-vlm with llguidance available.") from exc

    llg_tokenizer = _llg_tokenizer_cache.get(id(tokenizer))
    if llg_tokenizer is None:
        llg_tokenizer = _llg_tokenizer_cache[id(tokenizer)] = llguidance.hf.from_tokenizer(tokenizer)
    text = _serialize_schema(schema)
    if hasattr(llg, "JsonCompiler"):
        grammar = llg.JsonCompiler(separators=(", ", ": "), whitespace_pattern="").compile(text)
    else:
        grammar = llg.grammar_from("json_schema", text)
    return LLGuidanceLogitsProcessor(grammar, llg_tokenizer)
