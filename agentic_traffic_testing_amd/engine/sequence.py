"""Request / sequence state for the serving engine."""
from __future__ import annotations

import enum
import itertools
import math
import time
from dataclasses import dataclass, field

import numpy as np


MAX_LOGPROBS = 20  # most alternatives per position (ops.MAX_TOP_LOGPROBS)
MAX_LOGIT_BIAS = 300  # most logit_bias entries per request (ops.PENALTY_BIAS_ENTRIES)


@dataclass
class SamplingParams:
    """Per-request sampling knobs.  The reference sends SamplingParams(temperature=0.2,
    max_tokens=...) to vLLM (llm/serve_llm.py:379, 520-525); top_p/top_k stay disabled by
    default like vLLM's defaults."""
    temperature: float = 0.2
    max_tokens: int = 512
    ignore_eos: bool = False
    seed: int | None = None
    stop_token_ids: tuple = ()
    top_p: float = 1.0
    top_k: int = -1
    # None: no logprobs; 0: the logprob of each sampled token; N in 1 .. 20: also the N most
    # likely tokens of each position (higher logit first, equal logits by lower id).  A logprob
    # is l_tok - logsumexp(l) in fp32 over the RAW logits the sampler sees - the LM-head product
    # rounded to the model dtype, before temperature, Gumbel noise and top-k / top-p (vLLM's
    # default "raw_logprobs").  Tokens do not depend on this field.
    logprobs: int | None = None
    # None: no prompt logprobs; 0: log p(prompt[i] | prompt[:i]) for every prompt token but the
    # first; N in 1 .. 20: also the N most likely tokens of each of those positions.  Defined as
    # ``logprobs`` is (raw logits rounded to the model dtype, fp32 log-softmax).  A request that
    # asks takes no prefix-cache hit until its prompt is scored: every position is computed.
    # Tokens do not depend on this field.
    prompt_logprobs: int | None = None
    # Penalties and bias (defaults: off).  For a sampled row, per token v, from the raw logit l
    # in fp32:  1. v occurs in the prompt or the tokens generated so far -> l = l / rep if l > 0
    # else l * rep;  2. c = times v was generated (the prompt does not count): l -= freq * c,
    # l -= pres * (c > 0);  3. l += logit_bias[v].  Temperature, noise and top-k / top-p run on
    # the result; logprobs stay raw.
    presence_penalty: float = 0.0      # in [-2, 2]
    frequency_penalty: float = 0.0     # in [-2, 2]
    repetition_penalty: float = 1.0    # > 0
    logit_bias: dict | None = None     # {token id: bias in [-100, 100]}, <= 300 entries
    # Guided decoding (at most one; defaults: off): the generated text must full-match the
    # regex / be one of the strings / be an instance of the JSON schema in canonical form
    # (engine/guided.py: dialect, schema subset).  Tokens the guide's automaton does not allow
    # are masked to -inf after the penalties and before temperature, noise and top-k / top-p;
    # the end token is allowed exactly where the text so far is a complete match.  Logprobs
    # stay raw.  With ignore_eos the guide never allows an end token.
    guided_regex: str | None = None
    guided_choice: list | None = None
    guided_json: dict | str | None = None

    @property
    def guided(self) -> bool:
        """Is one of the guide fields set?"""
        return (self.guided_regex is not None or self.guided_choice is not None
                or self.guided_json is not None)

    @property
    def penalised(self) -> bool:
        """Does any penalty or bias field differ from "off"?"""
        return (self.presence_penalty != 0.0 or self.frequency_penalty != 0.0
                or self.repetition_penalty != 1.0 or bool(self.logit_bias))

    def check(self, vocab_size: int | None = None) -> None:
        """Raise ValueError for a field the engine cannot serve (called when a request is
        added, where the vocabulary size that bounds the logit_bias keys is known)."""
        lp = self.logprobs
        if lp is not None and (isinstance(lp, bool) or not isinstance(lp, int)
                               or not 0 <= lp <= MAX_LOGPROBS):
            raise ValueError(f"logprobs must be None or an integer in 0 .. {MAX_LOGPROBS}, "
                             f"got {lp!r}")
        lp = self.prompt_logprobs
        if lp is not None and (isinstance(lp, bool) or not isinstance(lp, int)
                               or not 0 <= lp <= MAX_LOGPROBS):
            raise ValueError(f"prompt_logprobs must be None or an integer in 0 .. "
                             f"{MAX_LOGPROBS}, got {lp!r}")
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(self, name)
            if not _is_number(v) or not -2.0 <= v <= 2.0:
                raise ValueError(f"{name} must be a finite number in [-2, 2], got {v!r}")
        v = self.repetition_penalty
        if not _is_number(v) or not v > 0.0:
            raise ValueError(f"repetition_penalty must be a finite number > 0, got {v!r}")
        if self.guided:
            from .guided import guide_spec

            guide_spec(self)   # one field at most, each of its type
        lb = self.logit_bias
        if lb is None:
            return
        if not isinstance(lb, dict):
            raise ValueError(f"logit_bias must be None or a dict of token id -> bias, got {lb!r}")
        if len(lb) > MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias takes at most {MAX_LOGIT_BIAS} entries, got {len(lb)}")
        for k, b in lb.items():
            if isinstance(k, bool) or not isinstance(k, int) or k < 0 \
                    or (vocab_size is not None and k >= vocab_size):
                bound = "" if vocab_size is None else f" in 0 .. {vocab_size - 1}"
                raise ValueError(f"logit_bias keys must be integer token ids{bound}, got {k!r}")
            if not _is_number(b) or not -100.0 <= b <= 100.0:
                raise ValueError(f"logit_bias values must be finite numbers in [-100, 100], "
                                 f"got {b!r} for token {k}")


def _is_number(v) -> bool:
    """A finite int or float; bools are not numbers here."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        return False
    try:
        return math.isfinite(v)
    except OverflowError:  # an int too large for a float
        return False


class SeqStatus(enum.Enum):
    WAITING = 0
    RUNNING = 1
    FINISHED = 2


_ids = itertools.count(1)


@dataclass
class Sequence:
    request_id: str
    prompt_ids: list
    sampling: SamplingParams
    arrival_time: float = field(default_factory=time.perf_counter)
    seq_id: int = field(default_factory=lambda: next(_ids))
    output_ids: list = field(default_factory=list)
    status: SeqStatus = SeqStatus.WAITING
    num_computed: int = 0          # tokens whose KV is in the cache
    num_cached_prompt: int = 0     # prompt tokens served by the prefix cache
    first_scheduled_time: float | None = None
    first_token_time: float | None = None
    finish_time: float | None = None
    finish_reason: str | None = None
    seed: int = 0
    num_preemptions: int = 0
    # with sampling.logprobs set: one entry per entry of output_ids - the token's logprob, and
    # (logprobs >= 1) the position's [(id, logprob), ...] alternatives
    logprobs: list | None = None
    top_logprobs: list | None = None
    # with sampling.prompt_logprobs set: one entry per prompt token scored so far, in position
    # order - entry 0 is None (nothing precedes the first token), entry i the logprob of
    # prompt[i] given prompt[:i] and (prompt_logprobs >= 1) the position's alternatives
    prompt_logprobs: list | None = None
    prompt_top_logprobs: list | None = None
    # guided decoding: the compiled guide (engine/guided.py) and the host's shadow of the
    # automaton state - the table row after every token appended so far
    guide: object | None = None
    guide_state: int = 1
    _ids_np: np.ndarray | None = None

    @property
    def num_prompt(self) -> int:
        return len(self.prompt_ids)

    @property
    def num_tokens(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids)

    @property
    def num_pending(self) -> int:
        """Tokens whose KV still has to be computed (1 = decode step)."""
        return self.num_tokens - self.num_computed

    @property
    def finished(self) -> bool:
        return self.status == SeqStatus.FINISHED

    def token_array(self) -> np.ndarray:
        """All token ids as int64 numpy (cached; extended lazily)."""
        n = self.num_tokens
        a = self._ids_np
        if a is None or a.shape[0] != n:
            a = np.asarray(self.prompt_ids + self.output_ids, dtype=np.int64)
            self._ids_np = a
        return a

    def __post_init__(self):
        if self.sampling.logprobs is not None:
            self.logprobs = []
            self.top_logprobs = []

        if self.sampling.prompt_logprobs is not None:
            self.prompt_logprobs = [None]
            self.prompt_top_logprobs = [None]

    @property
    def scoring(self) -> bool:
        """Does this sequence still owe prompt logprobs?  Until it does not, it is admitted
        without the prefix cache, so that every prompt position has a hidden state."""
        return self.prompt_logprobs is not None and len(self.prompt_logprobs) < self.num_prompt

    def set_prompt_logprob(self, idx: int, lp: float, top) -> bool:
        """Record prompt token ``idx``'s logprob and alternatives (as ``set_logprob``'s).
        Entries are recorded once, in position order: any other ``idx`` is ignored (False)."""
        if self.prompt_logprobs is None or idx != len(self.prompt_logprobs) \
                or idx >= self.num_prompt:
            return False
        n = self.sampling.prompt_logprobs
        alts = [(int(i), float(v)) for i, v in zip(top[0][:n], top[1][:n])] if n else []
        self.prompt_logprobs.append(float(lp))
        self.prompt_top_logprobs.append(alts)
        return True

    def append(self, tok: int):
        self.output_ids.append(int(tok))
        self._ids_np = None

    def set_logprob(self, idx: int, lp: float, top) -> None:
        """Record output token ``idx``'s logprob and alternatives (ids, logprobs arrays; cut
        to the N this request asked for).  Positions are filled in order; ``idx`` below the
        length overwrites (a look-ahead placeholder's slot)."""
        if self.logprobs is None:
            return
        n = self.sampling.logprobs
        alts = [(int(i), float(v)) for i, v in zip(top[0][:n], top[1][:n])] if n else []
        del self.logprobs[idx:], self.top_logprobs[idx:]
        self.logprobs.append(float(lp))
        self.top_logprobs.append(alts)
