"""Draft proposers for speculative decoding (``EngineConfig.speculative``).

A proposer guesses the next tokens of a sequence; the engine runs the pending token and the
guesses through ONE decode step (``ModelRunner.verify``) and keeps the guesses that equal the
samples of their rows.  Sampling is a pure function of (logits, seed, step, token id), so what
is kept is exactly what plain decode would have produced: a proposer changes how many steps a
generation takes, never its tokens.
"""
from __future__ import annotations

import numpy as np


class Proposer:
    """Interface: ``propose(seq, k)`` returns at most ``k`` draft token ids (possibly none)
    that may follow ``seq.token_array()``."""

    def propose(self, seq, k: int) -> list:
        raise NotImplementedError


class NgramProposer(Proposer):
    """Prompt lookup: for n = n_max .. n_min take the last n tokens of prompt + output, find
    their most recent earlier occurrence and return up to k tokens that followed it.  The
    longest n with a match wins.  Agent answers quote their subtask, evaluators quote results
    and tool JSON is copied verbatim, so no second model is needed."""

    def __init__(self, n_max: int = 4, n_min: int = 2):
        if not 1 <= n_min <= n_max:
            raise ValueError("NgramProposer: 1 <= n_min <= n_max")
        self.n_max, self.n_min = n_max, n_min

    def propose(self, seq, k: int) -> list:
        if k <= 0:
            return []
        return self.lookup(seq.token_array(), k)

    def lookup(self, arr: np.ndarray, k: int) -> list:
        L = arr.shape[0]
        if k <= 0:
            return []
        for n in range(min(self.n_max, L - 1), self.n_min - 1, -1):
            # windows of n tokens that start before the tail's own start (each has at least one
            # token after it), compared with the tail in one vectorised pass
            win = np.lib.stride_tricks.sliding_window_view(arr[:L - 1], n)
            hit = np.flatnonzero((win == arr[L - n:]).all(axis=1))
            if hit.size:
                start = int(hit[-1]) + n
                return arr[start:start + k].tolist()
        return []


def make_proposer(cfg) -> Proposer | None:
    if cfg.speculative == "ngram":
        return NgramProposer(cfg.spec_ngram_max, cfg.spec_ngram_min)
    return None
