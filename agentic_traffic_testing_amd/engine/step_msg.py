"""The step message rank 0 and the TP workers share, and the step variant decoded once.

``StepHeader`` is the message's 12-word int32 header as a record: ``words()`` and ``parse()``
are the only code that knows which word holds what.  ``SamplePlan`` is a step variant
(``variant_code``) decoded into the decisions the sampler tail takes
(``LlamaModel.sample_tail``).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from .. import ops

# step-message header (int32 words) shared by rank 0 and the TP workers
HDR_WORDS = 12
OP_STEP, OP_CAPTURE, OP_STOP, OP_BARRIER = 1, 2, 3, 4

# step variant (StepHeader.variant, third part of a graph key): bit 0 - some row samples with
# top-k / top-p (logits materialised); bits 1-2 - the logprob mode of the step's most demanding
# sequence; bit 3 - some sequence has a penalty or a logit bias (logits materialised, penalised
# into an fp32 buffer before the sampler, token counts updated after); bit 4 - some sequence is
# guided (logits materialised, masked into the fp32 buffer by its automaton state before the
# sampler, the state advanced after); bit 5 - a prefill step some of whose rows are scored for
# prompt logprobs (never a graph step: StepHeader.score_rows / score_topn)
V_TOPKP = 1
V_PENALTY = 8
V_GUIDE = 16
V_SCORE = 32
SCORE_TOPN = 1 << 30
LP_NONE, LP_SAMPLED, LP_TOPN = 0, 1, 2   # no logprobs / the sampled token's / + the top-N
TOP_N = ops.MAX_TOP_LOGPROBS             # a top-N step computes this many; requests cut theirs


def variant_code(topkp: bool, lp_mode: int, penalty: bool = False, guide: bool = False,
                 score: bool = False) -> int:
    return (int(bool(topkp)) | (lp_mode << 1) | (V_PENALTY if penalty else 0)
            | (V_GUIDE if guide else 0) | (V_SCORE if score else 0))


def variant_lp(variant: int) -> int:
    return (variant >> 1) & 3


class StepHeader(NamedTuple):
    """One message on the step channel: a step (OP_STEP: the shape of its ``MetaLayout`` and
    how to run it) or a control message (OP_CAPTURE: ``bucket``, ``num_parts``, ``variant``;
    OP_BARRIER, OP_STOP: the op alone)."""
    op: int
    T: int = 0
    S: int = 0
    W: int = 0
    NT: int = 0
    num_decode: int = 0
    num_parts: int = 0
    bucket: int = 0         # graph step: the batch bucket it replays from; 0: eager
    variant: int = 0
    n: int = 0              # sequences of the step (a graph step pads them to its bucket)
    size: int = 0           # int32 words of packed metadata behind the header
    score_rows: int = 0     # V_SCORE step: rows it scores ...
    score_topn: bool = False    # ... and whether some sequence wants the alternatives too
    max_qlen: int = 0       # verify step (speculative decoding): longest and shortest qlen;
    min_qlen: int = 0       # 0: a plain step

    def words(self) -> np.ndarray:
        """[op, T, S, W, NT, num_decode, num_parts, bucket-or-score-word, variant, n, size,
        verify-word]; OP_CAPTURE: [op, bucket, num_parts, variant, 0 ...].  A scoring step is
        never a graph step, so its word 7 holds score_rows | SCORE_TOPN; the verify word is
        max_qlen | min_qlen << 8."""
        if self.op == OP_CAPTURE:
            w = [self.op, self.bucket, self.num_parts, self.variant] + [0] * (HDR_WORDS - 4)
        else:
            w7 = self.bucket
            if self.variant & V_SCORE:
                w7 = self.score_rows | (SCORE_TOPN if self.score_topn else 0)
            w = [self.op, self.T, self.S, self.W, self.NT, self.num_decode, self.num_parts, w7,
                 self.variant, self.n, self.size, self.max_qlen | self.min_qlen << 8]
        return np.array(w, dtype=np.int32)

    @classmethod
    def parse(cls, words) -> "StepHeader":
        w = np.asarray(words[:HDR_WORDS]).tolist()
        if w[0] == OP_CAPTURE:
            return cls(w[0], bucket=w[1], num_parts=w[2], variant=w[3])
        h = cls(*w[:11], max_qlen=w[11] & 0xFF, min_qlen=w[11] >> 8)
        if h.variant & V_SCORE:
            h = h._replace(bucket=0, score_rows=h.bucket & (SCORE_TOPN - 1),
                           score_topn=bool(h.bucket & SCORE_TOPN))
        return h


class SamplePlan(NamedTuple):
    """A step variant decoded (``sample_plan``)."""
    topkp: bool
    lp_mode: int
    penalty: bool
    guide: bool
    score: bool
    # the logprob comes out of the fused LM head + sampler (the SAMPLE_LP epilogue): the
    # sampled token's alone, no top-k / top-p row, one GPU; every other logprob variant
    # materialises the logits for ``ops.token_logprobs``
    lp_fused: bool
    lp_top: int | None    # alternatives a materialised logprob step computes (None: no logprobs)
    # logits are materialised for top-k / top-p, penalties, guides and for every logprob the
    # fused sampler cannot record
    materialise: bool


@functools.lru_cache(maxsize=None)
def sample_plan(variant: int, tp_size: int = 1) -> SamplePlan:
    topkp, lp_mode = bool(variant & V_TOPKP), variant_lp(variant)
    penalty, guide = bool(variant & V_PENALTY), bool(variant & V_GUIDE)
    lp_fused = variant == variant_code(False, LP_SAMPLED) and tp_size == 1
    return SamplePlan(
        topkp, lp_mode, penalty, guide, bool(variant & V_SCORE), lp_fused,
        lp_top=None if lp_mode == LP_NONE else (TOP_N if lp_mode == LP_TOPN else 0),
        materialise=topkp or penalty or guide or (lp_mode != LP_NONE and not lp_fused))
