"""The model runner's step records (engine/step_msg.py, engine/model_runner.py): the step
header's wire layout, the decoded step variant, the order of the one sampler tail and the slot
pool - all on the host."""
import itertools

import pytest

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.engine import model_runner as mr
from agentic_traffic_testing_amd.engine.model_runner import (
    LP_NONE, LP_SAMPLED, LP_TOPN, OP_BARRIER, OP_CAPTURE, OP_STEP, OP_STOP, SamplePlan, SlotPool,
    StepHeader, sample_plan, variant_code)
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from test_guided import engine, prompts

H = StepHeader
# (record, its 12 words: [op, T, S, W, NT, num_decode, num_parts, bucket-or-score-word, variant,
# n, size, verify-word]; OP_CAPTURE: [op, bucket, parts, variant, 0 ...])
HEADERS = {
    "eager": (H(OP_STEP, 37, 3, 16, 2, 1, 1, 0, 3, 3, 214),
              [1, 37, 3, 16, 2, 1, 1, 0, 3, 3, 214, 0]),
    "graph": (H(OP_STEP, 8, 8, 16, 0, 8, 4, 8, 24, 5, 250),
              [1, 8, 8, 16, 0, 8, 4, 8, 24, 5, 250, 0]),
    "score": (H(OP_STEP, 12, 1, 16, 1, 0, 1, 0, 32, 1, 90, score_rows=5),
              [1, 12, 1, 16, 1, 0, 1, 5, 32, 1, 90, 0]),
    "score_topn": (H(OP_STEP, 12, 1, 16, 1, 0, 1, 0, 34, 1, 90, score_rows=5, score_topn=True),
                   [1, 12, 1, 16, 1, 0, 1, 5 | 1 << 30, 34, 1, 90, 0]),
    "verify": (H(OP_STEP, 7, 3, 16, 0, 3, 2, 0, 0, 3, 120, max_qlen=4, min_qlen=1),
               [1, 7, 3, 16, 0, 3, 2, 0, 0, 3, 120, 4 | 1 << 8]),
    "capture": (H(OP_CAPTURE, bucket=8, num_parts=4, variant=16),
                [2, 8, 4, 16, 0, 0, 0, 0, 0, 0, 0, 0]),
    "stop": (H(OP_STOP), [3] + [0] * 11),
    "barrier": (H(OP_BARRIER), [4] + [0] * 11),
}


@pytest.mark.parametrize("name", list(HEADERS))
def test_header_round_trip_and_wire_layout(name):
    hdr, words = HEADERS[name]
    w = hdr.words()
    assert w.dtype.name == "int32" and w.shape == (mr.HDR_WORDS,) and mr.HDR_WORDS == 12
    assert w.tolist() == words
    assert StepHeader.parse(w) == hdr
    # a worker parses the whole message: the payload behind the header is not the header's
    assert StepHeader.parse(words + [7, 7, 7]) == hdr


def test_header_overloads_decode_to_fields_of_their_own():
    s = StepHeader.parse(HEADERS["score_topn"][1])
    assert (s.bucket, s.score_rows, s.score_topn) == (0, 5, True)
    assert StepHeader.parse(HEADERS["score"][1]).score_topn is False
    v = StepHeader.parse(HEADERS["verify"][1])
    assert (v.max_qlen, v.min_qlen, v.bucket, v.score_rows) == (4, 1, 0, 0)
    g = StepHeader.parse(HEADERS["graph"][1])
    assert (g.bucket, g.num_parts, g.variant, g.max_qlen) == (8, 4, 24, 0)
    with pytest.raises(AttributeError):
        g.bucket = 4    # frozen


def test_sample_plan_truth_table():
    fused = []
    for tp in (1, 2):
        for topkp, lp, pen, gd in itertools.product((False, True),
                                                    (LP_NONE, LP_SAMPLED, LP_TOPN),
                                                    (False, True), (False, True)):
            variant = variant_code(topkp, lp, pen, gd)
            plan = sample_plan(variant, tp)
            assert isinstance(plan, SamplePlan)
            assert (plan.topkp, plan.lp_mode, plan.penalty, plan.guide, plan.score) == \
                (topkp, lp, pen, gd, False)
            # the rule, written out: only the sampled token's logprob, with nothing else asked
            # of the step, on one GPU, comes out of the fused LM head + sampler
            lp_fused = (lp == LP_SAMPLED and not topkp and not pen and not gd and tp == 1)
            assert plan.lp_fused is lp_fused
            assert plan.lp_top == {LP_NONE: None, LP_SAMPLED: 0, LP_TOPN: mr.TOP_N}[lp]
            assert plan.materialise is bool(topkp or pen or gd
                                            or (lp != LP_NONE and not lp_fused))
            if plan.lp_fused:
                fused.append((variant, tp))
    assert fused == [(2, 1)]
    assert len({variant_code(*c) for c in itertools.product(
        (False, True), (0, 1, 2), (False, True), (False, True))}) == 24
    # a scoring step's sampler is its variant's without the bit - but for the fused logprob,
    # which only the exact variant 2 has
    s = sample_plan(variant_code(True, LP_TOPN, score=True), 1)
    assert s.score and s[:4] == sample_plan(variant_code(True, LP_TOPN), 1)[:4]
    assert not sample_plan(variant_code(False, LP_SAMPLED, score=True), 1).lp_fused


TAIL = ["penalty_apply", "guide_apply", "sample", "penalty_update", "guide_advance",
        "token_logprobs"]


def test_sampler_tail_order(monkeypatch):
    eng = engine(model="tiny", max_model_len=64, num_kv_blocks=16, guided_pool_states=64)
    log = []

    def logged(name, fn):
        def call(*a, **kw):
            log.append(name)
            return fn(*a, **kw)
        return call

    for name in TAIL + ["sample_topkp", "decode_lm_head_sample"]:
        monkeypatch.setattr(ops, name, logged(name, getattr(ops, name)))
    sp = SamplingParams(temperature=0.0, max_tokens=40, guided_regex=r"[0-9]{4}", logprobs=2,
                        frequency_penalty=2.0, presence_penalty=2.0, repetition_penalty=1.5)
    steps0 = eng.runner.steps
    out = eng.generate([prompts(hi=4000)[0]], sp)[0]
    steps = eng.runner.steps - steps0
    assert out.finish_reason == "stop" and 2 <= len(out.token_ids) <= steps
    assert log == TAIL * steps


def test_slot_pool():
    pool = SlotPool("penalty", 3)
    assert [pool.acquire(s) for s in (10, 11, 12)] == [(0, True), (1, True), (2, True)]
    assert pool.acquire(11) == (1, False)       # the same sequence again: its slot, not fresh
    with pytest.raises(RuntimeError, match="no free penalty slot: a finished, aborted or "
                                           "preempted sequence was not released"):
        pool.acquire(13)
    pool.release(11)
    pool.release(11)                            # releasing twice gives the slot back once
    pool.release(99)                            # a sequence that never had one
    assert pool.free == [1] and pool.slots == {10: 0, 12: 2}
    assert pool.acquire(13) == (1, True)        # the released slot is reused
    with pytest.raises(RuntimeError, match="no free guide slot"):
        SlotPool("guide", 0).acquire(1)
