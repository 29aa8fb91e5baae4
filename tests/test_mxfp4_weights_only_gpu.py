"""The MXFP4 weights-only mode on the GPU: the engine holds the layer projections in 4 bits
alone (load and memory), and its tokens - 4-bit GEMV rows, wide 4-bit rows, expand + library
rows, decode graphs on the wide 4-bit kernels - against the teacher-forced dense oracle built
from ``model.dense_weight``, and against a default-mode mxfp4 engine where both run the same
library plan on the same values."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams

from helpers import dense_logits
from test_spec_decode import ReplayProposer, run_engine, runs_of

pytestmark = pytest.mark.gpu

PROJS = ("qkv", "o", "gate_up", "down")


def _engine(**kw):
    gc.collect()  # engines of earlier tests go now, not while this one captures a hipGraph
    base = dict(model="small", device="cuda", max_model_len=512, num_kv_blocks=512,
                max_num_seqs=8, graph_batch_sizes=(1, 2, 4, 8), quantization="mxfp4")
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _dense_oracle(model):
    """What tests/helpers.dense_logits reads of a model, with every projection a dense 16-bit
    copy from ``dense_weight`` - the engine itself keeps none."""
    layers = [SimpleNamespace(input_norm=L.input_norm, post_norm=L.post_norm,
                              **{p: model.dense_weight(i, p) for p in PROJS})
              for i, L in enumerate(model.layers)]
    return SimpleNamespace(cfg=model.cfg, embed=model.embed, head_dim=model.head_dim,
                           n_heads=model.n_heads, n_kv_heads=model.n_kv_heads,
                           cos_sin=model.cos_sin, g=model.g, scale=model.scale, norm=model.norm,
                           lm_head=model.lm_head, layers=layers)


def _oracle_check(oracle, prompts, sps, outs, tol_logit=0.25):
    """The rule of test_engine._check: every generated position teacher-forced on the engine's
    own prefix; a token that is not the oracle's argmax must be a near tie (gap < tol_logit),
    and at most one position in five may differ at all."""
    bad = checked = 0
    for p, sp_, o in zip(prompts, sps, outs):
        assert len(o.token_ids) == sp_.max_tokens
        ids = list(p)
        for got_t in o.token_ids:
            lg = dense_logits(oracle, ids)
            checked += 1
            if int(torch.argmax(lg)) != got_t:
                gap = float(lg.max() - lg[got_t])
                assert gap < tol_logit, (o.token_ids, len(ids) - len(p), gap)
                bad += 1
            ids.append(got_t)
    assert bad <= max(1, checked // 5), (bad, checked)


def _holds_4_bits_only(eng):
    m = eng.runner.model
    assert m.quant == "mxfp4" and m.w4_only
    nk = 0
    for L in m.layers:
        for proj in PROJS:
            assert getattr(L, proj) is None and getattr(L, proj + "_ps") is None
            wq, sq = getattr(L, proj + "_w4"), getattr(L, proj + "_b4")
            assert wq.dtype == sq.dtype == torch.uint8 and wq.shape[1] == 16 * sq.shape[1]
            nk = max(nk, wq.shape[0] * wq.shape[1] * 2)
    # embedding, final norm and LM head stay 16-bit
    assert m.embed.dtype == m.norm.dtype == m.lm_head.dtype == m.dtype
    assert m.w4_scratch.dtype == m.dtype and m.w4_scratch.numel() * 2 == 2 * nk
    assert m.w4_scratch.numel() == 5632 * 1024  # the small model's gate_up
    return 2 * nk


def _spies(m):
    """Record (op, rows, wide_w4) of the fused qkv calls, the rows of every forward and the
    expand calls; returns (log, undo)."""
    log = {"qkv": [], "forward": [], "expand": 0}
    real_qkv, real_expand, real_forward = ops.decode_qkv_rope, ops.expand_mxfp4, m.forward

    def qkv(x, *a, **kw):
        log["qkv"].append((x.shape[0], bool(kw.get("wide_w4")), kw.get("w_block_scale") is not None))
        return real_qkv(x, *a, **kw)

    def expand(*a, **kw):
        log["expand"] += 1
        return real_expand(*a, **kw)

    def forward(ids, *a, **kw):
        log["forward"].append(ids.shape[0])
        return real_forward(ids, *a, **kw)

    ops.decode_qkv_rope, ops.expand_mxfp4, m.forward = qkv, expand, forward

    def undo():
        ops.decode_qkv_rope, ops.expand_mxfp4 = real_qkv, real_expand
        del m.forward

    return log, undo


def test_load_and_memory():
    """(a) No layer holds a 16-bit projection, the scratch is exactly 2 * max(N * K) bytes, and
    the device memory in use after load is below a default-mode engine's by at least the
    default engine's 16-bit projections minus the scratch."""
    kw = dict(startup_warmup=False, use_graphs=False)
    torch.cuda.synchronize()
    dflt = _engine(**kw)
    torch.cuda.synchronize()
    used_default = torch.cuda.memory_allocated()
    dense16 = sum(getattr(L, p).numel() * getattr(L, p).element_size()
                  for L in dflt.runner.model.layers for p in PROJS)
    assert dflt.runner.resident_weights["scratch"] == 0
    del dflt
    gc.collect()
    eng = _engine(mxfp4_weights_only=True, **kw)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated()
    scratch = _holds_4_bits_only(eng)
    rw = eng.runner.resident_weights
    assert rw["scratch"] == scratch and rw["fp8"] == 0
    assert rw["codes4"] * 4 == dense16 and rw["scales4"] * 64 == dense16
    print(f"memory_allocated default {used_default} weights-only {used} "
          f"16-bit projections {dense16} scratch {scratch}")
    assert used_default - used >= dense16 - scratch, (used_default, used, dense16, scratch)
    assert eng.runner.model.step_plan(64).qkv == "fused"
    assert eng.runner.model.step_plan(300).qkv == "lib"


def test_tokens_against_the_dense_oracle():
    """(b) A 17-row and a 30-row prompt (4-bit GEMV), a 100-row prefill (the wide kernel's
    4-bit builds) and a 300-row prefill (expand + the library plan), each alone in its step."""
    eng = _engine(mxfp4_weights_only=True, max_num_batched_tokens=512)
    _holds_4_bits_only(eng)
    m = eng.runner.model
    oracle = _dense_oracle(m)
    rng = np.random.default_rng(11)
    sp_ = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    log, undo = _spies(m)
    try:
        for n in (17, 30, 100, 300):
            del log["qkv"][:], log["forward"][:]
            log["expand"] = 0
            prompts = [rng.integers(300, 30000, size=n).tolist()]
            outs = eng.generate(prompts, sp_)
            if n <= 32:
                assert (n, True, True) in log["qkv"] and log["expand"] == 0, log
            elif n == 100:  # the wide 4-bit route, unpadded, nothing expanded
                assert 100 in log["forward"] and (100, True, True) in log["qkv"], log
                assert log["expand"] == 0
            else:  # no fused qkv at these rows: every projection of every layer expanded
                assert any(t >= 300 for t in log["forward"]), log
                assert not any(rows >= 300 for rows, _, _ in log["qkv"]), log
                assert log["expand"] > 0 and log["expand"] % (4 * len(m.layers)) == 0, log
            _oracle_check(oracle, prompts, [sp_], outs)
    finally:
        undo()


def test_decode_graphs_past_32_rows_run_the_wide_4bit_kernels():
    """(b) The 40-sequence run of test_mxfp4_gpu.test_engine_crosses_between_4bit_and_16bit_decode:
    decode starts in graph bucket 64 - here on the wide kernel's 4-bit builds, there being no
    16-bit projection to run - and comes back to the 4-bit GEMV."""
    nseq = 40
    rng = np.random.default_rng(nseq)
    prompts = [rng.integers(300, 30000, size=int(n)).tolist()
               for n in rng.integers(3, 30, size=nseq)]
    sps = [SamplingParams(temperature=0.0, max_tokens=2 + i % 5, ignore_eos=True)
           for i in range(nseq)]
    eng = _engine(mxfp4_weights_only=True, num_kv_blocks=2048, max_num_seqs=nseq,
                  max_num_batched_tokens=4096, graph_batch_sizes=(1, 2, 4, 8, 16, 32, 64))
    _holds_4_bits_only(eng)
    m = eng.runner.model
    assert m.decode_step_fusable(nseq) and m.decode_step_fusable(64)
    assert m._w4_rows(32) and m._w4_rows(33) and m._w4_rows(128) and not m._w4_rows(129)
    assert m._decode_w(m.layers[0], "qkv", 64)["wide_w4"] is True
    r = eng.runner
    rows = []  # the graph bucket (= rows of the captured step) of every decode step
    graph_bucket = r.graph_bucket

    def spy(batch):
        b = graph_bucket(batch)
        rows.append(b)
        return b

    r.graph_bucket = spy
    try:
        outs = eng.generate(prompts, sps)
    finally:
        del r.graph_bucket
    assert 64 in rows and any(0 < b <= 32 for b in rows), sorted(set(rows))
    assert rows.index(64) < max(i for i, b in enumerate(rows) if 0 < b <= 32)
    assert r.graph_steps > 0
    _oracle_check(_dense_oracle(m), prompts, sps, outs)


def test_expand_rows_equal_the_default_mode_engine():
    """(c) A default-mode mxfp4 engine without pre-shuffled copies runs a 300-row prefill on
    the library plan over its stored dequantised weights; the weights-only engine runs the same
    plan over the same values expanded into its scratch, and the decode steps of both stream
    the same 4-bit copies: the greedy tokens are equal."""
    kw = dict(max_num_batched_tokens=512, preshuffle_decode_weights=False, startup_warmup=False)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(300, 30000, size=300).tolist()]
    sp_ = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    dflt = _engine(**kw)
    assert dflt.runner.model.layers[0].qkv_ps is None
    plan = dflt.runner.model.step_plan(300)
    want = [o.token_ids for o in dflt.generate(prompts, sp_)]
    del dflt
    eng = _engine(mxfp4_weights_only=True, **kw)
    _holds_4_bits_only(eng)
    assert eng.runner.model.step_plan(300) == plan
    got = [o.token_ids for o in eng.generate(prompts, sp_)]
    assert got == want


def test_speculative_verify_steps_go_past_32_rows():
    """The verify-row cap of the mode is the wide kernel's, not the 4-bit GEMV's: 10 sequences
    with 3 drafts each make 40-row verify steps (default-mode mxfp4 trims them to 32,
    test_mxfp4_gpu.test_engine_speculative_equals_plain_decode).  Drafts replay a plain run
    with every fifth token corrupted: accepted and rejected drafts, every position checked
    against the dense oracle."""
    rng = np.random.default_rng(7)
    prompts = [rng.integers(300, 30000, size=n).tolist() * 5
               for n in (6, 9, 5, 11, 7, 8, 10, 6, 12, 4)]
    sp_ = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True)
    kw = dict(mxfp4_weights_only=True, max_num_seqs=10, graph_batch_sizes=(1, 2, 4, 8, 16))
    base, _ = run_engine(_engine(**kw), prompts, sp_)
    eng = _engine(speculative="ngram", spec_tokens=4, **kw)
    _holds_4_bits_only(eng)
    r = eng.runner
    assert r.spec_tokens == 3 and 40 <= r.verify_rows() <= 128, r.verify_rows()
    seen = []
    verify = r.verify

    def spy(batch, drafts):
        seen.append(sum(int(q) for q in batch.q_len))
        return verify(batch, drafts)

    r.verify = spy
    try:
        eng.proposer = ReplayProposer(runs_of(base), corrupt_every=5, vocab=30000)
        res, _ = run_engine(eng, prompts, sp_)
    finally:
        del r.verify
    assert seen and max(seen) == 40, seen
    assert 0 < eng.spec_stats["accepted_tokens"] < eng.spec_stats["draft_tokens"]
    outs = [SimpleNamespace(token_ids=res[f"r{i}"]["tokens"]) for i in range(len(prompts))]
    _oracle_check(_dense_oracle(r.model), prompts, [sp_] * len(prompts), outs)
