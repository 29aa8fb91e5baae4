"""MXFP4 W4A8 prefill (mxfp4_fp8_activations) without a GPU: the CPU reference of
ops.gemm_w4a8 against an fp64 product on hand-built codes and scales, the configuration
switch, its rows of the step plan, and the CPU engine - the reference arithmetic of the mode -
against the dense oracle of tests/w4a8_oracle.py."""
import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import MODEL_PRESETS, EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.models import step_plan as sp
from agentic_traffic_testing_amd.models.llama import LlamaModel
from agentic_traffic_testing_amd.ops import reference as ref

import w4a8_oracle as wo


def hand_built(N, K, M, seed=0):
    """Codes cycling through all 16 e2m1 values (distinct along both axes), a scale byte per
    block from 125..129 that depends on (n, k / 32), integer activations in [-4, 4] as e4m3 and
    power-of-two row scales.  Returns (codes, scales, xq, xs, fp64 product of the values)."""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = ((3 * n + 5 * k + seed) % 16).to(torch.uint8)
    scales = (125 + (2 * n + 3 * (k[:, ::32] // 32) + seed) % 5).to(torch.uint8)
    xi = ((7 * torch.arange(M)[:, None] + 3 * k + seed) % 9 - 4).float()
    xq = xi.to(torch.float8_e4m3fn).view(torch.uint8)
    xs = torch.tensor([2.0 ** ((m % 5) - 2) for m in range(M)])
    mag = torch.tensor(ref.E2M1_VALUES, dtype=torch.float64)[(codes & 7).long()]
    w = torch.where(codes >= 8, -mag, mag)
    w = w * torch.pow(2.0, scales.double() - 127).repeat_interleave(32, 1)
    y = (xi.double() @ w.t()) * xs.double()[:, None]
    return codes, scales, xq, xs, y


@pytest.mark.parametrize("rowmap,N", [("plain", 96), ("qkv", 256), ("silu", 64), ("silu", 256)])
def test_cpu_reference_matches_fp64(rowmap, N):
    K, M = 256, 7
    codes, scales, xq, xs, y = hand_built(N, K, M, seed=N)
    wq, sq = ops.preshuffle_mxfp4(codes, scales, rowmap)
    assert float(y.abs().max()) > 0
    # every product is a multiple of 2^-3 times the row scale and the sums are far below 2^24
    # of them: fp32 is exact, the result is the fp64 product rounded once to bf16
    got = ops.gemm_w4a8(xq, xs, wq, sq, rowmap)
    assert got.dtype == torch.bfloat16 and got.shape == (M, N)
    assert torch.equal(got, y.to(torch.bfloat16))
    assert torch.equal(ops.gemm_w4a8(xq, xs.reshape(-1, 1), wq, sq, rowmap), got)
    out = torch.empty(M, N, dtype=torch.bfloat16)
    assert ops.gemm_w4a8(xq, xs, wq, sq, rowmap, out=out) is out and torch.equal(out, got)
    if rowmap == "silu":
        inter = N // 2
        want = (torch.nn.functional.silu(y[:, :inter]) * y[:, inter:])
        got = ops.gemm_w4a8(xq, xs, wq, sq, rowmap, ops.GEMM_SILU)
        assert got.shape == (M, inter) and got.dtype == torch.bfloat16
        # silu in fp32 against fp64: one bf16 ulp of slack on top of the rounding
        err = (got.double() - want).abs()
        assert bool((err <= want.abs() * 2.0 ** -7 + 1e-6).all()), float(err.max())


def test_op_refuses_what_it_cannot_run():
    codes, scales, xq, xs, _ = hand_built(64, 256, 3)
    wq, sq = ops.preshuffle_mxfp4(codes, scales)
    with pytest.raises(ValueError):
        ops.gemm_w4a8(xq[:, :128], xs, wq, sq, "plain")        # K of x and of the codes differ
    with pytest.raises(ValueError):
        ops.gemm_w4a8(xq, xs, wq, sq, "plain", ops.GEMM_SILU)  # SiLU needs the silu rowmap
    with pytest.raises(ValueError):
        ops.gemm_w4a8(xq, xs, wq, sq, "plain", ops.GEMM_RESADD)
    with pytest.raises(ValueError):
        ops.gemm_w4a8(xq, xs, wq[:16], sq[:16], "plain")       # N % 32
    with pytest.raises(ValueError):
        ops.gemm_w4a8(xq, xs, wq, sq, "diagonal")
    assert ops.gemm_w4a8_shape_ok(4096, 6144, ops.GEMM_PLAIN, "qkv")
    assert ops.gemm_w4a8_shape_ok(4096, 28672, ops.GEMM_SILU, "silu")
    assert ops.gemm_w4a8_shape_ok(14336, 4096, ops.GEMM_PLAIN)
    assert not ops.gemm_w4a8_shape_ok(4096 + 64, 4096)
    assert not ops.gemm_w4a8_shape_ok(4096, 4096 + 16)
    assert not ops.gemm_w4a8_shape_ok(4096, 4096 + 32, ops.GEMM_PLAIN, "qkv")
    assert not ops.gemm_w4a8_shape_ok(4096, 4096, ops.GEMM_RESADD)
    assert not ops.gemm_w4a8_shape_ok(4096, 4096, ops.GEMM_SILU, "plain")


def test_config_refuses_the_flag_without_mxfp4():
    for quant in ("", "fp8"):
        with pytest.raises(ValueError, match="mxfp4_fp8_activations"):
            EngineConfig(quantization=quant, mxfp4_fp8_activations=True)
        with pytest.raises(ValueError, match="mxfp4_fp8_activations"):
            LlamaModel(MODEL_PRESETS["tiny"], device="cpu", quantization=quant,
                       mxfp4_fp8_activations=True)
    assert not EngineConfig(quantization="mxfp4").mxfp4_fp8_activations
    # both memory modes take it
    assert EngineConfig(quantization="mxfp4", mxfp4_fp8_activations=True).mxfp4_fp8_activations
    cfg = EngineConfig(quantization="mxfp4", mxfp4_fp8_activations=True, mxfp4_weights_only=True)
    assert cfg.mxfp4_fp8_activations and cfg.mxfp4_weights_only


def test_config_from_env_and_serve_flag(monkeypatch):
    from agentic_traffic_testing_amd.serving import serve_llm

    monkeypatch.setenv("LLM_QUANTIZATION", "mxfp4")
    assert not EngineConfig.from_env().mxfp4_fp8_activations
    monkeypatch.setenv("LLM_MXFP4_FP8_ACTIVATIONS", "1")
    assert EngineConfig.from_env().mxfp4_fp8_activations
    monkeypatch.setenv("LLM_MXFP4_FP8_ACTIVATIONS", "0")
    assert not EngineConfig.from_env().mxfp4_fp8_activations
    monkeypatch.delenv("LLM_MXFP4_FP8_ACTIVATIONS")
    base = ["--model", "tiny", "--device", "cpu", "-q", "mxfp4"]
    assert not serve_llm.build_config(serve_llm.make_parser().parse_args(base)).mxfp4_fp8_activations
    cfg = serve_llm.build_config(
        serve_llm.make_parser().parse_args(base + ["--mxfp4-fp8-activations"]))
    assert cfg.mxfp4_fp8_activations and not cfg.mxfp4_weights_only
    cfg = serve_llm.build_config(serve_llm.make_parser().parse_args(
        base + ["--mxfp4-fp8-activations", "--mxfp4-weights-only"]))
    assert cfg.mxfp4_fp8_activations and cfg.mxfp4_weights_only
    monkeypatch.setenv("LLM_QUANTIZATION", "fp8")
    monkeypatch.setenv("LLM_MXFP4_FP8_ACTIVATIONS", "1")
    with pytest.raises(ValueError, match="mxfp4_fp8_activations"):
        EngineConfig.from_env()


def _facts(**kw):
    base = dict(gpu=True, quant="mxfp4", wdtype=torch.bfloat16, tp_size=1, preshuffled=True,
                hidden=4096, q_width=4096, kv_width=1024, inter=14336, gemm_tuned=True)
    base.update(kw)
    return sp.StepFacts(**base)


CHAIN = sp.StepPlan(sp.GEMM_W4A8, sp.GEMM_W4A8, sp.GEMM_W4A8, sp.GEMM_W4A8, fp8_chain=True,
                    pad_rows=False)


@pytest.mark.parametrize("w4_only", [False, True])
def test_step_plan_with_the_flag(w4_only):
    kw = dict(w4_only=w4_only, preshuffled=not w4_only)
    for T in (129, 3000):
        assert sp.step_plan(T, _facts(w4a8=True, **kw)) == CHAIN
    for T in (1, 17, 32, 33, 100, 128):  # steps of at most 128 rows are untouched
        assert sp.step_plan(T, _facts(w4a8=True, **kw)) == sp.step_plan(T, _facts(**kw)), T
    assert sp.step_plan(17, _facts(w4a8=True, **kw)).qkv == sp.FUSED
    assert sp.step_plan(100, _facts(w4a8=True, **kw)).qkv == sp.FUSED


def test_step_plan_weights_only_never_expands_with_the_flag():
    """Weights-only mode with the fused path off: every step would expand; with the flag every
    step runs the chain instead (no expand, no scratch)."""
    for kw in ({"small_prefill_fused": False}, {"fused_decode": False}):
        for T in (1, 17, 100, 129, 3000):
            assert sp.step_plan(T, _facts(w4a8=True, w4_only=True, preshuffled=False, **kw)) == CHAIN


def test_step_plan_without_the_flag_is_todays():
    """The field defaults to False and a plan with it clear is the plan without the field: a
    sweep of T over both memory modes, both layouts and the other quantisations."""
    assert sp.StepFacts.__dataclass_fields__["w4a8"].default is False
    sweep = list(range(1, 140)) + [187, 188, 189, 447, 448, 640, 641, 1024, 2047, 2048, 3000, 8192]
    for kw in (dict(w4_only=True, preshuffled=False), dict(preshuffled=True),
               dict(preshuffled=False), dict(quant="", preshuffled=True),
               dict(quant="fp8", wdtype=torch.uint8), dict(gpu=False, preshuffled=False)):
        for T in sweep:
            plan = sp.step_plan(T, _facts(**kw))
            assert sp.GEMM_W4A8 not in (plan.qkv, plan.o, plan.gate_up, plan.down)
            assert plan == sp.step_plan(T, _facts(w4a8=False, **kw))
            if kw.get("quant", "mxfp4") != "mxfp4":  # the flag means nothing to other modes
                assert plan == sp.step_plan(T, _facts(w4a8=True, **kw))
    # the plans of the parent commit at the rows the mode takes over
    assert sp.step_plan(300, _facts(w4_only=True, preshuffled=False)) == sp.StepPlan(
        sp.LIB, sp.LIB, sp.LIB, sp.LIB, fp8_chain=False, pad_rows=True)
    assert sp.step_plan(300, _facts()) == sp.step_plan(300, _facts(quant=""))


def test_step_plan_on_the_cpu():
    f = _facts(gpu=False, preshuffled=False, w4a8=True)
    assert sp.step_plan(160, f) == CHAIN
    assert sp.step_plan(100, f) == sp.step_plan(100, _facts(gpu=False, preshuffled=False))


def _cpu_engine(**kw):
    base = dict(model="small", device="cpu", max_model_len=512, num_kv_blocks=64,
                max_num_batched_tokens=512, max_num_seqs=4, use_graphs=False,
                quantization="mxfp4", mxfp4_fp8_activations=True)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_cpu_engine_tokens():
    """The CPU engine runs the mode's reference arithmetic (e4m3 activations of the prompt
    rows, fp32 products with the MXFP4 weight values, bf16 between the kernels): greedy tokens
    of a 160-row and a 300-row prompt, teacher-forced against the dense fp32 oracle with the
    project rule (0.3 logits, one position in five).  The seed (w4a8_oracle.PROMPT_SEED) is
    one for which this run has no divergent position at all - asserted here - so the cap hides
    nothing for the GPU test that shares prompts and oracle."""
    eng = _cpu_engine()
    m = eng.runner.model
    assert m.w4a8 and m.step_plan(160) == CHAIN and m.step_plan(300) == CHAIN
    assert m.w4_scratch is None and m.layers[0].qkv_w4 is None  # CPU: dequantised weights
    tokens, bad = wo.check(eng, wo.prompts())
    assert bad == 0, tokens
    assert all(len(t) == wo.MAX_TOKENS for t in tokens)
