"""The MXFP4 weights-only mode without a GPU: configuration refusals, its row of the step-plan
table and the routing of the explicit wide-kernel choice (ops.fused_kernel)."""
import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.models import step_plan as sp
from agentic_traffic_testing_amd.models.llama import LlamaModel
from agentic_traffic_testing_amd.config import MODEL_PRESETS


def test_config_refuses_the_mode_without_mxfp4():
    for quant in ("", "fp8"):
        with pytest.raises(ValueError, match="mxfp4_weights_only"):
            EngineConfig(quantization=quant, mxfp4_weights_only=True)
    cfg = EngineConfig(quantization="mxfp4", mxfp4_weights_only=True)
    assert cfg.mxfp4_weights_only and not EngineConfig(quantization="mxfp4").mxfp4_weights_only
    with pytest.raises(ValueError):  # TP stays refused, as for mxfp4
        EngineConfig(quantization="mxfp4", mxfp4_weights_only=True, tensor_parallel_size=2)


def test_config_from_env(monkeypatch):
    monkeypatch.setenv("LLM_QUANTIZATION", "mxfp4")
    monkeypatch.setenv("LLM_MXFP4_WEIGHTS_ONLY", "1")
    assert EngineConfig.from_env().mxfp4_weights_only
    monkeypatch.setenv("LLM_MXFP4_WEIGHTS_ONLY", "0")
    assert not EngineConfig.from_env().mxfp4_weights_only
    monkeypatch.setenv("LLM_QUANTIZATION", "fp8")
    monkeypatch.setenv("LLM_MXFP4_WEIGHTS_ONLY", "1")
    with pytest.raises(ValueError, match="mxfp4_weights_only"):
        EngineConfig.from_env()


def test_cpu_engine_and_model_refuse_the_mode():
    cfg = EngineConfig(model="tiny", device="cpu", max_model_len=256, num_kv_blocks=64,
                       max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False,
                       quantization="mxfp4", mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="mxfp4_weights_only"):
        LLMEngine(cfg)
    with pytest.raises(ValueError, match="mxfp4_weights_only"):
        LlamaModel(MODEL_PRESETS["tiny"], device="cpu", quantization="mxfp4",
                   mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="mxfp4_weights_only"):
        LlamaModel(MODEL_PRESETS["tiny"], device="cpu", quantization="",
                   mxfp4_weights_only=True)


def _facts(**kw):
    base = dict(gpu=True, quant="mxfp4", wdtype=torch.bfloat16, tp_size=1, preshuffled=False,
                hidden=4096, q_width=4096, kv_width=1024, inter=14336, gemm_tuned=True,
                w4_only=True)
    base.update(kw)
    return sp.StepFacts(**base)


@pytest.mark.parametrize("T", [1, 32, 33, 128])
def test_step_plan_fused_rows(T):
    """1-32 rows: the 4-bit GEMV; 33-128: the wide kernel's 4-bit builds; never padded."""
    plan = sp.step_plan(T, _facts())
    assert plan == sp.StepPlan(sp.FUSED, sp.FUSED, sp.FUSED, sp.FUSED, fp8_chain=False,
                               pad_rows=False)
    assert sp.proj_fusable(T, True, 1, False, "mxfp4", w4_only=True)
    assert ops.fused_kernel(T, True, mxfp4=True, wide_w4=True) == ("skinny" if T <= 32 else "wide")


@pytest.mark.parametrize("T", [129, 4096])
def test_step_plan_expand_rows(T):
    """The rest: expand + the plan of the unquantised model without pre-shuffled copies."""
    plan = sp.step_plan(T, _facts())
    assert plan == sp.step_plan(T, _facts(quant="", w4_only=False))
    assert plan == sp.StepPlan(sp.LIB, sp.LIB, sp.LIB, sp.LIB, fp8_chain=False, pad_rows=True)
    assert not sp.proj_fusable(T, True, 1, False, "mxfp4", w4_only=True)
    # no tuned library table: the hand-written GEMM where the 16-bit plan routes it
    untuned = sp.step_plan(T, _facts(gemm_tuned=False))
    assert untuned == sp.step_plan(T, _facts(quant="", w4_only=False, gemm_tuned=False))
    assert sp.FUSED not in (untuned.qkv, untuned.o, untuned.gate_up, untuned.down)


def test_step_plan_never_runs_a_16bit_kernel_on_the_scratch():
    """With the fused path off (either switch) every step expands and runs the library: a
    row-major GEMV on the scratch is never planned, whatever the rows."""
    for kw in ({"small_prefill_fused": False}, {"fused_decode": False}, {"hidden": 4096 + 64}):
        for T in (1, 17, 32, 33, 128, 129):
            plan = sp.step_plan(T, _facts(**kw))
            assert sp.FUSED not in (plan.qkv, plan.o, plan.gate_up, plan.down), (kw, T)
            assert plan.pad_rows and not plan.fp8_chain


def test_default_mxfp4_rows_are_unchanged():
    """Without the switch, 33 rows are planned as the 16-bit model's."""
    for ps in (False, True):
        f = _facts(w4_only=False, preshuffled=ps)
        assert sp.step_plan(33, f) == sp.step_plan(33, _facts(w4_only=False, preshuffled=ps,
                                                              quant=""))
        assert sp.step_plan(32, f).qkv == sp.FUSED


def test_fused_kernel_with_and_without_the_explicit_choice():
    for epi in ("plain", "resadd", "qkv", "silu"):
        for m in (1, 16, 32):
            assert ops.fused_kernel(m, True, epi=epi, mxfp4=True) == "skinny"
            assert ops.fused_kernel(m, True, epi=epi, mxfp4=True, wide_w4=True) == "skinny"
        for m in (33, 48, 100, 128):
            assert ops.fused_kernel(m, True, epi=epi, mxfp4=True) is None
            assert ops.fused_kernel(m, True, epi=epi, mxfp4=True, wide_w4=True) == "wide"
        for m in (0, 129, 640):
            assert ops.fused_kernel(m, True, epi=epi, mxfp4=True, wide_w4=True) is None
    for epi in ("sample", "sample_lp", "push"):  # the LM head stays 16-bit
        for m in (1, 33):
            assert ops.fused_kernel(m, True, epi=epi, mxfp4=True, wide_w4=True) is None
    # the keyword changes nothing for the other layouts
    for m in (1, 17, 33, 128, 129):
        assert ops.fused_kernel(m, True, wide_w4=True) == ops.fused_kernel(m, True)
        assert ops.fused_kernel(m, True, True, wide_w4=True) == ops.fused_kernel(m, True, True)
    assert ops.fused_max_rows(mxfp4=True) == 32
    assert ops.fused_max_rows(mxfp4=True, wide_w4=True) == 128
    assert ops.fused_max_rows() == ops.fused_max_rows(wide_w4=True)


def test_closed_form_bound_of_the_wide_w4_shapes():
    """The exactness argument of tests/test_mxfp4_wide_gpu.py, checked for every K it uses:
    |x| <= 4, |w| <= 6 * 2^(129 - 127) = 24, every product a multiple of 2^-3 (0.5 * 2^-2), so
    a partial sum is at most K * 4 * 6 * 4 multiples... below 2^21 of them * 2^3 = 2^24."""
    from test_mxfp4_wide_gpu import KS, NS, ROWS, closed_form_case

    for K in KS:
        assert K * 4 * 6 * 4 < 2 ** 21
        for N in NS:
            _, _, _, want = closed_form_case(N, K, torch.float16, "cpu")
            assert want.shape == (max(ROWS), N)
            assert float(want.abs().max()) < 60000
            assert bool(((want * 8) == (want * 8).round()).all())
