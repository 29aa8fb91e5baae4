"""MXFP4 weight-only quantisation, CPU tier: the quantiser against a brute-force search, the
pre-shuffle round trip, configuration and routing, and the CPU engine against the dense oracle
on the model's own (quantised) weights."""
import math

import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.models import step_plan as sp
from agentic_traffic_testing_amd.models.step_plan import StepFacts

from test_engine import _check, _prompts

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def brute_force(w: torch.Tensor):
    """The format's rule, element by element in Python floats (exact: every operand is a
    16-bit or fp32 value and every scale a power of two)."""
    N, K = w.shape
    codes = torch.zeros(N, K, dtype=torch.uint8)
    scales = torch.zeros(N, K // 32, dtype=torch.uint8)
    wl = w.double().tolist()
    for n in range(N):
        for b in range(K // 32):
            blk = wl[n][32 * b:32 * b + 32]
            amax = max(abs(v) for v in blk)
            e = 0 if amax == 0 else math.floor(math.log2(amax)) - 2
            e = min(max(e + 127, 1), 254) - 127
            scales[n, b] = e + 127
            for i, v in enumerate(blk):
                a = min(abs(v) / 2.0 ** e, 6.0)
                best = min(abs(a - g) for g in GRID)
                cands = [c for c, g in enumerate(GRID) if abs(a - g) == best]
                c = next((c for c in cands if c % 2 == 0), cands[0])  # ties: the even code
                codes[n, 32 * b + i] = c + (8 if v < 0 and c > 0 else 0)
    return codes, scales


def crafted_blocks() -> torch.Tensor:
    """One 32-element block per row: every rounding midpoint under both signs, saturation,
    zero blocks, values that round to zero, and the scale clamps."""
    rows = []
    mids = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    for e in (-9, 0, 3):  # amax = 4 * 2^e -> the block's scale exponent is e
        s = 2.0 ** e
        row = [4.0 * s] + [m * s for m in mids] + [-m * s for m in mids]
        row += [g * s for g in GRID] + [-g * s for g in GRID[1:]] + [0.1 * s, -0.1 * s]
        rows.append(row)
    for amax in (6.5, 7.0, 7.75):  # in (6, 8): e = 0, the maximum saturates to 6
        rows.append([amax, -amax, 6.0, 5.5, -5.0, 0.2, -0.2] + [0.0] * 25)
    rows.append([0.0] * 32)  # zero block: b = 127
    rows.append([2.0 ** -130, -(2.0 ** -131)] + [0.0] * 30)  # b clamps to 1
    rows.append([2.0 ** 127, -(2.0 ** 120)] + [0.0] * 30)    # the largest exponents
    return torch.tensor([r[:32] + [0.0] * (32 - len(r[:32])) for r in rows], dtype=torch.float32)


def test_quantiser_matches_brute_force():
    torch.manual_seed(0)
    rand = (torch.randn(6, 128) * 0.02).bfloat16()
    rand[2, 32:64] = 0  # a zero block inside a row
    for w in (crafted_blocks(), rand, (torch.randn(3, 64) * 3).half()):
        codes, scales = ops.quantize_mxfp4(w)
        want_c, want_s = brute_force(w)
        assert codes.dtype == scales.dtype == torch.uint8
        assert codes.shape == w.shape and scales.shape == (w.shape[0], w.shape[1] // 32)
        assert torch.equal(scales, want_s)
        assert torch.equal(codes, want_c)
        assert int((codes == 8).sum()) == 0, "-0 code"
        assert int(scales.min()) >= 1 and int(scales.max()) <= 254


def test_quantiser_edge_rules():
    w = crafted_blocks()
    codes, scales = ops.quantize_mxfp4(w)
    # ties to the even code: midpoints .25 .75 1.25 1.75 2.5 3.5 5 -> codes 0 2 2 4 4 6 6
    for r, b in ((0, 118), (1, 127), (2, 130)):
        assert int(scales[r, 0]) == b
        assert codes[r, 1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]
        assert codes[r, 8:15].tolist() == [0, 10, 10, 12, 12, 14, 14]  # -0.25 -> code 0, not 8
        assert codes[r, 30:32].tolist() == [0, 0]                      # +-0.1: rounds to zero
    for r in (3, 4, 5):  # amax in (6, 8) * 2^0 saturates
        assert int(scales[r, 0]) == 127 and codes[r, :2].tolist() == [7, 15]
    assert int(scales[6, 0]) == 127 and int(codes[6].sum()) == 0
    assert int(scales[7, 0]) == 1
    assert int(scales[8, 0]) == 252 and int(codes[8, 0]) == 6


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dequantised_values_are_exact_and_stable(dtype):
    torch.manual_seed(1)
    w = (torch.randn(64, 256) * 0.02).to(dtype)
    codes, scales = ops.quantize_mxfp4(w)
    d32 = ops.dequantize_mxfp4(codes, scales, torch.float32)
    d = ops.dequantize_mxfp4(codes, scales, dtype)
    assert torch.equal(d32, d32.bfloat16().float()), "a dequantised weight is not exact in bf16"
    assert torch.equal(d.float(), d32)
    c2, s2 = ops.quantize_mxfp4(d)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    rel = float((d32 - w.float()).norm() / w.float().norm())
    assert 0.05 < rel < 0.2, rel  # ~11 % on Gaussian weights


@pytest.mark.parametrize("rowmap", ["plain", "qkv", "silu"])
@pytest.mark.parametrize("shape", [(64, 128), (128, 384), (256, 2816)])
def test_preshuffle_round_trip(shape, rowmap):
    g = torch.Generator().manual_seed(shape[1])
    codes = torch.randint(0, 16, shape, dtype=torch.uint8, generator=g)
    scales = torch.randint(1, 255, (shape[0], shape[1] // 32), dtype=torch.uint8, generator=g)
    if rowmap == "qkv" and shape[0] % 128:
        # the qkv row map pairs RoPE dims d, d + 64 of whole 128-dim heads: 64 rows have none,
        # and the 4-bit layout refuses them as the 16-bit and fp8 ones do
        with pytest.raises(ValueError, match="whole 128-dim heads"):
            ops.preshuffle_mxfp4(codes, scales, rowmap)
        return
    wq, sq = ops.preshuffle_mxfp4(codes, scales, rowmap)
    assert wq.dtype == sq.dtype == torch.uint8
    assert wq.shape == (shape[0], shape[1] // 2) and sq.shape == scales.shape
    c, s = ops.unshuffle_mxfp4(wq, sq, rowmap)
    assert torch.equal(c, codes) and torch.equal(s, scales)
    if rowmap != "plain":  # the row map is part of the layout
        c_plain, _ = ops.unshuffle_mxfp4(wq, sq, "plain")
        assert not torch.equal(c_plain, codes)
    with pytest.raises(ValueError):
        ops.preshuffle_mxfp4(codes[:, :96], scales[:, :3], rowmap)


def test_config_and_serve_flag(monkeypatch):
    from agentic_traffic_testing_amd.serving import serve_llm

    assert EngineConfig(model="tiny", device="cpu", quantization="mxfp4").quantization == "mxfp4"
    with pytest.raises(ValueError):
        EngineConfig(model="tiny", device="cpu", quantization="mxfp4", tensor_parallel_size=2)
    with pytest.raises(ValueError):
        EngineConfig(model="tiny", device="cpu", quantization="mxfp4").replace(
            tensor_parallel_size=2)
    args = serve_llm.make_parser().parse_args(["--model", "tiny", "--device", "cpu", "-q", "mxfp4"])
    assert serve_llm.build_config(args).quantization == "mxfp4"
    args = serve_llm.make_parser().parse_args(
        ["--model", "tiny", "--device", "cpu", "--quantization", "mxfp4"])
    assert serve_llm.build_config(args).quantization == "mxfp4"
    monkeypatch.setenv("LLM_QUANTIZATION", "MXFP4")
    assert EngineConfig.from_env().quantization == "mxfp4"
    args = serve_llm.make_parser().parse_args(["--model", "tiny", "--device", "cpu"])
    assert serve_llm.build_config(args).quantization == "mxfp4"


def test_routing_names_the_4bit_kernel():
    for epi in ("plain", "resadd", "qkv", "silu"):
        assert ops.fused_kernel(1, True, epi=epi, mxfp4=True) == "skinny"
        assert ops.fused_kernel(32, True, epi=epi, mxfp4=True) == "skinny"
        assert ops.fused_kernel(33, True, epi=epi, mxfp4=True) is None
        assert ops.fused_kernel(0, True, epi=epi, mxfp4=True) is None
    for m in (1, 16, 32, 33):
        assert ops.fused_kernel(m, True, epi="sample", mxfp4=True) is None
        assert ops.fused_kernel(m, True, epi="push", mxfp4=True) is None
    assert ops.fused_max_rows(mxfp4=True) == 32
    for proj in ("qkv", "o", "gate_up", "down"):
        assert ops.decode_waves(proj, mxfp4=True) in (4, 8, 16)
    x = torch.zeros(4, 256)
    assert not ops.skinny_ok(x, torch.zeros(64, 128, dtype=torch.uint8), mxfp4=True)  # no GPU


def _facts(quant, preshuffled, hidden=4096, inter=14336):
    return StepFacts(gpu=True, quant=quant, wdtype=torch.bfloat16, tp_size=1,
                     preshuffled=preshuffled, hidden=hidden, q_width=hidden,
                     kv_width=hidden // 4, inter=inter, gemm_tuned=True)


@pytest.mark.parametrize("preshuffled", [True, False])
def test_step_plan_rows(preshuffled):
    q4 = _facts("mxfp4", preshuffled)
    for T in (1, 5, 16, 17, 32):
        plan = sp.step_plan(T, q4)
        assert (plan.qkv, plan.o, plan.gate_up, plan.down) == ("fused",) * 4
        assert not plan.fp8_chain and not plan.pad_rows
    for T in (33, 64, 128, 129, 188, 189, 447, 448, 640, 641, 1024, 2048, 4096):
        assert sp.step_plan(T, q4) == sp.step_plan(T, _facts("", preshuffled)), T
    # `small` (inter 2816 = 22 loads) and `tiny` (hidden 256 = 2 loads) fuse; K % 128 != 0 not
    assert sp.proj_dims_ok(True, "mxfp4", 1024, 1024, 2816)
    assert sp.proj_dims_ok(True, "mxfp4", 256, 512, 512)
    assert not sp.proj_dims_ok(True, "mxfp4", 1024, 1024, 2816 + 64)
    assert sp.step_plan(8, _facts("mxfp4", preshuffled, inter=2816 + 64)) == \
        sp.step_plan(8, _facts("", preshuffled, inter=2816 + 64))
    # on the CPU everything is the library
    cpu = StepFacts(gpu=False, quant="mxfp4", wdtype=torch.bfloat16, tp_size=1, preshuffled=False,
                    hidden=256, q_width=512, kv_width=256, inter=512)
    assert sp.step_plan(4, cpu).qkv == "lib"


def test_engine_cpu_matches_dense_on_quantised_weights():
    cfg = EngineConfig(model="tiny", device="cpu", max_model_len=256, num_kv_blocks=64,
                       max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False,
                       quantization="mxfp4")
    eng = LLMEngine(cfg)
    m = eng.runner.model
    assert m.quant == "mxfp4"
    for L in m.layers:  # the stored projections hold MXFP4 values, in the model's dtype
        for w in (L.qkv, L.o, L.gate_up, L.down):
            assert w.dtype == m.dtype
            assert torch.equal(ops.dequantize_mxfp4(*ops.quantize_mxfp4(w), w.dtype), w)
        assert L.qkv_w4 is None  # the 4-bit copies are the GPU kernels' business
    plain = LLMEngine(cfg.replace(quantization="")).runner.model
    assert not torch.equal(plain.layers[0].qkv, m.layers[0].qkv)
    assert torch.equal(plain.embed, m.embed) and torch.equal(plain.lm_head, m.lm_head)
    outs, _ = _check(eng, _prompts())
    assert outs[-1].cached_prompt_tokens == 48
