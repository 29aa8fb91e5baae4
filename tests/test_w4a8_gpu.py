"""MXFP4 W4A8 prefill GEMM (ops.gemm_w4a8, csrc/prefill_gemm_w4a8.hip) on the GPU: exact
integer cases by bit equality (row counts around every tile edge, every
depth of the K loop, the three row maps, both epilogues), layout probes that read single weights
back through the MFMA, Gaussian operands against fp32, and the engine with
mxfp4_fp8_activations in both memory modes against the oracle of tests/w4a8_oracle.py.

Exactness: activations are integers in [-4, 4] (exact e4m3 codes), weights are e2m1 values
times 2^(b - 127) with b in 125..129, so every product is a multiple of 2^-3 and every partial
sum stays below K * 4 * 24 <= 2^24 * 2^-3 at K <= 4096: fp32 accumulation is exact in any
order, the row scale is a power of two, and the output is ONE rounding of the fp64 product.
SiLU's exp is inexact: its cases keep |gate| <= helpers.SILU_EXACT_GATE (row scales 2^-8,
2^-9) and use the project's boundary rule - bit equality, except that an element whose fp64
value lies within helpers.ROW_DELTA of a rounding tie may be one step off."""
import functools
import gc

import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.ops import reference as ref

import w4a8_oracle as wo
from helpers import ROW_DELTA, SILU_EXACT_GATE, assert_rows, round_fmt
from test_mxfp4_gpu import close

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
H = ops.W4A8_TILE                           # the one tile height: 64
# 1, 31, 33, 129; h - 1, h, h + 1 and 2 h + 1 (2 h + 1 = 129)
MS = sorted({1, 31, 33, 129, H - 1, H, H + 1, 2 * H + 1})
# the K loop loads one chunk ahead (depth 2): 1..5 chunks cover the prologue at every depth
KS = (128, 256, 384, 512, 640)
# one column tile (4 waves x 32 rows) / two column tiles + one 32-row fragment; the qkv row map
# takes whole 128-row heads only, so its second width is three column tiles
NS = {"plain": (128, 288), "silu": (128, 288), "qkv": (128, 384)}
GUARD = 8                                   # sentinel rows behind row M of every output
SENTINEL = 0x5A5B


@functools.lru_cache(maxsize=None)
def exact_case(N, K, silu_scale=False):
    """(codes, scales, x integers, xs, fp64 W) on the CPU: every e2m1 code, a fresh draw of the
    scale byte from 125..129 for every block, x in [-4, 4], power-of-two row scales."""
    g = torch.Generator().manual_seed(1000 * N + K)
    codes = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
    assert len(torch.unique(codes)) == 16
    scales = torch.randint(125, 130, (N, K // 32), dtype=torch.uint8, generator=g)
    x = torch.randint(-4, 5, (max(MS), K), generator=g).float()
    e = torch.arange(max(MS)) % (2 if silu_scale else 4)
    xs = torch.pow(2.0, (-9.0 + e) if silu_scale else (-2.0 + e)).float()
    W = ops.dequantize_mxfp4(codes, scales, torch.float32).double()
    assert K * 4 * 24 * 8 <= 2 ** 24
    return codes, scales, x, xs, W


def _launch(xq, xs, wq, sq, rowmap, mode, m, width):
    """The op into rows [0, m) of a sentinel-filled buffer; the rows behind must stay."""
    big = torch.full((m + GUARD, width), SENTINEL, dtype=torch.int16, device="cuda").view(BF16)
    got = ops.gemm_w4a8(xq[:m], xs[:m], wq, sq, rowmap, mode, out=big[:m])
    assert got.data_ptr() == big.data_ptr()
    assert bool((big[m:].view(torch.int16) == SENTINEL).all()), f"rows past M written (m={m})"
    return got


@pytest.mark.parametrize("rowmap", ["plain", "qkv", "silu"])
def test_plain_exact(rowmap):
    launches = 0
    for N, K in [(N, K) for N in NS[rowmap] for K in KS] + [(512, 4096)]:
        codes, scales, x, xs, W = exact_case(N, K)
        want = ((x.double() @ W.t()) * xs.double()[:, None]).to(BF16).cuda()
        wq, sq = (t.cuda() for t in ops.preshuffle_mxfp4(codes, scales, rowmap))
        xq = x.to(torch.float8_e4m3fn).view(torch.uint8).cuda()
        xsd = xs.cuda()
        for m in MS:
            got = _launch(xq, xsd, wq, sq, rowmap, ops.GEMM_PLAIN, m, N)
            launches += 1
            if not torch.equal(got.view(torch.int16), want[:m].view(torch.int16)):
                assert_rows(got, want[:m], None, 0, f"{rowmap} N={N} K={K} m={m}")
    torch.cuda.synchronize()
    print(f"W4A8-EXACT plain {rowmap} launches={launches}")


@pytest.mark.parametrize("inter", [128, 384])
def test_silu_exact(inter):
    N = 2 * inter
    worst_share = 0.0
    for K in KS:
        codes, scales, x, xs, W = exact_case(N, K, silu_scale=True)
        y = (x.double() @ W.t()) * xs.double()[:, None]
        g, u = y[:, :inter], y[:, inter:]
        assert float(g.abs().max()) <= SILU_EXACT_GATE
        want, near = round_fmt(g / (1.0 + torch.exp(-g)) * u, BF16, delta=ROW_DELTA)
        want = want.to(BF16)
        wq, sq = (t.cuda() for t in ops.preshuffle_mxfp4(codes, scales, "silu"))
        xq = x.to(torch.float8_e4m3fn).view(torch.uint8).cuda()
        xsd = xs.cuda()
        for m in MS:
            got = _launch(xq, xsd, wq, sq, "silu", ops.GEMM_SILU, m, inter).cpu()
            if not torch.equal(got.view(torch.int16), want[:m].view(torch.int16)):
                worst_share = max(worst_share, assert_rows(
                    got, want[:m], near[:m], 1, f"silu I={inter} K={K} m={m}"))
    assert worst_share <= 0.02  # helpers.ROW_SHARE_CAP: the boundary rule stays the exception


@pytest.mark.parametrize("rowmap,N", [("plain", 288), ("qkv", 256), ("silu", 288)])
def test_layout_probe(rowmap, N):
    """Row m of xq is a single 1.0 at k = 128 c + m, so y[m, n] must be weight [n, 128 c + m]
    itself: codes distinct along both axes (an asymmetric matrix) and a scale byte that
    depends on (n, k / 32) - a wrong lane-to-k map, a neighbour's block scale, a transposed or
    permuted store each move values that differ."""
    K = 384
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = ((3 * n + 5 * k + (n * k) // 7) % 16).to(torch.uint8)
    scales = (125 + (n + 2 * torch.arange(K // 32)[None, :]) % 5).to(torch.uint8)
    W = ops.dequantize_mxfp4(codes, scales, torch.float32)
    assert not torch.equal(W[:128, :128], W[:128, :128].t())
    wq, sq = (t.cuda() for t in ops.preshuffle_mxfp4(codes, scales, rowmap))
    xs = torch.ones(128, device="cuda")
    for c in range(K // 128):
        x = torch.zeros(128, K)
        x[torch.arange(128), 128 * c + torch.arange(128)] = 1.0
        xq = x.to(torch.float8_e4m3fn).view(torch.uint8).cuda()
        want = (x.double() @ W.double().t()).to(BF16)  # the product: code 8 (-0) sums to +0
        assert torch.equal(want.float(), W[:, 128 * c:128 * (c + 1)].t())
        got = ops.gemm_w4a8(xq, xs, wq, sq, rowmap).cpu()
        assert_rows(got, want, None, 0, f"probe {rowmap} chunk {c}")


def test_binding_refuses_what_it_cannot_run():
    codes = torch.zeros(64, 256, dtype=torch.uint8, device="cuda")
    scales = torch.full((64, 8), 127, dtype=torch.uint8, device="cuda")
    wq, sq = ops.preshuffle_mxfp4(codes, scales)
    xq = torch.zeros(4, 256, dtype=torch.uint8, device="cuda")
    xs = torch.ones(4, device="cuda")
    assert ops.gemm_w4a8(xq, xs, wq, sq, "plain").shape == (4, 64)
    with pytest.raises(ValueError):  # rows of xq not 16-byte aligned
        ops.gemm_w4a8(torch.zeros(4, 264, dtype=torch.uint8, device="cuda")[:, 8:], xs, wq, sq,
                      "plain")
    with pytest.raises(ValueError):  # N % 32
        ops.gemm_w4a8(xq, xs, wq[:48], sq[:48], "plain")
    with pytest.raises(ValueError):  # out of another dtype
        ops.gemm_w4a8(xq, xs, wq, sq, "plain",
                      out=torch.empty(4, 64, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):  # fp16 scales
        ops.gemm_w4a8(xq, xs.half(), wq, sq, "plain")


def test_random_operands_vs_fp32():
    """Gaussian operands through ops.quant_rows_fp8 / ops.quantize_mxfp4 at M = 160 with the 8B
    K: a gate_up slice (N = 2 x 512, both epilogues) and a qkv slice (N = 768).  Both sides use
    the same quantised values; the bounds are test_mxfp4_gpu.close with that file's constants
    (2e-2 + 1 % for a plain product, 3e-2 + 3 % behind SiLU-mul)."""
    torch.manual_seed(43)
    M, K = 160, 4096
    x = torch.randn(M, K, dtype=BF16, device="cuda")
    xq, xs = ops.quant_rows_fp8(x)
    xf = xq.view(torch.float8_e4m3fn).float() * xs

    def q(w, rowmap):
        codes, scales = ops.quantize_mxfp4(w)
        return (*ops.preshuffle_mxfp4(codes, scales, rowmap),
                ops.dequantize_mxfp4(codes, scales, torch.float32))

    wq, sq, wf = q(torch.randn(768, K, dtype=BF16, device="cuda") * 0.05, "qkv")
    close(ops.gemm_w4a8(xq, xs, wq, sq, "qkv"), xf @ wf.t(), 2e-2, 1e-2)
    wq, sq, wf = q(torch.randn(1024, K, dtype=BF16, device="cuda") * 0.05, "silu")
    exp = xf @ wf.t()
    close(ops.gemm_w4a8(xq, xs, wq, sq, "silu"), exp, 2e-2, 1e-2)
    close(ops.gemm_w4a8(xq, xs, wq, sq, "silu", ops.GEMM_SILU), ref.silu_and_mul(exp), 3e-2, 3e-2)


def _engine(**kw):
    gc.collect()  # engines of earlier tests go now, not while this one captures a hipGraph
    base = dict(model="small", device="cuda", max_model_len=512, num_kv_blocks=512,
                max_num_seqs=8, graph_batch_sizes=(1, 2, 4, 8), max_num_batched_tokens=512,
                quantization="mxfp4")
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def test_engine_tokens_against_the_oracle():
    """mxfp4 + the flag, default memory mode: the 160-row and the 300-row prompt of the CPU
    test (which has no divergent position on them) run the chain on ops.gemm_w4a8; the 0.3
    near-tie rule and the one-in-five cap of w4a8_oracle.check."""
    eng = _engine(mxfp4_fp8_activations=True)
    m = eng.runner.model
    plan = m.step_plan(160)
    assert plan.fp8_chain and not plan.pad_rows
    assert (plan.qkv, plan.o, plan.gate_up, plan.down) == ("gemm_w4a8",) * 4
    calls = []
    real = ops.gemm_w4a8

    def spy(xq, *a, **kw):
        calls.append(xq.shape[0])
        return real(xq, *a, **kw)

    ops.gemm_w4a8 = spy
    try:
        wo.check(eng, wo.prompts())
    finally:
        ops.gemm_w4a8 = real
    assert calls.count(160) == calls.count(300) == 4 * len(m.layers), calls
    assert all(rows > 128 for rows in calls), calls


def test_engine_weights_only_runs_without_expand_or_scratch(monkeypatch):
    """Both switches: no scratch is allocated, ops.expand_mxfp4 is never reached, and the
    tokens pass the same check."""
    def no_expand(*a, **kw):
        raise AssertionError("expand_mxfp4 reached with mxfp4_fp8_activations")

    monkeypatch.setattr(ops, "expand_mxfp4", no_expand)
    eng = _engine(mxfp4_fp8_activations=True, mxfp4_weights_only=True)
    m = eng.runner.model
    assert m.w4_only and m.w4a8 and m.w4_scratch is None
    assert eng.runner.resident_weights["scratch"] == 0
    assert all(getattr(L, p) is None for L in m.layers for p in wo.PROJS)
    wo.check(eng, wo.prompts())


def test_rows_up_to_128_are_untouched():
    """A 100-row prompt: the flag-on engine gives the flag-off engine's tokens exactly."""
    import numpy as np

    prompt = np.random.default_rng(100).integers(300, 30000, size=100).tolist()
    sp_ = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    toks = []
    for flag in (False, True):
        eng = _engine(mxfp4_fp8_activations=flag, graph_batch_sizes=(1,))
        plan = eng.runner.model.step_plan(100)
        assert (plan.qkv, plan.o, plan.gate_up, plan.down) == ("fused",) * 4 and not plan.fp8_chain
        toks.append(eng.generate([prompt], sp_)[0].token_ids)
        del eng
    assert toks[0] == toks[1]

