"""Stage loop of the skinny decode GEMV (ops/csrc/skinny.h): the two-stage register pipeline
and its peeled tail, by stages per wave.

Shapes are chosen by what the loop does, not by model size.  A launch with `waves` waves and
`unroll` 32-wide K steps per stage gives each wave K / waves of K, consumed in stages of
STEP = 32 * unroll plus a 32-wide tail loop.  K = waves * STEP * n + waves * 32 * r, n in
0..4, r in {0, 1}, walks a wave through 0, 1, 2, 3 and 4 full stages (no stage at all; the
single peeled stage; the peeled pair; one steady-state iteration + one peeled stage; one
iteration + the peeled pair), each with and without a tail step.  N = 64 (four workgroups).
Every (waves, unroll) the launcher can select for 16-bit weights is covered, in the row-major
and the pre-shuffled layout, at M = 1, 5 and 16 rows (one MFMA row tile: the pipelined order;
two row tiles keep the drained order, which tests/test_kernels_gpu.py covers).

Every call is compared with an fp32 reference computed once on the CPU (ops/reference.py for
the fused epilogues) at the tolerance tests/test_kernels_gpu.py uses for the same op, and is
issued twice: both results must be bit-identical.  The plain GEMM has to meet that file's
bound (2e-2 * sqrt(K / 4096) absolute + 1e-2 relative) and the same two figures with
absolute and relative exchanged; the outputs are bf16 roundings (2^-9 relative) of an fp32
sum, far inside either.

test_references_are_finite_and_discriminating runs without a GPU: the references are finite,
and one dropped 32-wide K step (the smallest slip a stage loop can make) moves more than
half of a plain call's outputs past the tolerance at every K used, so a passing comparison
means every stage was consumed exactly once.
"""
import functools
import math

import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.ops import reference as ref

DT = torch.bfloat16
EPS = 1e-5
ROWS = (1, 5, 16)
N = 64
# (layout, waves) -> unroll, as launch_epi picks it (ops/csrc/gemv.hip)
CONFIGS = {("rm", 16): 2, ("rm", 8): 2, ("rm", 4): 4, ("ps", 16): 2, ("ps", 8): 4, ("ps", 4): 4}


def stage_ks(waves, unroll):
    """K giving a wave 0..4 full stages, each with and without a 32-wide tail step."""
    ks = [waves * 32 * (unroll * n + r) for n in range(5) for r in (0, 1)]
    return [k for k in ks if k > 0]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).to(DT)


def _norm(x):
    return ref.rms_norm(x, torch.ones(x.shape[1], dtype=x.dtype), EPS)


@functools.lru_cache(maxsize=None)
def plain_case(k):
    """x [16, K], W [N, K], residual [16, N], fp32 x W^T; rows are used as x[:m]."""
    x = _randn((16, k), 100 + k)
    w = _randn((N, k), 200 + k, 0.02)
    r = _randn((16, N), 300 + k)
    return x, w, r, x.float() @ w.float().t()


HQ, HKV, BS, NB = 1, 1, 16, 4


@functools.lru_cache(maxsize=None)
def qkv_case(k, m):
    x = _randn((m, k), 400 + k, 2.0)
    w = _randn(((HQ + 2 * HKV) * 128, k), 500 + k, 0.02)
    pos = torch.randint(0, 64, (m,), generator=_gen(600 + k), dtype=torch.int32)
    slots = torch.randperm(NB * BS, generator=_gen(700 + k))[:m].to(torch.int32)
    if m > 1:
        slots[1] = -1  # padded row: nothing may be written for it
    cs = ref.rope_cos_sin(128, 64, 500000.0, None)
    kc = _randn((NB, HKV, BS, 128), 800 + k)
    vc = _randn((NB, HKV, 128, BS), 900 + k)
    kc_exp, vc_exp = kc.clone(), vc.clone()
    qkv = (_norm(x).float() @ w.float().t()).to(DT)
    q_exp = ref.rope_cache(qkv, pos, slots, cs, kc_exp, vc_exp, HQ, HKV, 128)
    return x, w, pos, slots, cs, kc, vc, q_exp, kc_exp, vc_exp


INTER = N // 2


@functools.lru_cache(maxsize=None)
def silu_case(k):
    x = _randn((16, k), 1000 + k, 2.0)
    w = _randn((2 * INTER, k), 1100 + k, 0.02)
    exp = ref.silu_and_mul((_norm(x).float() @ w.float().t()).to(DT))
    return x, w, exp


VOCAB = 64


@functools.lru_cache(maxsize=None)
def lm_case(k):
    x = _randn((16, k), 1200 + k, 2.0)
    w = _randn((VOCAB, k), 1300 + k, 0.05)
    return x, w, _norm(x).float() @ w.float().t()


def plain_tols(k):
    a, b = 2e-2 * math.sqrt(k / 4096), 1e-2
    return (a, b), (b, a)  # (atol, rtol): test_kernels_gpu.py's reading and the exchanged one


def close(a, b, atol, rtol=0.0):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    assert bool((err <= tol).all()), f"max err {err.max().item():.4g}"


def all_ks():
    return sorted({k for (_, wv), u in CONFIGS.items() for k in stage_ks(wv, u)})


def test_stage_shapes():
    assert stage_ks(4, 4) == [128, 512, 640, 1024, 1152, 1536, 1664, 2048, 2176]
    for (_, waves), unroll in CONFIGS.items():
        for k in stage_ks(waves, unroll):
            kw = k // waves
            assert k % 128 == 0 and k % (32 * waves) == 0
            assert kw // (32 * unroll) in range(5) and (kw % (32 * unroll)) in (0, 32)


def test_references_are_finite_and_discriminating():
    for k in all_ks():
        x, w, r, exp = plain_case(k)
        assert bool(torch.isfinite(exp).all())
        (a1, r1), (a2, r2) = plain_tols(k)
        tol = torch.maximum(a1 + r1 * exp.abs(), a2 + r2 * exp.abs())
        # output change if the last 32-wide K step were dropped (or, negated, read twice)
        slip = (x[:, -32:].float() @ w[:, -32:].float().t()).abs()
        frac = float((slip > tol).float().mean())
        assert frac > 0.5, (k, frac)
        assert float(exp.std()) > 0.1
        _, _, sexp = silu_case(k)
        assert bool(torch.isfinite(sexp.float()).all()) and float(sexp.float().std()) > 0.02
        _, _, logits = lm_case(k)
        assert bool(torch.isfinite(logits).all()) and float(logits.std()) > 0.3
        for m in ROWS:
            c = qkv_case(k, m) if k in qkv_ks() else None
            if c is not None:
                assert bool(torch.isfinite(c[7].float()).all()) and float(c[7].float().std()) > 0.1
                assert not torch.equal(c[5], c[8]) and not torch.equal(c[6], c[9])


def qkv_ks():
    # the qkv launcher takes 8 waves row-major (8 x 2) and 4 waves pre-shuffled (4 x 4)
    return sorted(set(stage_ks(8, 2)) | set(stage_ks(4, 4)))


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), ops._load_error


def _w(w, layout, rowmap="plain"):
    w = w.cuda()
    return ops.preshuffle(w, rowmap) if layout == "ps" else w


@pytest.mark.gpu
@pytest.mark.parametrize("layout,waves", list(CONFIGS))
def test_plain_and_residual(native, layout, waves):
    ps = layout == "ps"
    for k in stage_ks(waves, CONFIGS[(layout, waves)]):
        x, w, r, exp = plain_case(k)
        xg, wg = x.cuda(), _w(w, layout)
        for m in ROWS:
            a = ops.linear(xg[:m], wg, waves=waves, preshuffled=ps)
            b = ops.linear(xg[:m], wg, waves=waves, preshuffled=ps)
            assert torch.equal(a, b), (k, m)
            for atol, rtol in plain_tols(k):
                close(a, exp[:m], atol, rtol)
            exp_r = exp[:m].to(DT).float() + r[:m].float()
            r1, r2 = r[:m].cuda(), r[:m].cuda()
            ops.linear(xg[:m], wg, residual=r1, waves=waves, preshuffled=ps)
            ops.linear(xg[:m], wg, residual=r2, waves=waves, preshuffled=ps)
            assert torch.equal(r1, r2), (k, m)
            close(r1, exp_r, 3e-2 * math.sqrt(k / 4096), 1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rm", "ps"])
def test_qkv_rope_cache(native, layout):
    ps = layout == "ps"
    waves = ops.decode_waves("qkv", ps)
    for k in stage_ks(waves, CONFIGS[(layout, waves)]):
        for m in ROWS:
            x, w, pos, slots, cs, kc, vc, q_exp, kc_exp, vc_exp = qkv_case(k, m)
            wg = _w(w, layout, "qkv")
            outs = []
            for _ in range(2):
                k2, v2 = kc.cuda(), vc.cuda()
                q = ops.decode_qkv_rope(x.cuda(), wg, EPS, pos.cuda(), slots.cuda(), cs.cuda(),
                                        k2, v2, HQ, HKV, preshuffled=ps, ksplit=1)
                outs.append((q, k2, v2))
            for a, b in zip(*outs):
                assert torch.equal(a, b), (k, m)
            close(outs[0][0], q_exp, 3e-2, 2e-2)
            close(outs[0][1], kc_exp, 3e-2, 2e-2)
            close(outs[0][2], vc_exp, 3e-2, 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rm", "ps"])
def test_gate_up_silu_norm_fold(native, layout):
    ps = layout == "ps"
    waves = ops.decode_waves("gate_up", ps, m=1)
    ops.set_wide_min_rows(33, 33)  # 12-16 pre-shuffled rows would run the wide kernel
    try:
        for k in stage_ks(waves, CONFIGS[(layout, waves)]):
            x, w, exp = silu_case(k)
            xg, wg = x.cuda(), _w(w, layout, "silu")
            for m in ROWS:
                a = ops.decode_gate_up_silu(xg[:m], wg, EPS, preshuffled=ps, ksplit=1)
                b = ops.decode_gate_up_silu(xg[:m], wg, EPS, preshuffled=ps, ksplit=1)
                assert torch.equal(a, b), (k, m)
                close(a, exp[:m], 4e-2, 4e-2)
    finally:
        ops.set_wide_min_rows()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rm", "ps"])
def test_lm_head_sample_small_vocab(native, layout):
    ps = layout == "ps"
    waves = ops.decode_waves("lm_head", ps)
    for k in stage_ks(waves, CONFIGS[(layout, waves)]):
        x, w, logits = lm_case(k)
        xg, wg = x.cuda(), _w(w, layout)
        top2 = torch.topk(logits, 2, dim=-1)
        for m in ROWS:
            keys = torch.full((m * VOCAB // 16,), -1, dtype=torch.int64, device="cuda")
            temp = torch.zeros(m, device="cuda")
            seeds = torch.arange(m, dtype=torch.int64, device="cuda")
            steps = torch.zeros(m, dtype=torch.int64, device="cuda")
            a = ops.decode_lm_head_sample(xg[:m], wg, EPS, temp, seeds, steps, keys,
                                          preshuffled=ps).clone()
            b = ops.decode_lm_head_sample(xg[:m], wg, EPS, temp, seeds, steps, keys,
                                          preshuffled=ps).clone()
            assert torch.equal(a, b), (k, m)
            for row in range(m):
                g = int(a[row])
                # exact argmax unless the top-2 are within bf16 rounding of each other
                assert g == int(top2.indices[row, 0]) or \
                    float(top2.values[row, 0] - logits[row, g]) < 0.05, (k, m, row)
            temp.fill_(0.8)
            t1 = ops.decode_lm_head_sample(xg[:m], wg, EPS, temp, seeds, steps, keys,
                                           preshuffled=ps).clone()
            t2 = ops.decode_lm_head_sample(xg[:m], wg, EPS, temp, seeds, steps, keys,
                                           preshuffled=ps).clone()
            assert torch.equal(t1, t2), (k, m)
            assert bool(((t1 >= 0) & (t1 < VOCAB)).all())
