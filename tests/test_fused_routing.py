"""The routing table of the fused weight-streaming GEMMs.

CPU: ``ops.fused_kernel`` against the table written out literally (docs/kernels.md, the
comment above ``route()`` in ops/csrc/gemv.hip).  GPU: the native entry points agree with it -
a call runs and matches ops/reference.py where the table names a kernel, and is refused on the
host (``check_rc``) where it names none."""
import math

import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.ops import reference as ref

ROWS = (0, 1, 11, 12, 16, 17, 32, 33, 128, 129, 1024, 1025)
S, W, M, N = "skinny", "wide", "midm", None
# rows:             0  1 11 12 16 17 32 33 128 129 1024 1025
ROW_MAJOR =        (N, S, S, S, S, S, S, N, N, N, N, N)
PS_FROM_17 =       (N, S, S, S, S, W, W, W, W, M, M, N)
PS_FROM_12 =       (N, S, S, W, W, W, W, W, W, M, M, N)
PS_SAMPLE =        (N, S, S, S, S, W, W, W, W, N, N, N)
FP8 =              (N, S, S, S, S, S, S, W, W, M, M, N)
FP8_SAMPLE =       (N, S, S, S, S, S, S, N, N, N, N, N)
TABLE = {
    "row-major": dict(plain=ROW_MAJOR, resadd=ROW_MAJOR, qkv=ROW_MAJOR, silu=ROW_MAJOR,
                      sample=ROW_MAJOR),
    "pre-shuffled": dict(plain=PS_FROM_17, resadd=PS_FROM_17, qkv=PS_FROM_17, silu=PS_FROM_12,
                         sample=PS_SAMPLE),
    "fp8": dict(plain=FP8, resadd=FP8, qkv=FP8, silu=FP8, sample=FP8_SAMPLE),
}
LAYOUTS = {"row-major": (False, False), "pre-shuffled": (True, False), "fp8": (True, True)}
EPIS = ("plain", "resadd", "qkv", "silu", "sample")


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fused_kernel_table(layout, epi):
    ps, fp8 = LAYOUTS[layout]
    got = tuple(ops.fused_kernel(m, ps, fp8, epi) for m in ROWS)
    assert got == TABLE[layout][epi], dict(zip(ROWS, got))


def test_fused_kernel_push_variant():
    """The TP push epilogue exists in the 16-row-tile GEMV only, whatever the layout."""
    for ps, fp8 in LAYOUTS.values():
        got = tuple(ops.fused_kernel(m, ps, fp8, "push") for m in ROWS)
        assert got == ROW_MAJOR


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_wide_max_zero_turns_wide_and_midm_off(monkeypatch, layout, epi):
    monkeypatch.setattr(ops, "WIDE_MAX_M", 0)
    ps, fp8 = LAYOUTS[layout]
    for m in ROWS:
        if m > 32:
            assert ops.fused_kernel(m, ps, fp8, epi) is None, m
        elif m >= 1:  # and nothing at or below 32 rows takes the kernel that is off
            assert ops.fused_kernel(m, ps, fp8, epi) == "skinny", m
    assert ops.fused_max_rows() == ops.SKINNY_MAX_M


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_midm_max_zero_turns_midm_off(monkeypatch, layout, epi):
    monkeypatch.setattr(ops, "MIDM_MAX_M", 0)
    ps, fp8 = LAYOUTS[layout]
    for m, want in zip(ROWS, TABLE[layout][epi]):
        assert ops.fused_kernel(m, ps, fp8, epi) == (None if m > 128 else want), m
    assert ops.fused_max_rows() == 128


# ---- GPU: the native entry points route as the table says -----------------------------------
GPU_ROWS = (1, 16, 17, 32, 33, 128, 129, 144)
K, NOUT, HQ, HKV = 256, 128, 1, 1  # one 128-dim q head + one kv head: 384 qkv rows


def close(a, b, atol, rtol=0.0):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), f"max err {err.max().item():.4g}"


def _norm_ref(x, eps=1e-5):
    return ref.rms_norm(x, torch.ones(x.shape[1], dtype=x.dtype, device=x.device), eps)


@pytest.fixture(scope="module")
def gpu_case():
    """Weights (both layouts), the widest x and the fp32 references, computed once."""
    assert ops.native_available(), ops._load_error
    ops.ensure_splitk_workspace("cuda")
    torch.manual_seed(61)
    dt, mmax = torch.bfloat16, max(GPU_ROWS)
    c = {"x": torch.randn(mmax, K, dtype=dt, device="cuda")}
    for name, n, rowmap in (("plain", NOUT, "plain"), ("qkv", (HQ + 2 * HKV) * 128, "qkv"),
                            ("silu", 2 * NOUT, "silu"), ("lm", 2048, "plain")):
        w = torch.randn(n, K, dtype=dt, device="cuda") * 0.05
        c[name] = {False: w, True: ops.preshuffle(w, rowmap), "w": w}
    c["res"] = torch.randn(mmax, NOUT, dtype=dt, device="cuda")
    c["exp_plain"] = c["x"].float() @ c["plain"]["w"].float().t()
    c["exp_silu"] = ref.silu_and_mul(torch.nn.functional.linear(_norm_ref(c["x"]),
                                                               c["silu"]["w"]))
    c["logits"] = torch.nn.functional.linear(_norm_ref(c["x"]), c["lm"]["w"]).float()
    c["cos_sin"] = ref.rope_cos_sin(128, 8192, 500000.0, None, device="cuda")
    c["pos"] = torch.randint(0, 4000, (mmax,), dtype=torch.int32, device="cuda")
    c["slots"] = torch.randperm(16 * 16, device="cuda")[:mmax].to(torch.int32)
    c["k0"] = torch.randn(16, HKV, 16, 128, dtype=dt, device="cuda")
    c["v0"] = torch.randn(16, HKV, 128, 16, dtype=dt, device="cuda")
    return c


def _refused(fn):
    """A shape the table has no kernel for: check_rc raises on the host-side -1, before any
    launch - so the device has no error pending afterwards either."""
    with pytest.raises(RuntimeError, match=r"launch failed \(rc=-1\)"):
        fn()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("ps", [True, False], ids=["pre-shuffled", "row-major"])
@pytest.mark.parametrize("m", GPU_ROWS)
def test_native_entry_points_follow_the_table(gpu_case, m, ps):
    c, nat = gpu_case, ops._native()
    x = c["x"][:m]
    # plain and residual (ops.linear would take row-major weights past the table to the
    # library GEMM, so the refusals go to the native op itself)
    w = c["plain"][ps]
    if ops.fused_kernel(m, ps, False, "plain") is not None:
        close(ops.linear(x, w, preshuffled=ps), c["exp_plain"][:m], 2e-2 * math.sqrt(K / 4096),
              1e-2)
    else:
        y = torch.empty(m, NOUT, dtype=x.dtype, device="cuda")
        _refused(lambda: nat.skinny_gemm(y, x, w, None, 8, ps, None, 1))
    r = c["res"][:m].clone()
    if ops.fused_kernel(m, ps, False, "resadd") is not None:
        ops.linear(x, w, residual=r, preshuffled=ps)
        close(r, c["exp_plain"][:m].to(x.dtype).float() + c["res"][:m].float(),
              3e-2 * math.sqrt(K / 4096), 1e-2)
    else:
        _refused(lambda: nat.skinny_gemm(r, x, w, r, 8, ps, None, 1))
        assert torch.equal(r, c["res"][:m])
    # qkv + RoPE + paged K/V write
    k1, v1, k2, v2 = c["k0"].clone(), c["v0"].clone(), c["k0"].clone(), c["v0"].clone()

    def qkv():
        return ops.decode_qkv_rope(x, c["qkv"][ps], 1e-5, c["pos"][:m], c["slots"][:m],
                                   c["cos_sin"], k2, v2, HQ, HKV, preshuffled=ps)

    if ops.fused_kernel(m, ps, False, "qkv") is not None:
        q_exp = ref.rope_cache(torch.nn.functional.linear(_norm_ref(x), c["qkv"]["w"]),
                               c["pos"][:m], c["slots"][:m], c["cos_sin"], k1, v1, HQ, HKV, 128)
        close(qkv(), q_exp, 3e-2, 2e-2)
        close(k2, k1, 3e-2, 2e-2)
        close(v2, v1, 3e-2, 2e-2)
    else:
        _refused(qkv)
        assert torch.equal(k2, c["k0"]) and torch.equal(v2, c["v0"])
    # gate_up + SiLU

    def silu():
        return ops.decode_gate_up_silu(x, c["silu"][ps], 1e-5, preshuffled=ps)

    if ops.fused_kernel(m, ps, False, "silu") is not None:
        close(silu(), c["exp_silu"][:m], 4e-2, 4e-2)
    else:
        _refused(silu)
    # LM head + greedy sampler
    V = c["lm"]["w"].shape[0]
    keys = torch.full((m * V // 16,), -1, dtype=torch.int64, device="cuda")
    temp = torch.zeros(m, device="cuda")
    seeds = torch.arange(m, dtype=torch.int64, device="cuda")
    steps = torch.zeros(m, dtype=torch.int64, device="cuda")

    def lm():
        return ops.decode_lm_head_sample(x, c["lm"][ps], 1e-5, temp, seeds, steps, keys,
                                         preshuffled=ps)

    if ops.fused_kernel(m, ps, False, "sample") is not None:
        got = lm()
        top2 = torch.topk(c["logits"][:m], 2, dim=-1)
        for i in range(m):
            g = int(got[i])
            assert g == int(top2.indices[i, 0]) or \
                float(top2.values[i, 0] - c["logits"][i, g]) < 0.05
    else:
        _refused(lm)
