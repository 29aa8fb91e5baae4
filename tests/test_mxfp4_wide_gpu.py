"""The wide kernel's MXFP4 (W4) builds, 33-128 rows over the 4-bit copies: closed-form answers
with torch.equal for the plain / residual epilogues (every row block, loop shape, wave count
and split-K), the norm-fold epilogues against the fp32 reference ops on the dequantised
weights, and the refusals around the explicit route."""
import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# first row of MT 3; full MT 3; first row of MT 4; MT 7 with 12 padded rows; full MT 8
ROWS = (33, 48, 49, 100, 128)
# fewer tiles than a workgroup has waves (idle waves); a second, mostly idle column block
NS = (64, 16 * 9)
# one chunk (prologue only); three (under one period); one 4-period + 1; 22 chunks; 32 chunks
KS = (128, 384, 640, 2816, 4096)
WAVES = (4, 6, 7, 8)


def closed_form_case(N, K, dtype, device):
    """The inputs of test_mxfp4_gpu.test_gemv_closed_form (from a CPU generator, so the values
    are the same wherever they are made): x integers in [-4, 4], codes uniform in 0..15, scale
    bytes uniform in 125..129; and the exact product x W^T in fp64."""
    g = torch.Generator().manual_seed(N * 10007 + K)
    codes = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
    scales = torch.randint(125, 130, (N, K // 32), dtype=torch.uint8, generator=g)
    xs = torch.randint(-4, 5, (max(ROWS), K), generator=g).to(dtype)
    W = ops.dequantize_mxfp4(codes, scales, torch.float32).double()
    want = (xs.double() @ W.t()).to(device)
    return codes.to(device), scales.to(device), xs.to(device), want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_wide_w4_closed_form(N, K, dtype):
    """Every product is a multiple of 2^-3 and every partial sum stays below 2^21 of them, so
    each fp32 sum is exact in any order and across split-K slabs: the output is ONE rounding of
    the fp64 product and the comparison is torch.equal.  The library's own plan, then every
    wave count with split-K 1 and 2 (2 where K has two chunks to split)."""
    codes, scales, xs, want_all = closed_form_case(N, K, dtype, "cuda")
    assert K * 4 * 6 * 4 < 2 ** 21 and float(want_all.abs().max()) < 60000
    wq, sq = ops.preshuffle_mxfp4(codes, scales)
    plans = [(0, 0)] + [(w, s) for w in WAVES for s in (1, 2) if K // 128 >= s]
    g = torch.Generator().manual_seed(K + N)
    res_all = torch.randint(-8, 9, (max(ROWS), N), generator=g).to(dtype).cuda()
    for m in ROWS:
        x = xs[:m]
        want = want_all[:m].to(dtype)
        # the residual-add epilogue: (res + y) with y rounded first
        want_res = (res_all[:m].double() + want.double()).to(dtype)
        for plan in plans:
            ops.set_wide_plan(*plan)
            got = ops.linear(x, wq, w_block_scale=sq, wide_w4=True)
            assert got.dtype == dtype and got.shape == (m, N)
            assert torch.equal(got, want), (m, plan,
                                            float((got.double() - want.double()).abs().max()))
            ops.set_wide_plan(*plan)
            got = ops.linear(x, wq, residual=res_all[:m].clone(), w_block_scale=sq, wide_w4=True)
            assert torch.equal(got, want_res), ("resadd", m, plan)


def test_wide_w4_strided_x_and_rows_past_m_untouched():
    """x rows with a stride, and an output with guard rows after row M."""
    N, K, m = 64, 640, 49
    codes, scales, xs, want_all = closed_form_case(N, K, torch.bfloat16, "cuda")
    wq, sq = ops.preshuffle_mxfp4(codes, scales)
    big = torch.zeros(m, K + 64, dtype=torch.bfloat16, device="cuda")
    big[:, :K] = xs[:m]
    out = torch.full((m + 4, N), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.linear(big[:, :K], wq, out=out[:m], w_block_scale=sq, wide_w4=True)
    assert torch.equal(out[:m], want_all[:m].to(torch.bfloat16))
    assert bool((out[m:] == 7.0).all())


def close(a, b, atol, rtol=0.0):
    a, b = a.float(), b.float()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    assert bool((err <= bound).all()), f"max err {float(err.max())}"


@pytest.mark.parametrize("m", [33, 64, 128])
def test_wide_w4_norm_epilogues_vs_fp32_reference(m):
    """RMSNorm + gate_up + SiLU*up and RMSNorm + QKV + RoPE + paged K/V write at H = 1024
    against the fp32 reference ops on the dequantised weights, with the tolerances of
    test_mxfp4_gpu.test_mxfp4_decode_kernels_vs_fp32_reference (3e-2 / 3e-2: the weight values
    are exact on both sides, what is bounded is the bf16-output and summation-order error)."""
    torch.manual_seed(41)
    dt, H = torch.bfloat16, 1024
    x = torch.randn(m, H, dtype=dt, device="cuda")
    xf = x.float()

    def q(w, rowmap="plain"):
        codes, scales = ops.quantize_mxfp4(w)
        return (*ops.preshuffle_mxfp4(codes, scales, rowmap),
                ops.dequantize_mxfp4(codes, scales, torch.float32))

    eps, inter = 1e-5, 512
    ones = torch.ones(H, dtype=torch.float32, device="cuda")
    wg = torch.randn(2 * inter, H, dtype=dt, device="cuda") * 0.05
    gq, gs, gf = q(wg, "silu")
    exp = ref.silu_and_mul(ref.rms_norm(xf, ones, eps) @ gf.t())
    close(ops.decode_gate_up_silu(x, gq, eps, w_block_scale=gs, wide_w4=True), exp, 3e-2, 3e-2)
    hq, hkv, bs, nb = 8, 2, 16, 32
    wqkv = torch.randn((hq + 2 * hkv) * 128, H, dtype=dt, device="cuda") * 0.05
    kq, ks, kf = q(wqkv, "qkv")
    kc = torch.zeros(nb, hkv, bs, 128, dtype=dt, device="cuda")
    vc = torch.zeros(nb, hkv, 128, bs, dtype=dt, device="cuda")
    kc_r = torch.zeros(nb, hkv, bs, 128, dtype=torch.float32, device="cuda")
    vc_r = torch.zeros(nb, hkv, 128, bs, dtype=torch.float32, device="cuda")
    pos = torch.arange(3, 3 + m, dtype=torch.int32, device="cuda")
    slots = torch.arange(m, dtype=torch.int32, device="cuda") * 3
    assert int(slots.max()) < nb * bs
    cs = ref.rope_cos_sin(128, 256, 500000.0, None, device="cuda")
    got = ops.decode_qkv_rope(x, kq, eps, pos, slots, cs, kc, vc, hq, hkv, w_block_scale=ks,
                              wide_w4=True)
    qkv = ref.rms_norm(xf, ones, eps) @ kf.t()
    exp = ref.rope_cache(qkv, pos, slots, cs, kc_r, vc_r, hq, hkv, 128)
    close(got, exp, 3e-2, 3e-2)
    close(kc, kc_r, 3e-2, 3e-2)
    close(vc, vc_r, 3e-2, 3e-2)


def test_wide_w4_refusals():
    codes = torch.zeros(64, 256, dtype=torch.uint8, device="cuda")
    scales = torch.full((64, 8), 127, dtype=torch.uint8, device="cuda")
    wq, sq = ops.preshuffle_mxfp4(codes, scales)
    x33 = torch.zeros(33, 256, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):  # a default call at 33 rows: still no kernel
        ops.linear(x33, wq, w_block_scale=sq)
    assert ops.linear(x33, wq, w_block_scale=sq, wide_w4=True).shape == (33, 64)
    with pytest.raises(ValueError):  # the explicit route ends at 128 rows
        ops.linear(torch.zeros(129, 256, dtype=torch.bfloat16, device="cuda"), wq,
                   w_block_scale=sq, wide_w4=True)
    # at most 32 rows the explicit choice stays on the 4-bit GEMV: the same bits
    x = torch.randn(17, 256, dtype=torch.bfloat16, device="cuda")
    codes = torch.randint(0, 16, (64, 256), dtype=torch.uint8, device="cuda")
    wq, sq = ops.preshuffle_mxfp4(codes, scales)
    assert torch.equal(ops.linear(x, wq, w_block_scale=sq, wide_w4=True),
                       ops.linear(x, wq, w_block_scale=sq))
    assert ops.skinny_ok(x33, wq, True, mxfp4=True, wide_w4=True)
    assert not ops.skinny_ok(x33, wq, True, mxfp4=True)
