"""ops.expand_mxfp4: one projection's pre-shuffled 4-bit codes and block scales into row-major
16-bit values, bit for bit the dequantised weight, for the three tile row maps."""
import pytest
import torch

from agentic_traffic_testing_amd import ops

pytestmark = pytest.mark.gpu

# scale bytes for which every e2m1 value times the block scale is a normal number of the type
SCALES = {torch.bfloat16: (97, 157), torch.float16: (114, 140)}
# (N, K): one tile row x one chunk; an odd chunk count (one live wave in the last workgroup);
# the small model's gate_up.  "qkv" needs whole 128-row heads: N 64 / 96 -> 128 / 256
SHAPES = ((64, 128), (96, 384), (5632, 1024))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rowmap", ["plain", "qkv", "silu"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_expand_equals_unshuffle_dequantize(N, K, rowmap, dtype):
    if rowmap == "qkv":
        N = -(-N // 128) * 128
    lo, hi = SCALES[dtype]
    g = torch.Generator().manual_seed(N + K)
    codes = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
    codes.view(-1)[:16] = torch.arange(16, dtype=torch.uint8)  # all 16 codes, whatever the draw
    scales = torch.randint(lo, hi + 1, (N, K // 32), dtype=torch.uint8, generator=g)
    scales.view(-1)[:2] = torch.tensor([lo, hi], dtype=torch.uint8)
    wq, sq = ops.preshuffle_mxfp4(codes.cuda(), scales.cuda(), rowmap)
    want = ops.dequantize_mxfp4(*ops.unshuffle_mxfp4(wq, sq, rowmap), dtype)
    assert torch.equal(want, ops.dequantize_mxfp4(codes.cuda(), scales.cuda(), dtype))
    out = torch.full((N, K), float("nan"), dtype=dtype, device="cuda")
    assert ops.expand_mxfp4(wq, sq, rowmap, out) is out
    assert not bool(torch.isnan(out).any()), "an element was not written"
    assert torch.equal(out, want)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)), "the sign of a zero"


def test_expand_into_a_slice_of_a_larger_scratch():
    """As the model uses it: a [N, K] view at the head of a flat scratch; nothing past it moves."""
    N, K = 96, 384
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g).cuda()
    scales = torch.randint(120, 131, (N, K // 32), dtype=torch.uint8, generator=g).cuda()
    wq, sq = ops.preshuffle_mxfp4(codes, scales, "silu")
    scratch = torch.full((N * K + 4096,), 3.0, dtype=torch.bfloat16, device="cuda")
    ops.expand_mxfp4(wq, sq, "silu", scratch[:N * K].view(N, K))
    assert torch.equal(scratch[:N * K].view(N, K),
                       ops.dequantize_mxfp4(codes, scales, torch.bfloat16))
    assert bool((scratch[N * K:] == 3.0).all())


def test_expand_refuses_bad_arguments():
    wq = torch.zeros(64, 64, dtype=torch.uint8, device="cuda")
    sq = torch.full((64, 4), 127, dtype=torch.uint8, device="cuda")
    out = torch.empty(64, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        ops.expand_mxfp4(wq, sq, "rows", out)
    with pytest.raises(RuntimeError):  # qkv: whole 128-row heads
        ops.expand_mxfp4(wq, sq, "qkv", out)
    with pytest.raises(RuntimeError):  # out of another shape
        ops.expand_mxfp4(wq, sq, "plain", torch.empty(64, 256, dtype=torch.bfloat16,
                                                      device="cuda"))
    with pytest.raises(RuntimeError):  # fp32 out
        ops.expand_mxfp4(wq, sq, "plain", out.float())
