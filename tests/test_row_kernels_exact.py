"""Row kernels against fp64 references that round where the kernels round (tests/helpers.py).

The kernels: rms_norm / fused_add_rms_norm / silu_and_mul / embed (ops/csrc/norm_act.hip),
rope_cache (ops/csrc/rope_cache.hip) and quant_rows_fp8 (ops/csrc/quant_fp8.hip).  The
random-data tests of test_kernels_gpu.py allow 2e-2 + 1e-2 |ref| (the fp8 one a whole code
step), which a sum of squares that misses a vector, a skipped intermediate rounding, round-
toward-zero fp8 codes or a slipped RoPE index all pass.  Here every element is held to the
fp64 evaluation of the documented definition:

* an element is a *boundary* element if an inexact rounding step of it has its fp64 value
  within relative delta of a rounding tie of the target format; every other element must be
  bit-equal to the reference; a boundary element may be off by one representable step per
  rounding it went through (2 for rms_norm and silu_and_mul, 1 for RoPE and an fp8 code).
* delta = 2^-16, from the arithmetic, not from a run: a row sum of up to 16384 squares is at
  most 64 serial fp32 adds per lane plus a shuffle / LDS tree, relative error below about
  75 * 2^-24; rsqrt, one multiply and the division add a few units of 2^-24.  __expf is
  exp2(g * log2 e): the rounded argument costs |g| * 2^-24 relative, v_exp_f32 one ulp; the
  CUDA programming guide's intrinsic table gives the same shape, 2 + floor(|1.16 g|) ulp = 20
  ulp = 2^-19.7 at |g| = 16.  Below delta, so silu_and_mul keeps it; beyond |g| = 16 the
  gate sweep allows 2 steps of T on every element, as specified.
* only inexact roundings count.  The second rounding of rms_norm and silu_and_mul and the
  residual add round a product or sum of two T values that fp32 holds exactly (16 / 22
  significant bits), so the kernel cannot differ there and no allowance is given: this is
  stricter than counting every rounding, and keeps the fp16 share below its cap.
* RoPE measures the window against |x1 c| + |x2 s|, not against the possibly cancelling
  result: that is what the fp32 error of the kernel's two products is relative to.
* the boundary share is a condition (at most 2 % in bf16, 8 % in fp16), checked by the CPU
  tier on exactly the inputs the GPU tier runs.  Measured (bf16 / fp16): rms_norm and
  fused_add_rms_norm 0.57 % / 4.5 %, silu_and_mul 0.92 % / 4.5 %, RoPE with the real table
  1.0 % / 6.7 % (q and K alike); fp8 codes (an 8-steps-per-binade grid) 0.02 % - 0.07 % in
  the norm and SiLU modes, 0.81 % / 0.07 % in plain mode.
* the fp8 SiLU mode inherits the rule: where the silu rounding is a boundary one the kernel
  may hold the neighbouring T value, so the code of either neighbour's product passes.

The CPU tier (unmarked) holds the project's CPU paths to the same comparator on every
GPU-tier input, checks the caps, and checks that fourteen deliberately wrong references fail.
The fp8 norm modes and the SiLU mode of the CPU path get a looser rule: the CPU path rounds
the value to T (twice for the norms, once for SiLU-mul) before it quantises and the kernel
keeps fp32, so there only "within one code step of the fp64 reference" is asserted.

Dispatch reached (as read from the launchers):
  rms_norm, rows < 1024 ("waves4", 4 waves per row): hidden <= 2048 ITERS 1, <= 4096 ITERS 2,
    <= 8192 ITERS 4; 2056 / 4104 / 8184 leave the last iteration partly empty.
  rows >= 1024 ("wave1", one wave per row): hidden 1024 ITERS 2, 1032 / 2048 ITERS 4, 4096
    ITERS 8, 8184 / 8192 ITERS 16; 1027 rows leave one live wave in the last workgroup (the
    dead-wave return).
  hidden > 8192 ("block", 256 threads per row): 8200 .. 16384, 2 to 8 iterations.
  quant_rows_fp8: 8 .. 4096 (256 x 2), 4104 / 8192 (256 x 4), 8200 / 16384 (1024 x 2),
    16392 / 32768 (1024 x 4), 32776 two passes.
  rope_cache: 16-token tiles for T >= 16 with hq % hkv == 0, the per-token kernel for T < 16
    and for (5, 2) heads at every T.
  embed: hidden 4096 is two trips of the 256-thread copy loop.

Findings: the fp8 conversion (v_cvt_pk_fp8_f32) rounds exact ties to even, subnormal range
included, as torch does, and keeps the sign of a zero (-0 gives code 0x80); no kernel defect
was found.  The CPU path of quant_rows_fp8 differs from the kernel in the norm and SiLU
modes (it quantises values already rounded to T).  The bindings of rms_norm, fused_add_rms_norm, silu_and_mul and
rope_cache did not check row strides, base alignment, output shape / dtype or the weight;
ops/csrc/bindings.cpp now refuses those before a launch (test_refusals_*).
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.ops import reference as ref
from helpers import (QUANT_EXACT_SCALE_MODES, ROW_SENTINEL, ROW_SHARE_CAP, assert_rows,
                     e4m3_midpoints, e4m3_values, embed_ref, fp8_codes64, needle_positions,
                     needle_rows, quant_model, quant_values64, quant_violations,
                     rms_norm_ref64, rope_exact_qkv, rope_exact_table, rope_ref64,
                     round_fmt, row_mismatches, silu_neighbours64, silu_ref64)

DT = [torch.bfloat16, torch.float16]
EPS = 1e-5
gpu = pytest.mark.gpu
LLAMA3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
          "original_max_position_embeddings": 8192}


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), ops._load_error


def _name(dtype):
    return str(dtype).split(".")[-1]


def _sentinel(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, ROW_SENTINEL & 0xFF, dtype=torch.uint8)
    return torch.full(shape, ROW_SENTINEL, dtype=torch.int16).view(dtype)


class Guard:
    """A GPU buffer of sentinel patterns with one spare row either side; ``win`` is its
    [rows, width] window (a column slice when ``stride`` > width).  ``intact()``: nothing
    outside the window changed."""

    def __init__(self, rows, width, dtype, stride=0, off=0, fill=None):
        stride = stride or width
        assert off + width <= stride
        self.raw = _sentinel((rows + 2, stride), dtype).cuda()
        self.win = self.raw[1:rows + 1, off:off + width]
        self.box = (rows, width, off)
        if fill is not None:
            self.win.copy_(fill)

    def intact(self):
        rows, width, off = self.box
        b = self.raw.clone()
        b[1:rows + 1, off:off + width] = _sentinel((1,), b.dtype).cuda()
        return torch.equal(b.cpu(), _sentinel(tuple(b.shape), b.dtype))

    def untouched(self):
        return torch.equal(self.raw.cpu(), _sentinel(tuple(self.raw.shape), self.raw.dtype))


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.dtype != torch.uint8:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return torch.equal(a, b)


# =========================================================================================
# The cases (shared by both tiers)
# =========================================================================================
# path -> (row counts, hiddens)
RMS_PATHS = {"waves4": ((1, 3), (8, 256, 2048, 2056, 3072, 4096, 4104, 8184, 8192)),
             "wave1": ((1024, 1027), (1024, 1032, 2048, 4096, 8184, 8192)),
             "block": ((1, 3), (8200, 12288, 16376, 16384))}
RMS_CASES = [(p, h) for p, (_, hs) in RMS_PATHS.items() for h in hs]
RMS_STRIDED = [("waves4", 4104), ("wave1", 1032), ("block", 16376)]
RMS_NEEDLE = [("waves4", 8), ("waves4", 2048), ("waves4", 2056), ("waves4", 4096),
              ("waves4", 8184), ("wave1", 1024), ("wave1", 2048), ("wave1", 4096),
              ("wave1", 8184), ("block", 8200), ("block", 16376), ("block", 16384)]


@functools.lru_cache(maxsize=2)
def _rms_case(path, hidden, dtype):
    """Random rows of mixed magnitude; row 1 is all zeros and row 2 so small that eps is a
    tenth of its mean square.  ``r`` = round(x + res) is also the input of the plain norm, so
    one reference serves rms_norm and fused_add_rms_norm."""
    rows = max(RMS_PATHS[path][0])
    g = torch.Generator().manual_seed(hidden * 7 + rows)
    mag = torch.pow(2.0, torch.randint(-3, 4, (rows, 1), generator=g).float())
    x = torch.randn(rows, hidden, generator=g) * mag
    res = torch.randn(rows, hidden, generator=g) * mag
    if rows > 2:
        x[1], res[1] = 0.0, 0.0
        x[2] = torch.randn(hidden, generator=g) * 0.007
        res[2] = torch.randn(hidden, generator=g) * 0.007
    x, res = x.to(dtype), res.to(dtype)
    w = (torch.rand(hidden, generator=g) + 0.5).to(dtype)
    out, near, r = rms_norm_ref64(x, w, EPS, res)
    return SimpleNamespace(x=x, res=res, w=w, r=r, out=out, near=near, hidden=hidden)


def _needle_case(path, hidden, dtype):
    rows = len(needle_positions(hidden))
    if path == "wave1":
        rows = max(rows, 1027)
    assert path == "wave1" or rows < 1024
    return needle_rows(hidden, rows, dtype)


SILU_INTERS = (8, 256, 2048, 2056, 3584, 14336)


@functools.lru_cache(maxsize=2)
def _silu_case(inter, dtype):
    g = torch.Generator().manual_seed(inter)
    x = torch.randn(5, 2 * inter, generator=g) * 3
    x[:, :inter].clamp_(-16.0, 16.0)
    x = x.to(dtype)
    out, near, _ = silu_ref64(x)
    return SimpleNamespace(x=x, out=out, near=near, inter=inter)


def _silu_sweep(dtype):
    """One row: gates +-{0, 2^-20, 1, 8, 16, 30, 60} and +- the largest finite value, each
    against ups of +-1, 2 and two random values."""
    big = float(torch.finfo(dtype).max)
    gates = [s * v for v in (0.0, 2.0 ** -20, 1.0, 8.0, 16.0, 30.0, 60.0, big) for s in (1, -1)]
    ups = [1.0, -1.0, 2.0, 0.7265625, -1.3125]
    g = torch.tensor([a for a in gates for _ in ups])
    u = torch.tensor([b for _ in gates for b in ups])
    assert g.numel() % 8 == 0
    x = torch.cat([g, u])[None, :].to(dtype)
    out, near, _ = silu_ref64(x)
    return SimpleNamespace(x=x, out=out, near=near, inter=g.numel())


EMBED_CASES = [(h, r, v) for h in (8, 256, 2048, 2056, 4096) for r in (1, 300) for v in (1, 1000)]


def _embed_inputs(hidden, rows, vocab, dtype):
    """(table, [ids ...], [prev ...]): ids hold -5, vocab and 2^31 - 1, prev -1 and 2^40."""
    g = torch.Generator().manual_seed(hidden + rows + vocab)
    table = torch.randn(vocab, hidden, generator=g).to(dtype)
    if rows == 1:
        ids = [torch.tensor([v], dtype=torch.int32) for v in (-5, vocab, 2 ** 31 - 1, vocab // 2)]
        prev = [torch.tensor([v, 0, 0, 0], dtype=torch.int64) for v in (-1, 2 ** 40, vocab // 3)]
        return table, ids, prev
    i = torch.randint(0, vocab, (rows,), generator=g, dtype=torch.int32)
    i[0], i[rows // 2], i[-1] = -5, 2 ** 31 - 1, vocab
    p = torch.randint(0, vocab, (rows + 3,), generator=g, dtype=torch.int64)
    p[0], p[rows - 1], p[7] = -1, 2 ** 40, vocab
    return table, [i], [p]


# (T, hq, hkv, head_dim, block size, slots): tiles need T >= 16 and hq % hkv == 0
ROPE_CFG = [(1, 32, 8, 128, 16, "perm"), (1, 24, 8, 64, 128, "midpage"),
            (15, 8, 1, 64, 32, "holes"), (15, 4, 4, 128, 64, "perm"),
            (16, 32, 8, 128, 16, "holes"), (17, 8, 1, 64, 32, "midpage"),
            (31, 4, 4, 128, 64, "perm"), (48, 24, 8, 64, 128, "deadtile"),
            (48, 32, 8, 128, 32, "midpage"), (31, 24, 8, 64, 16, "holes"),
            (16, 5, 2, 128, 16, "perm"), (17, 5, 2, 64, 32, "holes"),
            (31, 5, 2, 128, 64, "midpage"), (48, 5, 2, 64, 128, "deadtile")]
ROPE_MAX_POS = 256


def _rope_kernel(cfg):
    t, hq, hkv = cfg[:3]
    return "tile" if t >= 16 and hq % hkv == 0 else "token"


def test_rope_cfg_covers_every_axis_with_every_kernel():
    for kern in ("tile", "token"):
        cs = [c for c in ROPE_CFG if _rope_kernel(c) == kern]
        assert {c[3] for c in cs} == {64, 128} and {c[4] for c in cs} == {16, 32, 64, 128}
        assert {c[0] for c in cs} >= ({16, 17, 31, 48} if kern == "tile" else {1, 15, 16, 17, 31, 48})
        assert {c[5] for c in cs} == {"perm", "midpage", "holes", "deadtile"}
    assert {c[1:3] for c in ROPE_CFG} == {(32, 8), (8, 1), (4, 4), (24, 8), (5, 2)}


@functools.lru_cache(maxsize=4)
def _rope_case(cfg, kind, dtype):
    t, hq, hkv, d, bs, how = cfg
    g = torch.Generator().manual_seed(t * 131 + hq + d + bs)
    w = (hq + 2 * hkv) * d
    nb = (t + bs) // bs + 3
    if kind == "exact":
        qkv, table = rope_exact_qkv(t, w, dtype), rope_exact_table(ROPE_MAX_POS, d)
    else:
        qkv = torch.randn(t, w, generator=g).to(dtype)
        table = ref.rope_cos_sin(d, ROPE_MAX_POS, 500000.0, LLAMA3)
    pos = torch.randint(0, ROPE_MAX_POS, (t,), generator=g, dtype=torch.int32)
    pos[0] = 0
    if t > 1 or bs == 16:
        pos[-1] = ROPE_MAX_POS - 1
    if how == "perm":
        slots = torch.randperm(nb * bs, generator=g)[:t].to(torch.int32)
    else:  # in order from mid-page: a 16-token tile straddles pages
        slots = torch.arange(t, dtype=torch.int32) + bs // 2 + 3
    if how == "holes":  # -1 at the first and last token of every tile (and of a short one)
        for a in range(0, t, 16):
            slots[a] = -1
            slots[min(a + 15, t - 1)] = -1
    if how == "deadtile":
        slots[16:32] = -1
    k0, v0 = _sentinel((nb, hkv, bs, d), dtype), _sentinel((nb, hkv, d, bs), dtype)
    q, qn, kc, kn, vc = rope_ref64(qkv, pos, slots, table, k0, v0, hq, hkv, d)
    return SimpleNamespace(qkv=qkv, pos=pos, slots=slots, table=table, k0=k0, v0=v0, q=q, qn=qn,
                           kc=kc, kn=kn, vc=vc, cfg=cfg)


QUANT_WIDTHS = (8, 256, 4096, 4104, 8192, 8200, 16384, 16392, 32768, 32776)
QUANT_STRIDED = (4104, 32776)


@functools.lru_cache(maxsize=2)
def _quant_case(mode, width, dtype):
    """Three rows; row 1 is all zeros; the row amax sits in the last 8-wide vector.  The SiLU
    rows plant it as gate 4, up +-16 (about 62.9) above every other product (below 48)."""
    g = torch.Generator().manual_seed(mode * 100003 + width)
    mag = torch.tensor([[0.25], [0.0], [3.0]])
    w = res = None
    if mode == 1:
        gate = (torch.randn(3, width, generator=g) * 2).clamp(-8.0, 8.0)
        up = torch.randn(3, width, generator=g).clamp(-5.5, 5.5)
        gate[:, -3], up[:, -3] = 4.0, torch.tensor([16.0, -16.0, 16.0])
        gate[1], up[1] = 0.0, 0.0
        x = torch.cat([gate, up], dim=1).to(dtype)
    else:
        x = torch.randn(3, width, generator=g) * mag
        x[:, -3] = x.abs().amax(-1) * 1.5
        x[1] = 0.0  # +0 throughout: a -0 would rightly come out as code 0x80
        x = x.to(dtype)
        if mode in (0, 3):
            w = (torch.rand(width, generator=g) + 0.5).to(dtype)
            w[-3] = 1.5
        if mode == 3:  # the planted amax of x + res: res is 0 there
            res = (torch.randn(3, width, generator=g) * mag).to(dtype)
            res[:, -3] = 0.0
            res[1] = 0.0
            x[:, -3] = ((x.float() + res.float()).abs().amax(-1) * 1.5).to(dtype)
    v64, r = quant_values64(x, mode, w, EPS, res)
    alts = silu_neighbours64(x) if mode == 1 else []
    return SimpleNamespace(x=x, w=w, res=res, v64=v64, r=r, mode=mode, width=width, alts=alts)


CENSUS_K = (-3, 0, 5)


def _census_case(dtype):
    """Row i: every finite e4m3fn value (254 codes, both zeros) times 2^k, two zeros of
    padding, in a fixed shuffled order: amax = 448 * 2^k, scale 2^k, every code its own."""
    codes, vals = e4m3_values()
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(5))
    codes = torch.cat([codes, torch.zeros(2, dtype=torch.uint8)])[perm]
    vals = torch.cat([vals, torch.zeros(2)])[perm]
    x = torch.stack([vals * 2.0 ** k for k in CENSUS_K])
    assert bool((x.to(dtype).float() == x).all())
    return x.to(dtype), codes[None, :].expand(3, -1).contiguous(), torch.tensor(
        [2.0 ** k for k in CENSUS_K])


def _ties_case(dtype):
    mid = e4m3_midpoints()
    x = torch.cat([mid, torch.tensor([448.0, 0.0, 0.0, 0.0])])[None, :]
    assert x.shape[1] % 8 == 0 and bool((x.to(dtype).float() == x).all())
    return x.to(dtype), x.to(torch.float8_e4m3fn).view(torch.uint8)


# =========================================================================================
# CPU tier
# =========================================================================================
def _share(stats, op, near):
    n, k = stats.get(op, (0, 0))
    stats[op] = (n + near.numel(), k + int(near.sum()))


def _check_caps(stats, dtype):
    for op, (n, k) in stats.items():
        print(f"SHARE {op} {_name(dtype)} {k / n:.4%} of {n}")
        assert k / n <= ROW_SHARE_CAP[dtype], (op, k / n)


@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("path", list(RMS_PATHS))
def test_cpu_rms_norm_and_boundary_share(path, dtype):
    """ops.rms_norm / ops.fused_add_rms_norm on CPU tensors satisfy the comparator on every
    GPU-tier input of the path (needle rows with no allowance), and the boundary share of
    each input set stays under its cap."""
    stats = {}
    for hidden in RMS_PATHS[path][1]:
        c = _rms_case(path, hidden, dtype)
        what = f"cpu rms_norm {path} {hidden} {_name(dtype)}"
        assert_rows(ops.rms_norm(c.r, c.w, EPS), c.out, c.near, 2, what)
        res = c.res.clone()
        got = ops.fused_add_rms_norm(c.x, res, c.w, EPS)
        assert_rows(got, c.out, c.near, 2, what + " fused")
        assert_rows(res, c.r, what=what + " residual")
        _share(stats, "rms_norm", c.near)
        assert float(c.near.float().mean()) <= ROW_SHARE_CAP[dtype], what
        assert not bool(c.out.float().isnan().any())
        if c.x.shape[0] > 2:
            assert bool((c.out[1].float() == 0).all())
            ms = float(c.r[2].double().pow(2).mean())
            assert 0.05 <= EPS / ms <= 0.2, "eps must weigh about a tenth of row 2's mean square"
    for p, hidden in RMS_NEEDLE:
        if p == path:
            x, w, exp = _needle_case(p, hidden, dtype)
            assert_rows(ops.rms_norm(x, w, 0.0), exp, what=f"cpu needle {p} {hidden}")
            assert_rows(rms_norm_ref64(x, w, 0.0)[0], exp, what=f"ref64 needle {p} {hidden}")
            half = (x.float() / 2).to(dtype)
            res = half.clone()
            assert_rows(ops.fused_add_rms_norm(half, res, w, 0.0), exp, what="cpu needle fused")
            assert_rows(res, x, what="cpu needle residual")
    _check_caps(stats, dtype)


@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_cpu_silu_embed_and_boundary_share(dtype):
    stats = {}
    for inter in SILU_INTERS:
        c = _silu_case(inter, dtype)
        assert_rows(ops.silu_and_mul(c.x), c.out, c.near, 2, f"cpu silu {inter} {_name(dtype)}")
        _share(stats, "silu_and_mul", c.near)
    s = _silu_sweep(dtype)
    assert_rows(ops.silu_and_mul(s.x), s.out, s.near, 2, "cpu silu gate sweep")
    _check_caps(stats, dtype)
    for hidden, rows, vocab in EMBED_CASES:
        table, ids, prev = _embed_inputs(hidden, rows, vocab, dtype)
        for i in ids:
            assert _same_bits(ops.embed(table, i), embed_ref(table, i))
            for p in prev:
                for flag in (0, 1):
                    got = ops.embed(table, i, p, torch.tensor([flag], dtype=torch.int32))
                    assert _same_bits(got, embed_ref(table, i, p, flag))


@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_cpu_rope_cache_and_boundary_share(dtype):
    stats = {}
    for cfg in ROPE_CFG:
        t, hq, hkv, d, bs, how = cfg
        for kind in ("exact", "real"):
            c = _rope_case(cfg, kind, dtype)
            kc, vc = c.k0.clone(), c.v0.clone()
            q = ops.rope_cache(c.qkv, c.pos, c.slots, c.table, kc, vc, hq, hkv, d)
            what = f"cpu rope {kind} {cfg} {_name(dtype)}"
            near = (None, None) if kind == "exact" else (c.qn, c.kn)
            assert_rows(q, c.q, near[0], 1, what + " q")
            assert_rows(kc, c.kc, near[1], 1, what + " k")
            assert _same_bits(vc, c.vc), what + " v"
            if kind == "real":
                _share(stats, "rope q", c.qn)
                live = int((c.slots >= 0).sum())
                if live:
                    stats["rope k"] = tuple(a + b for a, b in zip(
                        stats.get("rope k", (0, 0)), (live * hkv * d, int(c.kn.sum()))))
    _check_caps(stats, dtype)


def _quant_cpu(c):
    res = None if c.res is None else c.res.clone()
    q, s = ops.quant_rows_fp8(c.x, c.mode, c.w, EPS, res)
    return q, s, res


@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_cpu_quant_rows_fp8(mode, dtype):
    """The CPU path of ops.quant_rows_fp8 on every GPU-tier row.  Plain mode: the full rule
    (scale within one fp32 step, round-to-nearest-even codes, the adjacent code only within
    delta of a midpoint).  Norm and SiLU modes: the CPU path rounds the value to T before it
    quantises (rms_norm twice, silu_and_mul once more than the kernel), so only "every code
    within one step of the fp64 reference's code at the returned scale" is asserted."""
    n = k = 0
    for width in QUANT_WIDTHS:
        c = _quant_case(mode, width, dtype)
        q, s, res = _quant_cpu(c)
        if mode == 2:
            assert quant_violations(q, s, c.v64, True) == [], (mode, width)
        else:
            assert row_mismatches(q, fp8_codes64(c.v64 / s.double())[0],
                                  torch.ones_like(q, dtype=torch.bool), 1)[0] == 0, (mode, width)
        if mode == 3:
            assert _same_bits(res, c.r)
        near = fp8_codes64(c.v64 / quant_model(c.v64)[1].double()[:, None])[1]
        n, k = n + near.numel(), k + int(near.sum())
        assert bool((c.v64[1] == 0).all())
        if mode == 1:  # the planted amax: not near a tie itself, and above everything else
            s64 = torch.tensor([4.0 / (1.0 + math.exp(-4.0))], dtype=torch.float64)
            assert not bool(round_fmt(s64, dtype)[1].any())
            rest = c.v64.abs().clone()
            rest[:, -3] = 0
            assert bool((rest.amax(-1)[[0, 2]] < 0.9 * c.v64[[0, 2], -3].abs()).all())
    print(f"SHARE quant mode {mode} {_name(dtype)} {k / n:.4%} of {n}")
    assert k / n <= ROW_SHARE_CAP[dtype]
    if mode == 2:
        x, codes, scales = _census_case(dtype)
        q, s = ops.quant_rows_fp8(x)
        assert _same_bits(q, codes) and torch.equal(s.reshape(-1), scales)
        x, codes = _ties_case(dtype)
        q, s = ops.quant_rows_fp8(x)
        assert _same_bits(q, codes) and float(s) == 1.0
        assert _same_bits(fp8_codes64(x.double())[0], codes), "fp64 model: ties to even"


@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_wrong_references_are_caught(dtype):
    """Fourteen wrong references, each a plain Python variant of the fp64 definition, fail
    the comparator on GPU-tier inputs - and the unmodified definition passes on the same.
    (The residual variant normalises the unrounded sum: an add carried out in T itself is
    correctly rounded and so bit-identical to the single rounding of the exact sum.)"""
    caught = []

    def expect_fail(name, bad):
        assert bad > 0, f"wrong reference {name} passes"
        caught.append(name)

    c = _rms_case("waves4", 3072, dtype)
    assert row_mismatches(rms_norm_ref64(c.x, c.w, EPS, c.res)[0], c.out, c.near, 2)[0] == 0
    for m in ("ss_drop_last", "ss_drop_mid", "no_round", "mean_pad2048", "norm_of_unrounded_sum"):
        out = rms_norm_ref64(c.x, c.w, EPS, c.res, mutant=m)[0]
        expect_fail("rms " + m, row_mismatches(out, c.out, c.near, 2)[0])
    s = _silu_case(2056, dtype)
    expect_fail("silu no_round",
                row_mismatches(silu_ref64(s.x, mutant="no_round")[0], s.out, s.near, 2)[0])

    p = _quant_case(2, 4104, dtype)
    assert quant_violations(*quant_model(p.v64), p.v64, True) == []
    for m in ("rtz", "scale_drop_last"):
        expect_fail("fp8 " + m, len(quant_violations(*quant_model(p.v64, m), p.v64, True)))
    x = _census_case(dtype)[0].double()
    assert quant_violations(*quant_model(x), x, True) == []
    expect_fail("fp8 flush_subnormal",
                len(quant_violations(*quant_model(x, "flush_subnormal"), x, True)))

    for cfg in (ROPE_CFG[4], ROPE_CFG[12]):  # one per kernel
        r = _rope_case(cfg, "exact", dtype)
        t, hq, hkv, d = cfg[:4]
        for m in ("pair_shift", "pos_plus1", "v_swapped", "k_slot_plus1"):
            q, _, kc, _, vc = rope_ref64(r.qkv, r.pos, r.slots, r.table, r.k0, r.v0, hq, hkv, d, m)
            bad = (row_mismatches(q, r.q)[0] + row_mismatches(kc, r.kc)[0]
                   + row_mismatches(vc, r.vc)[0])
            expect_fail(f"rope {m}", bad)
    real = _rope_case(ROPE_CFG[4], "real", dtype)
    t, hq, hkv, d = ROPE_CFG[4][:4]
    q = rope_ref64(real.qkv, real.pos, real.slots, real.table, real.k0, real.v0, hq, hkv, d,
                   "pos_plus1")[0]
    expect_fail("rope pos_plus1 (real table)", row_mismatches(q, real.q, real.qn, 1)[0])

    table, ids, prev = _embed_inputs(256, 300, 1000, dtype)
    bad = int((embed_ref(table, ids[0], mutant="no_clamp") != embed_ref(table, ids[0])).sum())
    bad_prev = int((embed_ref(table, ids[0], prev[0], 1, mutant="no_clamp")
                    != embed_ref(table, ids[0], prev[0], 1)).sum())
    expect_fail("embed no_clamp", min(bad, bad_prev))
    assert len({n.split(" (")[0] for n in caught}) == 14, caught


# =========================================================================================
# GPU tier
# =========================================================================================
def _run_norm(x, res, w, eps, exp, near, exp_res, fused, strided, what):
    """One launch with guarded buffers.  ``x`` and ``res`` are the fused op's operands; the
    plain norm reads ``exp_res`` = round(x + res)."""
    rows, h = exp.shape
    dt = exp.dtype
    sx, so, sr = (h + 24, h + 16, h + 40) if strided else (0, 0, 0)
    out = Guard(rows, h, dt, so, 8 if strided else 0)
    wg = w.cuda()
    if fused:
        xin = Guard(rows, h, dt, sx, 16 if strided else 0, fill=x.cuda())
        rg = Guard(rows, h, dt, sr, 0, fill=res.cuda())
        ops.fused_add_rms_norm(xin.win, rg.win, wg, eps, out=out.win)
        assert_rows(rg.win, exp_res, what=what + " residual")
        assert rg.intact(), what + ": residual guard"
    else:
        xin = Guard(rows, h, dt, sx, 16 if strided else 0, fill=exp_res.cuda())
        ops.rms_norm(xin.win, wg, eps, out=out.win)
    assert_rows(out.win, exp, near, 2, what)
    assert out.intact(), what + ": out guard"
    assert xin.intact() and _same_bits(xin.win, x if fused else exp_res), what + ": x changed"


def _run_rms_case(path, hidden, dtype, strided):
    c = _rms_case(path, hidden, dtype)
    for rows in RMS_PATHS[path][0]:
        for fused in (False, True):
            what = f"rms {path} {rows}x{hidden} {_name(dtype)}{' fused' if fused else ''}" \
                   f"{' strided' if strided else ''}"
            _run_norm(c.x[:rows], c.res[:rows], c.w, EPS, c.out[:rows], c.near[:rows], c.r[:rows],
                      fused, strided, what)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("path,hidden", RMS_CASES)
def test_rms_norm_rows(native, path, hidden, dtype):
    """Random rows, a zero row (zeros, not NaN) and a row where eps is a tenth of the mean
    square; rms_norm and fused_add_rms_norm at both row counts of the path; the written-back
    residual bit-equal to the singly rounded sum."""
    _run_rms_case(path, hidden, dtype, strided=False)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("path,hidden", RMS_STRIDED)
def test_rms_norm_strided(native, path, hidden, dtype):
    """x, out and residual are column slices of wider buffers: three different row strides,
    all multiples of 8 and greater than hidden."""
    _run_rms_case(path, hidden, dtype, strided=True)


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("path,hidden", RMS_NEEDLE)
def test_rms_norm_needle(native, path, hidden, dtype):
    """Row r holds 63/64 of its energy in one 8-wide vector that sweeps the row; rms is
    exactly 8 and every output exactly representable: compared bitwise, nothing allowed."""
    x, w, exp = _needle_case(path, hidden, dtype)
    half = (x.float() / 2).to(dtype)
    for fused in (False, True):
        _run_norm(half, half, w, 0.0, exp, None, x, fused, False,
                  f"needle {path} {x.shape[0]}x{hidden} {_name(dtype)} fused={fused}")


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_rms_norm_refused_and_empty(native, dtype):
    """hidden 16392 (too wide) and 12 (not whole vectors) raise and leave the output alone;
    zero rows are a no-op."""
    for hidden in (16392, 12):
        stride = (hidden + 15) // 16 * 16  # keeps the rows 16-byte aligned: the width is refused
        x = Guard(3, hidden, dtype, stride, fill=torch.ones(3, hidden, dtype=dtype).cuda())
        r = Guard(3, hidden, dtype, stride, fill=torch.ones(3, hidden, dtype=dtype).cuda())
        out = Guard(3, hidden, dtype, stride)
        w = torch.ones(hidden, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError):
            ops.rms_norm(x.win, w, EPS, out=out.win)
        with pytest.raises(RuntimeError):
            ops.fused_add_rms_norm(x.win, r.win, w, EPS, out=out.win)
        torch.cuda.synchronize()
        assert out.untouched() and r.intact() and bool((r.win == 1).all())
    c = _rms_case("waves4", 256, dtype)
    out = Guard(0, 256, dtype)
    r = Guard(0, 256, dtype)
    ops.rms_norm(c.x[:0].cuda(), c.w.cuda(), EPS, out=out.win)
    ops.fused_add_rms_norm(c.x[:0].cuda(), r.win, c.w.cuda(), EPS, out=out.win)
    torch.cuda.synchronize()
    assert out.untouched() and r.untouched()


def _run_silu(x, exp, near, strided, what):
    rows, inter = exp.shape
    dt = exp.dtype
    xin = Guard(rows, 2 * inter, dt, 2 * inter + 24 if strided else 0, 8 if strided else 0,
                fill=x.cuda())
    out = Guard(rows, inter, dt, inter + 16 if strided else 0, 16 if strided else 0)
    ops.silu_and_mul(xin.win, out=out.win)
    assert_rows(out.win, exp, near, 2, what)
    assert out.intact() and xin.intact() and _same_bits(xin.win, x), what + ": guards"


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("inter", SILU_INTERS)
def test_silu_and_mul_rows(native, inter, dtype):
    c = _silu_case(inter, dtype)
    for rows in (1, 5):
        for strided in (False, True):
            _run_silu(c.x[:rows], c.out[:rows], c.near[:rows], strided,
                      f"silu {rows}x{inter} {_name(dtype)} strided={strided}")


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_silu_and_mul_gate_sweep(native, dtype):
    """Gates from 0 to where __expf saturates and the largest finite value: the boundary rule
    up to |g| = 16, 2 steps beyond; gate * up or its overflow at the largest gate."""
    s = _silu_sweep(dtype)
    _run_silu(s.x, s.out, s.near, False, f"silu gate sweep {_name(dtype)}")


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("hidden,rows,vocab", EMBED_CASES)
def test_embed_rows(native, hidden, rows, vocab, dtype):
    """Out-of-range ids (-5, vocab, 2^31 - 1; prev -1, 2^40) read row 0 or row vocab - 1;
    contiguous and strided out; bitwise."""
    table, ids, prev = _embed_inputs(hidden, rows, vocab, dtype)
    tg = table.cuda()
    for strided in (False, True):
        for i in ids:
            calls = [(None, 0)] + [(p, f) for p in prev for f in (0, 1)]
            for p, flag in calls:
                out = Guard(rows, hidden, dtype, hidden + 16 if strided else 0, 8 if strided else 0)
                if p is None:
                    ops.embed(tg, i.cuda(), out=out.win)
                else:
                    ops.embed(tg, i.cuda(), p.cuda(),
                              torch.tensor([flag], dtype=torch.int32, device="cuda"), out=out.win)
                assert _same_bits(out.win, embed_ref(table, i, p, flag)), (i[:1], flag, strided)
                assert out.intact()


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("cfg", ROPE_CFG, ids=lambda c: "-".join(map(str, c)))
def test_rope_cache_rows(native, cfg, kind, dtype):
    """exact: a table of 0, +-1 and powers of two and integer qkv - q, K and V bitwise.
    real: the llama3-scaled table and random qkv - one rounding under the boundary rule, V
    bitwise.  qkv rows and q_out are column slices of wider buffers; the caches start as
    sentinels and every element no live slot owns must keep them."""
    t, hq, hkv, d, bs, how = cfg
    c = _rope_case(cfg, kind, dtype)
    w = (hq + 2 * hkv) * d
    qkv = Guard(t, w, dtype, w + 24, 8, fill=c.qkv.cuda())
    qo = Guard(t, hq * d, dtype, hq * d + 16, 8)
    kc, vc = c.k0.cuda(), c.v0.cuda()
    got = ops.rope_cache(qkv.win, c.pos.cuda(), c.slots.cuda(), c.table.cuda(), kc, vc, hq, hkv, d,
                         q_out=qo.win.unflatten(1, (hq, d)))
    what = f"rope {_rope_kernel(cfg)} {kind} {cfg} {_name(dtype)}"
    near = (None, None) if kind == "exact" else (c.qn, c.kn)
    assert_rows(got, c.q, near[0], 1, what + " q")
    assert_rows(kc, c.kc, near[1], 1, what + " k")
    assert _same_bits(vc, c.vc), what + ": V cache"
    assert qo.intact() and qkv.intact() and _same_bits(qkv.win, c.qkv), what + ": guards"


def _run_quant(c, rows, strided, what):
    mode, width = c.mode, c.width
    dt = c.x.dtype
    xw = c.x.shape[1]
    x = Guard(rows, xw, dt, xw + 8 if strided else 0, fill=c.x[:rows].cuda())
    q = Guard(rows, width, torch.uint8, width + 16 if strided else 0, 8 if strided else 0)
    res = None
    if mode == 3:
        res = Guard(rows, width, dt, width + 24 if strided else 0, 8 if strided else 0,
                    fill=c.res[:rows].cuda())
    scale = torch.full((rows + 4,), -7.0, dtype=torch.float32, device="cuda")
    ops._native().quant_rows_fp8(q.win, scale, x.win, None if c.w is None else c.w.cuda(), mode,
                                 EPS, None if res is None else res.win)
    assert bool((scale[rows:] == -7.0).all()), what + ": scale guard"
    bad = quant_violations(q.win, scale[:rows], c.v64[:rows], mode in QUANT_EXACT_SCALE_MODES,
                           alts=[a[:rows] for a in c.alts])
    print(f"QUANT {what} scale={scale[:rows].tolist()} violations={bad}")
    assert bad == [], what
    if rows > 1:
        assert float(scale[1]) == 1.0 and bool((q.win[1] == 0).all()), what + ": zero row"
    if res is not None:
        assert _same_bits(res.win, c.r[:rows]) and res.intact(), what + ": residual"
    assert q.intact() and x.intact() and _same_bits(x.win, c.x[:rows]), what + ": guards"


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("width", QUANT_WIDTHS)
def test_quant_rows_fp8_rows(native, width, mode, dtype):
    """Scale: one fp32 step around fp32(amax) / 448 (plain, SiLU), relative delta around the
    fp64 value (norm modes).  Codes: round-to-nearest-even of value / returned scale, the
    adjacent code only within delta of a midpoint.  SiLU mode: where the silu rounding itself
    is a boundary one the kernel may hold the neighbouring T value, so the code may be the one
    of either neighbour's product (the boundary rule of silu_and_mul carried through).  A zero
    row: scale 1, zero codes.  Mode 3's residual bit-equal to the singly rounded sum."""
    c = _quant_case(mode, width, dtype)
    for rows in (1, 3):
        _run_quant(c, rows, False, f"quant mode {mode} {rows}x{width} {_name(dtype)}")
    if width in QUANT_STRIDED:
        _run_quant(c, 3, True, f"quant mode {mode} 3x{width} {_name(dtype)} strided")


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_quant_rows_fp8_code_census(native, dtype):
    """Every finite e4m3fn value of both signs, subnormals included, times 2^k: the scale is
    bit-equal to 2^k and every code is that value's own encoding."""
    x, codes, scales = _census_case(dtype)
    q, s = ops.quant_rows_fp8(x.cuda())
    assert torch.equal(s.reshape(-1).cpu(), scales), s
    bad = (q.cpu() != codes).nonzero()
    print("CENSUS mismatches", [(int(r), hex(int(codes[r, c])), hex(int(q[r, c]))) for r, c in bad])
    assert bad.numel() == 0


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_quant_rows_fp8_ties(native, dtype):
    """Exact midpoints between adjacent codes, the subnormal range included: ties to even, as
    torch's conversion to float8_e4m3fn gives them."""
    x, codes = _ties_case(dtype)
    q, s = ops.quant_rows_fp8(x.cuda())
    bad = (q.cpu() != codes).nonzero()
    print("TIES scale", float(s), "mismatches",
          [(float(x[r, c]), hex(int(codes[r, c])), hex(int(q[r, c]))) for r, c in bad])
    assert float(s) == 1.0 and bad.numel() == 0


# ---- host-side refusals ------------------------------------------------------------------
# Every misaligned operand below belongs to a call the launcher refuses anyway (too wide a
# row, inter or head_dim not whole vectors), and the tests match the alignment message: were
# a binding check missing the test would fail on the message without a kernel ever reading a
# misaligned view.
def _odd_stride(rows, width, dtype):
    return torch.ones(rows, width + 1, dtype=dtype, device="cuda")[:, :width]


def _one_in(rows, width, dtype):
    return torch.ones(rows, width + 8, dtype=dtype, device="cuda")[:, 1:width + 1]


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_refusals_rms_norm(native, dtype):
    h = 16392
    w = torch.ones(h, dtype=dtype, device="cuda")
    good = torch.ones(3, h, dtype=dtype, device="cuda")
    for bad, msg in ((_odd_stride(3, h, dtype), "multiple of 8"), (_one_in(3, h, dtype), "aligned")):
        out = Guard(3, h, dtype)
        res = Guard(3, h, dtype)
        with pytest.raises(RuntimeError, match=msg):
            ops.rms_norm(bad, w, EPS, out=out.win)
        with pytest.raises(RuntimeError, match=msg):
            ops.rms_norm(good, w, EPS, out=bad)
        with pytest.raises(RuntimeError, match=msg):
            ops.fused_add_rms_norm(bad, res.win, w, EPS, out=out.win)
        with pytest.raises(RuntimeError, match=msg):
            ops.fused_add_rms_norm(good, bad, w, EPS, out=out.win)
        torch.cuda.synchronize()
        assert out.untouched() and res.untouched() and bool((bad == 1).all())
    out = Guard(3, h, dtype)
    with pytest.raises(RuntimeError, match="weight"):
        ops.rms_norm(good, w[:-8], EPS, out=out.win)
    with pytest.raises(RuntimeError, match="out must match"):
        ops.rms_norm(good, w, EPS, out=out.win[:, :-8])
    assert out.untouched()


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_refusals_silu_and_mul(native, dtype):
    inter = 12  # not whole vectors: the launcher refuses it whatever the alignment
    for bad, msg in ((_odd_stride(3, 2 * inter, dtype), "multiple of 8"),
                     (_one_in(3, 2 * inter, dtype), "aligned")):
        out = Guard(3, inter, dtype, 16)
        with pytest.raises(RuntimeError, match=msg):
            ops.silu_and_mul(bad, out=out.win)
        assert out.untouched()
    x = torch.ones(3, 2 * inter, dtype=dtype, device="cuda")
    out = Guard(3, inter, dtype, 16)
    with pytest.raises(RuntimeError, match="inter must be a multiple of 8"):
        ops.silu_and_mul(x, out=out.win)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.silu_and_mul(x, out=_odd_stride(3, inter, dtype))
    torch.cuda.synchronize()
    assert out.untouched()


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_refusals_rope_cache(native, dtype):
    t, hq, hkv, d, bs = 3, 2, 1, 24, 16  # head_dim 24: the launcher refuses it
    w = (hq + 2 * hkv) * d
    pos = torch.zeros(t, dtype=torch.int32, device="cuda")
    slots = torch.arange(t, dtype=torch.int32, device="cuda")
    table = torch.ones(8, d, device="cuda")
    good = torch.ones(t, w, dtype=dtype, device="cuda")
    kc, vc = _sentinel((2, hkv, bs, d), dtype).cuda(), _sentinel((2, hkv, d, bs), dtype).cuda()
    qo = Guard(t, hq * d, dtype)

    def call(qkv, q_out):
        ops.rope_cache(qkv, pos, slots, table, kc, vc, hq, hkv, d, q_out=q_out)

    for mk, msg in ((_odd_stride, "multiple of 8"), (_one_in, "aligned")):
        with pytest.raises(RuntimeError, match=msg):
            call(mk(t, w, dtype), qo.win.unflatten(1, (hq, d)))
        with pytest.raises(RuntimeError, match=msg):
            call(good, mk(t, hq * d, dtype).unflatten(1, (hq, d)))
    with pytest.raises(RuntimeError, match="head_dim must be a multiple of 16"):
        call(good, qo.win.unflatten(1, (hq, d)))
    torch.cuda.synchronize()
    assert qo.untouched()
    assert _same_bits(kc, _sentinel(tuple(kc.shape), dtype))
    assert _same_bits(vc, _sentinel(tuple(vc.shape), dtype))
