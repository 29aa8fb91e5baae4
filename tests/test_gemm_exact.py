"""Wide small-M GEMM (ops/csrc/wide.h), mid-M GEMM (ops/csrc/midm.h) and the bf16 prefill GEMM
(ops/csrc/prefill_gemm.hip) on exact integer operands (builders: tests/helpers.py).

The random-operand tests (test_wide_gemm.py, test_midm_gemm.py, test_prefill_gemm.py) allow
about 2e-2 absolute plus 1-4 % relative at model shapes: one lost, doubled or misplaced product,
an inv_rms or fp8 row scale taken from a neighbouring row, or a store past row M all pass.
Here every operand is a small nonzero integer (times a power of two), so fp32 accumulation is
exact in any order and for any split; the expectation is the exact product rounded once where
wide::epi_apply rounds (the mid-M kernel calls the same epi_load / epi_apply: midm.h, the end
of midm_kernel and midm_reduce_kernel) and the comparison is bit equality.  The only allowance
is the row-kernel tests' boundary rule for SiLU, whose exp is inexact: elements silu_ref64 /
round_fmt mark ``near`` may differ by the steps test_row_kernels_exact.py allows.

Shapes follow the loops, not the models.  K slices (chunks of 128 columns):
  * wide kernel: 4 weight stages, 2 x buffers - whole periods of 4 chunks then a peeled tail
    of up to 3: slices of 1 .. 9 chunks are no period with each tail, one period with each
    tail, two periods, two periods plus one.
  * mid-M kernel, row blocks up to 128 rows (bmt <= 8, every one built with XD = 1): three x
    buffers and three weight stages, period 3: 1 .. 7 chunks (and 8 for one-chunk slices at
    S = 8).
  * mid-M kernel, bmt 10 and 12 (XD = 0, wstages = 3): period 6 with a tail of up to 5:
    1 .. 13 chunks.
  * the XD = 0 loop with wstages(bmt) = 4 is compiled for no built row-block height
    (ATTA_MIDM_TU gives every bmt <= 8 the XD = 1 loop), so it has no case.
Rows sit on every 16-row-block edge of the wide kernel and on both sides of every row-block
multiple of the mid-M kernel; outputs go to a view of a sentinel-filled buffer whose rows past
M must stay untouched; K and V go to sentinel-filled paged caches compared as a whole.

The CPU tier asserts the builders' conditions for every case, the literal (K, S) lists, the
routing, and that every wrong kernel the exact data is meant to expose changes the expectation
of every case it applies to.  test_comparison_sees_one_wrong_weight_row is the same check on
the device: a launch over weights with two rows exchanged must be reported.

fp8 gate rows: the issue's row scale 2^((5 n) % 4 - 2) reaches 2, which would take gates of
+-206 / 16 past SILU_EXACT_GATE, so the gate rows' scales carry 2^-5 instead of the 16-bit
cases' 1 / 16 in the weights (helpers.GEMM_FP8_GATE_SHIFT); the scales of a tile still differ
by factors of 2 to 8.

Findings: every case passes by bit equality on an MI355X (SiLU: inside the boundary rule); no
kernel defect was found.  The mid-M K loop with four weight stages and two x buffers (XD = 0,
wstages(bmt) = 4) is dead code in the shipped builds.
"""
import functools

import pytest
import torch

from agentic_traffic_testing_amd import ops
from helpers import (GEMM_BS, GEMM_EPS, GEMM_EXACT_MAX, GEMM_HKV, GEMM_HQ, GEMM_NB,
                     GEMM_OPERAND_MUTANTS, ROW_DELTA, ROW_SHARE_CAP, SILU_EXACT_GATE,
                     assert_rows, gemm_exact_case, gemm_exact_expected, gemm_fp8_codes,
                     gemm_mutate, gemm_sentinel, gemm_slice_partials_max, round_fmt, row_ok)

BF16, FP16 = torch.bfloat16, torch.float16
gpu = pytest.mark.gpu
GUARD = 32                      # sentinel rows behind row M of every output
SILU_STEPS = 2                  # test_row_kernels_exact.py: steps a boundary SiLU element may move


def _name(dtype):
    return str(dtype).split(".")[-1]


# =========================================================================================
# K slices: chunk counts per pipeline and the (K, S) pairs that produce them
# =========================================================================================
def pipeline_chunks(period: int):
    """Chunks per slice that walk a loop of whole ``period``-chunk periods plus a peeled tail
    of up to period - 1: no period with each tail (1 .. period - 1), one period with each tail
    (period .. 2 period - 1), two periods and two periods plus one."""
    return list(range(1, 2 * period + 2))


def slice_chunks(nch: int, s: int):
    """Chunks of each of the s slices of nch chunks ([i nch / s, (i + 1) nch / s): wide.h c0 /
    c1, midm.h the same)."""
    return [(i + 1) * nch // s - i * nch // s for i in range(s)]


WIDE_PERIOD = 4
WIDE_SPLITS = [(2, 2), (4, 4), (7, 3), (9, 4), (9, 2), (13, 2), (8, 8), (10, 5)]  # (chunks, S)
WIDE_KS = [(128 * n, 1) for n in pipeline_chunks(WIDE_PERIOD)] + \
          [(128 * n, s) for n, s in WIDE_SPLITS]
MIDM_SPLITS = (1, 2, 3, 4, 8)


def midm_period(bmt: int) -> int:
    """Period of the K loop the build of this row-block height runs (midm.h: XD = 1 for
    bmt <= 8, else two x buffers with wstages(bmt) = 3 weight stages)."""
    return 3 if bmt <= 8 else 6


def midm_ks(bmt: int):
    chunks = pipeline_chunks(midm_period(bmt))
    if chunks[-1] < 8:
        chunks.append(8)   # S = 8 needs 8 chunks: one-chunk slices in eight slabs
    return [(128 * n, s) for n in chunks for s in MIDM_SPLITS if s <= n]


def test_chunk_counts():
    assert pipeline_chunks(4) == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert pipeline_chunks(3) == [1, 2, 3, 4, 5, 6, 7]
    assert pipeline_chunks(6) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    assert slice_chunks(7, 3) == [2, 2, 3] and slice_chunks(9, 4) == [2, 2, 2, 3]
    assert slice_chunks(13, 2) == [6, 7] and slice_chunks(8, 8) == [1] * 8
    assert WIDE_KS == [(128, 1), (256, 1), (384, 1), (512, 1), (640, 1), (768, 1), (896, 1),
                       (1024, 1), (1152, 1), (256, 2), (512, 4), (896, 3), (1152, 4), (1152, 2),
                       (1664, 2), (1024, 8), (1280, 5)]
    # every slice length 1 .. 7 also occurs in a split launch (slab writer + reduce)
    assert {n for k, s in WIDE_KS if s > 1 for n in slice_chunks(k // 128, s)} == set(range(1, 8))
    assert [midm_period(b) for b in ops.MIDM_BUILT] == [3, 3, 3, 3, 3, 6, 6]
    assert midm_ks(3) == [
        (128, 1), (256, 1), (256, 2), (384, 1), (384, 2), (384, 3),
        (512, 1), (512, 2), (512, 3), (512, 4), (640, 1), (640, 2), (640, 3), (640, 4),
        (768, 1), (768, 2), (768, 3), (768, 4), (896, 1), (896, 2), (896, 3), (896, 4),
        (1024, 1), (1024, 2), (1024, 3), (1024, 4), (1024, 8)]
    assert midm_ks(8) == midm_ks(3)
    by_k = {}
    for k, s in midm_ks(12):
        by_k.setdefault(k, []).append(s)
    assert midm_ks(10) == midm_ks(12)
    assert by_k == {128: [1], 256: [1, 2], 384: [1, 2, 3], 512: [1, 2, 3, 4], 640: [1, 2, 3, 4],
                    768: [1, 2, 3, 4], 896: [1, 2, 3, 4], 1024: [1, 2, 3, 4, 8],
                    1152: [1, 2, 3, 4, 8], 1280: [1, 2, 3, 4, 8], 1408: [1, 2, 3, 4, 8],
                    1536: [1, 2, 3, 4, 8], 1664: [1, 2, 3, 4, 8]}
    # unsplit, every chunk count of the build's pipeline runs
    for b in ops.MIDM_BUILT:
        assert {k // 128 for k, s in midm_ks(b) if s == 1} >= set(pipeline_chunks(midm_period(b)))


# =========================================================================================
# Launch lists (shared by the CPU tier, which checks every case, and the GPU tier)
# =========================================================================================
WIDE_MS = (17, 31, 32, 33, 48, 49, 64, 65, 80, 96, 97, 112, 113, 127, 128)
WIDE_LOW_MS = (1, 15, 16)       # the MT = 1 build, reached with set_wide_min_rows(1, 1)
WIDE_ROWS = 128
WIDE_WAVES = (4, 6, 7, 8)
WIDE_NS = (16, 368)             # one tile; 23 tiles: idle waves in the last column block
SILU_NS = (64, 368)             # inter 32 and 184
QKV_N = (GEMM_HQ + 2 * GEMM_HKV) * 128
MIDM_NS = (16, 112, 128, 144, 368)   # 1, 7, 8, 9 and 23 tiles at 8 tiles per workgroup
MIDM_ROWS = 401
FP8_WIDE_WAVES = (4, 7, 8)
FP8_WIDE_KS = [(512, 1), (640, 1), (768, 1), (896, 1), (896, 3)]
FP8_MIDM = (3, 8, 12)
FP8_MIDM_KS = [(512, 1), (512, 2), (896, 1), (896, 2)]
PREFILL_MS = (1, 63, 64, 65, 257, 300)
PREFILL_KS = tuple(32 * n for n in (1, 2, 3, 4, 5, 8, 9))
PREFILL_PLANS = [(s, bm) for s in ("hybrid", "streamk", "dp", "splitk") for bm in (64, 128, 256)]


def wide_norm_fits(waves: int, m: int) -> bool:
    """wide.h norm_fits: the builds whose RMSNorm fold spills are not built."""
    mt = (m + 15) // 16
    return not ((mt == 8 and waves in (6, 7)) or (mt == 7 and waves == 6))


def midm_ms(bmt: int):
    bm = 16 * bmt
    ms = {129, 143, 144, 145}
    for j in range(1, 400 // bm + 1):
        if 128 < bm * j <= 400:
            ms.update((bm * j - 1, bm * j, bm * j + 1))
    return sorted(ms)


def midm_launches(bmt: int, ns=MIDM_NS, ks=None):
    """(m, n, k, s): every row count with every (k, s) pair of this row-block height (the
    row-block edges meet the K loop, the slab writer and the reduce), the column counts taken
    in turn, then every (m, n) pair (the edges meet the grid) with the K pairs in turn."""
    ms = midm_ms(bmt)
    b = midm_ks(bmt) if ks is None else ks
    out = [(m, ns[(i * len(b) + j) % len(ns)], k, s)
           for i, m in enumerate(ms) for j, (k, s) in enumerate(b)]
    have = {(m, n) for m, n, _, _ in out}
    rest = [(m, n) for m in ms for n in ns if (m, n) not in have]
    return out + [mn + b[i % len(b)] for i, mn in enumerate(rest)]


def midm_grid(bmt: int, m: int, n_tiles: int, s: int) -> int:
    return -(-m // (16 * bmt)) * -(-n_tiles // 8) * s


def fp8_wide_first_row() -> int:
    return next(m for m in range(1, 200) if ops.fused_kernel(m, True, True, "plain") == "wide")


def fp8_wide_ms():
    first = fp8_wide_first_row()
    return tuple(sorted({first} | {m for m in WIDE_MS if m >= first}))


@functools.lru_cache(maxsize=4)
def _case(epi, rows, n, k, fp8=False):
    return gemm_exact_case(epi, rows, n, k, fp8)


def all_case_keys():
    """(epi, rows, n, k, fp8) of every case a GPU test of this file builds."""
    keys = []
    for k in sorted({k for k, _ in WIDE_KS}):
        keys += [(e, WIDE_ROWS, n, k, False) for e in ("plain", "resadd") for n in WIDE_NS]
        keys += [("qkv", WIDE_ROWS, QKV_N, k, False)]
        keys += [("silu", WIDE_ROWS, n, k, False) for n in SILU_NS]
    for k in sorted({k for b in ops.MIDM_BUILT for k, _ in midm_ks(b)}):
        keys += [(e, MIDM_ROWS, n, k, False) for e in ("plain", "resadd") for n in MIDM_NS]
        if k <= 1024:
            keys += [("qkv", MIDM_ROWS, QKV_N, k, False)]
            keys += [("silu", MIDM_ROWS, n, k, False) for n in SILU_NS]
    for k in sorted({k for k, _ in FP8_WIDE_KS}):
        keys += [(e, WIDE_ROWS, 368, k, True) for e in ("plain", "resadd", "silu")]
        keys += [("qkv", WIDE_ROWS, QKV_N, k, True)]
    for k in sorted({k for k, _ in FP8_MIDM_KS}):
        keys += [(e, MIDM_ROWS, 368, k, True) for e in ("plain", "resadd", "silu")]
        keys += [("qkv", MIDM_ROWS, QKV_N, k, True)]
    for k in PREFILL_KS:
        keys += [("plain", 300, 256, k, False), ("resadd", 300, 256, k, False)]
    return keys


# =========================================================================================
# CPU tier
# =========================================================================================
def _inv_rms_holds(c, dtype):
    """T(acc * scale * inv_rms) in fp32 arithmetic, inv_rms up to 2 ulp off either way, is
    the integer sum times the row scale."""
    acc = (c.x @ c.w.t())                                  # fp32, exact
    if c.wscale is not None:
        acc = acc * c.wscale[None, :]
    ms = (c.x * c.x).sum(1) / c.k
    assert torch.equal(ms, torch.pow(torch.tensor(4.0), (torch.arange(len(ms)) % 3).float()))
    inv = torch.rsqrt(ms + GEMM_EPS)
    want = c.ints().float() * (c.w[:, 0] / c.w_int[:, 0].float())[None, :]
    if c.wscale is not None:
        want = want * c.wscale[None, :]
    want = want.to(dtype)
    assert float(((inv.double() * torch.sqrt(ms.double())) - 1).abs().max()) < 6e-6
    for _ in range(2):
        inv = torch.nextafter(inv, torch.zeros_like(inv))
    for _ in range(5):
        if not torch.equal((acc * inv[:, None]).to(dtype).view(torch.int16),
                           want.view(torch.int16)):
            return False
        inv = torch.nextafter(inv, torch.full_like(inv, 2.0 ** 20))
    return True


def test_builder_conditions():
    first = True
    for key in all_case_keys():
        epi, rows, n, k, fp8 = key
        c = _case(*key)
        assert bool((c.x != 0).all()) and bool((c.w_int != 0).all()) and bool((c.w != 0).all())
        ints = c.ints()
        assert int(ints.abs().max()) <= GEMM_EXACT_MAX[BF16] <= GEMM_EXACT_MAX[FP16], key
        assert float((ints.abs() > GEMM_EXACT_MAX[BF16]).float().mean()) == 0.0
        if epi == "plain" and rows == WIDE_ROWS and not fp8:   # the bf16 slabs stay exact
            for kk, s in WIDE_KS:
                if kk == k and s > 1:
                    assert gemm_slice_partials_max(c, s) <= GEMM_EXACT_MAX[BF16], (key, s)
        if fp8:
            codes = gemm_fp8_codes(c.w_int)
            assert torch.equal(codes.view(torch.float8_e4m3fn).float(), c.w_int.float())
            idx = ops._rowmap_index(c.w.shape[0], c.rowmap, "cpu")
            s = c.wscale if idx is None else c.wscale[idx]
            s = s.reshape(-1, 16)
            assert bool((s.max(1).values >= 2 * s.min(1).values).all())   # every tile
            assert bool((torch.log2(c.wscale) % 1 == 0).all())
        for dtype in ((BF16, FP16) if epi in ("plain", "qkv") else (BF16,)):
            if c.norm:
                assert _inv_rms_holds(c, dtype), key
            e = gemm_exact_expected(c, dtype)
            assert bool(torch.isfinite(e["y"].float()).all())
            if epi == "plain":   # every stored value is the integer itself
                w = ints.double() if not fp8 else ints.double() * c.wscale.double()[None, :]
                assert torch.equal(e["y"].double(), w)
            if epi == "silu":
                inter = c.w.shape[0] // 2
                g = (ints[:, :inter].double() * (c.w[:inter, 0] / c.w_int[:inter, 0]).double())
                if fp8:
                    g = g * c.wscale[:inter].double()[None, :]
                assert float(g.abs().max()) <= SILU_EXACT_GATE and bool(((g * 128) % 1 == 0).all())
                if not fp8:
                    assert bool(((g * 16) % 1 == 0).all())
                share = float(e["near"].float().mean())
                assert share <= ROW_SHARE_CAP[dtype], (key, share)
                if first:
                    print(f"GEMM-EXACT silu boundary share {key}: {share:.4%}")
                    first = False
            if epi == "qkv":
                live = c.slots[c.slots >= 0]
                assert int((c.slots < 0).sum()) == 1 and len(set(live.tolist())) == len(live)
                page = (c.slots // GEMM_BS)[c.slots >= 0]
                assert float((page[1:] != page[:-1]).float().mean()) > 0.9
                sent = gemm_sentinel(e["k"].shape, dtype)
                assert int((e["k"].view(torch.int16) != sent.view(torch.int16)).any(-1).sum()) \
                    == len(live) * GEMM_HKV


def test_prefill_silu_boundary_share():
    for k in PREFILL_KS:
        exp, near = _prefill_silu_expected(k)
        assert float(near.float().mean()) <= ROW_SHARE_CAP[BF16]
        assert bool(torch.isfinite(exp.float()).all())


def test_wrong_references_are_caught():
    """Every wrong kernel the exact operands are meant to expose changes at least one expected
    element of every case it applies to (cases cut to 34 live rows: the mutants touch rows 15,
    16, M - 2 and M - 1)."""
    m = 34
    applied = {}
    for key in all_case_keys():
        epi, rows, n, k, fp8 = key
        c = _case(*key).cut(m)
        dtypes = (BF16, FP16) if epi in ("plain", "qkv") else (BF16,)
        for dtype in dtypes:
            base = gemm_exact_expected(c, dtype, m)

            def differs(e):
                return any(not torch.equal(e[f].view(torch.int16), base[f].view(torch.int16))
                           for f in ("y", "k", "v") if f in base)

            for name in GEMM_OPERAND_MUTANTS:
                mc = gemm_mutate(c, name, m)
                if mc is None:
                    continue
                assert differs(gemm_exact_expected(mc, dtype, m)), (key, dtype, name)
                applied[name] = applied.get(name, 0) + 1
            if c.norm:
                assert differs(gemm_exact_expected(c, dtype, m, inv_shift=1)), (key, "inv_next")
                applied["inv_next"] = applied.get("inv_next", 0) + 1
            if epi == "qkv":
                assert differs(gemm_exact_expected(c, dtype, m, rope_mutant="pair_shift")), key
                assert differs(gemm_exact_expected(c, dtype, m, v_as_k=True)), key
                applied["rope"] = applied.get("rope", 0) + 1
    assert set(applied) == set(GEMM_OPERAND_MUTANTS) | {"inv_next", "rope"}, applied


def test_routing_and_grids():
    for epi in ("plain", "resadd", "qkv", "silu"):
        for m in WIDE_MS:
            assert ops.fused_kernel(m, True, False, epi) == "wide"
        for b in ops.MIDM_BUILT:
            for m in midm_ms(b):
                assert ops.fused_kernel(m, True, False, epi) == "midm"
                assert ops.fused_kernel(m, True, True, epi) == "midm"
        for m in fp8_wide_ms():
            assert ops.fused_kernel(m, True, True, epi) == "wide"
    assert fp8_wide_first_row() == 33
    assert fp8_wide_ms() == (33, 48, 49, 64, 65, 80, 96, 97, 112, 113, 127, 128)
    assert midm_ms(3)[:7] == [129, 143, 144, 145, 191, 192, 193] and midm_ms(5)[-1] == 401
    assert midm_ms(8) == [129, 143, 144, 145, 255, 256, 257, 383, 384, 385]
    assert max(m for b in ops.MIDM_BUILT for m in midm_ms(b)) == MIDM_ROWS
    # both arms of the XCD-aware block order: grids that are and are not a multiple of 8
    for b in ops.MIDM_BUILT:
        grids = [midm_grid(b, m, n // 16, s) for m, n, k, s in midm_launches(b)]
        assert any(g % 8 == 0 for g in grids) and any(g % 8 for g in grids), b
        seen = midm_launches(b)
        assert {(m, n) for m, n, _, _ in seen} == {(m, n) for m in midm_ms(b) for n in MIDM_NS}
        assert {(k, s) for _, _, k, s in seen} == set(midm_ks(b))


# =========================================================================================
# GPU tier
# =========================================================================================
@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), ops._load_error
    ops.ensure_splitk_workspace("cuda")


class Dev:
    """One case's operands and expectation on the GPU in one dtype."""

    def __init__(self, c, dtype, strided=False):
        self.c, self.dtype = c, dtype
        rows, k = c.x.shape
        if strided:   # x: a column window of a wider buffer (x.stride(0) > K)
            wide = torch.full((rows, k + 64), 3.0).to(dtype).cuda()
            wide[:, 32:32 + k] = c.x.to(dtype).cuda()
            self.x = wide[:, 32:32 + k]
            assert self.x.stride(0) > k
        else:
            self.x = c.x.to(dtype).cuda()
        if c.wscale is None:
            self.w = ops.preshuffle(c.w.to(dtype).cuda(), c.rowmap)
            self.ws = None
        else:
            self.w = ops.preshuffle_fp8(gemm_fp8_codes(c.w_int).cuda(), c.rowmap)
            self.ws = c.wscale.cuda().contiguous()
        self.exp = gemm_exact_expected(c, dtype)
        self.y = self.exp["y"].cuda()
        width = self.y.shape[1]
        self.sent = gemm_sentinel((rows + GUARD, width), dtype).cuda()
        self.big = self.sent.clone()
        self.want = self.sent.clone()
        if c.epi == "resadd":
            self.res = c.res.to(dtype).cuda()
        if c.epi == "qkv":
            self.pos, self.slots, self.table = c.pos.cuda(), c.slots.cuda(), c.table.cuda()
            self.ksent = gemm_sentinel((GEMM_NB, GEMM_HKV, GEMM_BS, 128), dtype).cuda()
            self.vsent = gemm_sentinel((GEMM_NB, GEMM_HKV, 128, GEMM_BS), dtype).cuda()
            self.kc, self.vc = self.ksent.clone(), self.vsent.clone()
            self.live = torch.nonzero(c.slots >= 0).reshape(-1)           # CPU
            sl = c.slots[self.live].long()
            self.page, self.off = (sl // GEMM_BS).cuda(), (sl % GEMM_BS).cuda()
            self.krows = self.exp["k"][sl // GEMM_BS, :, sl % GEMM_BS, :].cuda()
            self.vrows = self.exp["v"][sl // GEMM_BS, :, :, sl % GEMM_BS].cuda()
            self.kwant, self.vwant = None, None

    def prepare(self, m):
        """Expectation of the first m rows (the whole guarded buffer and caches)."""
        self.want[:m + GUARD].copy_(self.sent[:m + GUARD])
        self.want[:m].copy_(self.y[:m])
        if self.c.epi == "qkv":
            nl = int((self.live < m).sum())
            self.kwant, self.vwant = self.ksent.clone(), self.vsent.clone()
            self.kwant[self.page[:nl], :, self.off[:nl], :] = self.krows[:nl]
            self.vwant[self.page[:nl], :, :, self.off[:nl]] = self.vrows[:nl]

    def launch(self, m):
        c, big = self.c, self.big
        big[:m + GUARD].copy_(self.sent[:m + GUARD])
        x = self.x[:m]
        if c.epi == "plain":
            ops.linear(x, self.w, out=big[:m], preshuffled=True, w_scale=self.ws)
        elif c.epi == "resadd":
            big[:m].copy_(self.res[:m])
            ops.linear(x, self.w, residual=big[:m], preshuffled=True, w_scale=self.ws)
        elif c.epi == "silu":
            ops.decode_gate_up_silu(x, self.w, GEMM_EPS, out=big[:m], preshuffled=True,
                                    w_scale=self.ws, ksplit=1)
        else:
            self.kc.copy_(self.ksent)
            self.vc.copy_(self.vsent)
            ops.decode_qkv_rope(x, self.w, GEMM_EPS, self.pos[:m], self.slots[:m], self.table,
                                self.kc, self.vc, GEMM_HQ, GEMM_HKV,
                                q_out=big[:m].view(m, GEMM_HQ, 128), preshuffled=True,
                                w_scale=self.ws, ksplit=1)

    def check(self, m, what):
        i16 = torch.int16
        ok = torch.equal(self.big[:m + GUARD].view(i16), self.want[:m + GUARD].view(i16))
        if ok and self.c.epi == "qkv":
            ok = torch.equal(self.kc.view(i16), self.kwant.view(i16)) and \
                torch.equal(self.vc.view(i16), self.vwant.view(i16))
        if ok:
            return
        got = self.big[:m + GUARD].cpu()
        assert torch.equal(got[m:].view(i16), self.sent[:GUARD].cpu().view(i16)), \
            f"{what}: rows past M = {m} were written"
        near = self.exp.get("near")
        _report(got[:m], self.exp["y"][:m], None if near is None else near[:m],
                SILU_STEPS if near is not None else 0, what)
        if self.c.epi == "qkv":
            _report(self.kc.cpu().reshape(-1, 128), self.kwant.cpu().reshape(-1, 128), None, 0,
                    what + " K cache")
            _report(self.vc.cpu().reshape(-1, GEMM_BS), self.vwant.cpu().reshape(-1, GEMM_BS),
                    None, 0, what + " V cache")


def _report(got, exp, near, steps, what):
    """Slow path: name the first bad element, then assert with the shared comparator."""
    ok, _ = row_ok(got, exp, near, steps)
    if not bool(ok.all()):
        r, col = (int(v) for v in (~ok).nonzero()[0])
        what = (f"{what}: first bad element [{r}, {col}] got {float(got[r, col])!r} expected "
                f"{float(exp[r, col])!r}")
    assert_rows(got, exp, near, steps, what)


def _counters_zero():
    _, counters = ops._SPLITK_WS[torch.cuda.current_device()]
    return bool((counters == 0).all())


def _run_wide(epi, dtype, ns, pairs, ms, waves, fp8=False, strided_at=None):
    """Every (n, (k, s), m, waves) of the lists on the wide kernel; returns launches."""
    launches = 0
    for n in ns:
        for k, s in pairs:
            c = _case(epi, WIDE_ROWS, n, k, fp8)
            devs = [Dev(c, dtype)]
            if strided_at == (n, k, s):
                devs.append(Dev(c, dtype, strided=True))
            for d in devs:
                for m in ms:
                    assert ops.fused_kernel(m, True, fp8, epi) == "wide"
                    d.prepare(m)
                    for wv in waves:
                        if c.norm and not wide_norm_fits(wv, m):
                            continue
                        ops.set_wide_plan(wv, s)
                        d.launch(m)
                        d.check(m, f"wide {epi} {_name(dtype)} fp8={fp8} m={m} n={n} k={k} "
                                   f"waves={wv} split={s} strided={d is not devs[0]}")
                        launches += 1
    return launches


def _wide_test(epi, kernel_name, runs):
    """runs: (dtype, ns, pairs, half slabs) on the 16-bit wide kernel, rows 1 .. 128."""
    launches = cases = 0
    prev = list(ops._wide_min_rows)
    try:
        ops.set_wide_min_rows(1, 1)
        for dtype, ns, pairs, half in runs:
            ops.set_splitk_half(half)
            launches += _run_wide(epi, dtype, ns, pairs, WIDE_LOW_MS + WIDE_MS, WIDE_WAVES,
                                  strided_at=(ns[-1], 896, 3))
            cases += len(ns) * len(pairs)
    finally:
        ops.set_splitk_half(False)
        ops.set_wide_min_rows(*prev)
    assert _counters_zero()
    assert launches > 0
    print(f"GEMM-EXACT {kernel_name} {epi} cases={cases} launches={launches}")


SPLIT_KS = [p for p in WIDE_KS if p[1] > 1]


@gpu
@pytest.mark.parametrize("epi", ["plain", "silu"])
def test_comparison_sees_one_wrong_weight_row(native, epi):
    """The device-side comparison itself: the kernels run on weights with two rows of one tile
    exchanged, held against the unchanged expectation, must be reported - on the wide and the
    mid-M path alike."""
    for rows, m, plan in ((WIDE_ROWS, 33, lambda: ops.set_wide_plan(4, 1)),
                          (MIDM_ROWS, 145, lambda: ops.set_midm_plan(3, 1))):
        c = _case(epi, rows, 368, 512)
        d = Dev(c, BF16)
        d.w = Dev(gemm_mutate(c, "w_rows_in_tile", m), BF16).w
        d.prepare(m)
        plan()
        d.launch(m)
        with pytest.raises(AssertionError, match="first bad element"):
            d.check(m, f"negative control {epi}")


@gpu
def test_wide_plain(native):
    _wide_test("plain", "wide", [(BF16, WIDE_NS, WIDE_KS, False), (BF16, WIDE_NS, SPLIT_KS, True),
                                 (FP16, WIDE_NS, WIDE_KS, False)])


@gpu
def test_wide_residual(native):
    _wide_test("resadd", "wide", [(BF16, WIDE_NS, WIDE_KS, False)])


@gpu
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_name)
def test_wide_qkv(native, dtype):
    _wide_test("qkv", "wide", [(dtype, (QKV_N,), WIDE_KS, False)])


@gpu
def test_wide_silu(native):
    _wide_test("silu", "wide", [(BF16, SILU_NS, WIDE_KS, False)])


def _run_midm(epi, dtype, bmt, launch_list, devs, fp8=False, strided_first=False):
    """``devs``: the calling test's cache of uploaded cases, shared by its row-block heights."""
    launches = 0
    for i, (m, n, k, s) in enumerate(launch_list):
        strided = strided_first and i == 0
        d = devs.get((n, k, strided))
        if d is None:
            d = devs[(n, k, strided)] = Dev(_case(epi, MIDM_ROWS, n, k, fp8), dtype, strided)
        assert ops.fused_kernel(m, True, fp8, epi) == "midm"
        d.prepare(m)
        ops.set_midm_plan(bmt, s)
        d.launch(m)
        d.check(m, f"midm {epi} {_name(dtype)} fp8={fp8} m={m} n={n} k={k} bmt={bmt} split={s} "
                   f"strided={strided}")
        launches += 1
    return launches


@gpu
@pytest.mark.parametrize("epi,dtype", [("plain", BF16), ("resadd", BF16), ("plain", FP16)],
                         ids=lambda v: v if isinstance(v, str) else _name(v))
def test_midm_plain_and_residual(native, epi, dtype):
    launches, devs = 0, {}
    for bmt in ops.MIDM_BUILT:
        launches += _run_midm(epi, dtype, bmt, midm_launches(bmt), devs, strided_first=True)
    assert _counters_zero()
    print(f"GEMM-EXACT midm {epi} {_name(dtype)} cases={len(devs)} launches={launches}")


def midm_norm_launches(bmt, n):
    return midm_launches(bmt, (n,), [(k, 1) for k, s in midm_ks(bmt) if s == 1])


@gpu
@pytest.mark.parametrize("epi", ["qkv", "silu"])
def test_midm_norm_epilogues(native, epi):
    launches, devs = 0, {}
    for bmt in ops.MIDM_BUILT:
        if bmt > 8:      # midm.h norm_fits: the norm-folded builds stop at 128-row blocks
            continue
        for n in ((QKV_N,) if epi == "qkv" else SILU_NS):
            launches += _run_midm(epi, BF16, bmt, midm_norm_launches(bmt, n), devs,
                                  strided_first=True)
    print(f"GEMM-EXACT midm {epi} cases={len(devs)} launches={launches}")


@gpu
@pytest.mark.parametrize("epi", ["plain", "resadd", "qkv", "silu"])
def test_fp8_weights(native, epi):
    n = QKV_N if epi == "qkv" else 368
    wide = _run_wide(epi, BF16, (n,), FP8_WIDE_KS, fp8_wide_ms(), FP8_WIDE_WAVES, fp8=True)
    midm, devs = 0, {}
    for bmt in FP8_MIDM:
        norm = epi in ("qkv", "silu")
        if norm and bmt > 8:
            continue
        ks = [p for p in FP8_MIDM_KS if p[1] == 1 or not norm]
        midm += _run_midm(epi, BF16, bmt, midm_launches(bmt, (n,), ks), devs, fp8=True)
    assert _counters_zero()
    assert wide > 0 and midm > 0
    print(f"GEMM-EXACT wide+midm fp8 {epi} cases={len(FP8_WIDE_KS) + len(FP8_MIDM_KS)} "
          f"launches={wide + midm} (wide {wide}, midm {midm})")


# ---- bf16 prefill GEMM -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prefill_silu_case(k):
    """w = [gate / 16; up] of [256, k] (its x carries the norm-fold row magnitudes, which the
    prefill GEMM has no use for: the test takes the plain case's x)."""
    return gemm_exact_case("silu", 1, 256, k)


@functools.lru_cache(maxsize=None)
def _prefill_silu_expected(k):
    """The prefill kernel keeps gate and up in fp32 (prefill_gemm.hip: bf16(silu(acc_gate) *
    acc_up)): one rounding of silu64(g) * u; ``near``: within ROW_DELTA of a tie."""
    y = (_case("plain", 300, 256, k).x @ _prefill_silu_case(k).w.t()).double()
    g, u = y[:, :128], y[:, 128:]
    out, near = round_fmt(g / (1.0 + torch.exp(-g)) * u, BF16, delta=ROW_DELTA)
    return out.to(BF16), near


@gpu
def test_prefill_gemm_bf16_exact_integer(native):
    """Plain and residual by bit equality under every schedule and tile height (stream-K and
    split-K partials are exact integers); SiLU against one rounding of the fp64 value, one
    step allowed only within ROW_DELTA of a tie."""
    i16 = torch.int16
    launches = 0
    ops.prefill_gemm_error_reset()
    for k in PREFILL_KS:
        cp, cr = _case("plain", 300, 256, k), _case("resadd", 300, 256, k)
        cs = _prefill_silu_case(k)
        assert torch.equal(cp.x, cr.x)
        x = cp.x.to(BF16).cuda()
        wp, wr, wsl = (c.w.to(BF16).cuda() for c in (cp, cr, cs))
        ep = gemm_exact_expected(cp, BF16)["y"].cuda()
        er = gemm_exact_expected(cr, BF16)["y"].cuda()
        es, near = _prefill_silu_expected(k)
        esd, res = es.cuda(), cr.res.to(BF16).cuda()
        for m in PREFILL_MS:
            for sched, bm in PREFILL_PLANS:
                what = f"prefill m={m} k={k} {sched} bm={bm}"
                got = ops.prefill_gemm(x[:m], wp, schedule=sched, bm=bm)
                if not torch.equal(got.view(i16), ep[:m].view(i16)):
                    _report(got.cpu(), ep[:m].cpu(), None, 0, what + " plain")
                r = res[:m].clone()
                ops.prefill_gemm(x[:m], wr, ops.GEMM_RESADD, residual=r, schedule=sched, bm=bm)
                if not torch.equal(r.view(i16), er[:m].view(i16)):
                    _report(r.cpu(), er[:m].cpu(), None, 0, what + " residual")
                got = ops.prefill_gemm(x[:m], wsl, ops.GEMM_SILU, schedule=sched, bm=bm)
                if not torch.equal(got.view(i16), esd[:m].view(i16)):
                    _report(got.cpu(), es[:m], near[:m], 1, what + " silu")
                launches += 3
    torch.cuda.synchronize()
    assert ops.prefill_gemm_error() == 0
    print(f"GEMM-EXACT prefill plain+residual+silu cases={3 * len(PREFILL_KS)} launches={launches}")
