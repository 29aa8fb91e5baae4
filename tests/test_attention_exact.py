"""Paged-attention kernels against answers known in closed form (tests/helpers.py).

The random-data attention tests of test_kernels_gpu.py allow 1.5e-2 absolute, which at 2k keys
and more is most of the signal: a dropped key, a dropped tile or a mis-weighted merge passes.
Here every output element is known exactly - a key census (uniform weights over one-hot V:
integer counts over an integer) and a needle (one dominant key: the output is that key's V
row) - so one wrong key moves some element by at least 4x the tolerance at any length:
relative 2^-8 (bf16) / 2^-11 (fp16), absolute 0 (census) / 2^-16 (needle).

The unmarked tests check the builders themselves on the CPU: the project's reference
reproduces the closed forms, the sensitivity conditions hold for every length and seed the
GPU tests use, and a deliberately wrong dense reference fails the comparator.
"""
import functools
import math
import os

import pytest
import torch

from agentic_traffic_testing_amd import ops
from helpers import (ATT_GROUPS, ATT_HKV, ATT_SCALE, NEEDLE_ATOL, NEEDLE_OFF_MASS, PREFILL_SEQS,
                     SPLIT_SEQS, assert_exact, attn_rtol, census_case, census_drop_margin,
                     census_max_keys, decode_kvlens, decode_merge_trip, dense_attention64,
                     exact_errors, needle_case, needle_off_mass, prefill_tiles)

DT = [torch.bfloat16, torch.float16]
PART_TOKENS = [64, 128, 256, 512]
BLOCK_SIZES = [16, 32, 64]
# (part_tokens, block size, G): every G at block size 16, blocks of 32 and 64 keys for G = 4
DECODE_CFG = ([(pt, 16, g) for pt in PART_TOKENS for g in ATT_GROUPS] +
              [(pt, bs, 4) for pt in PART_TOKENS for bs in (32, 64)])
PREFILL_IMPLS = ["flash4", "flash8", "v1"]
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), ops._load_error


def _name(dtype):
    return str(dtype).split(".")[-1]


# ---- the cases the GPU tests run (shared with the CPU-tier checks) -------------------------
@functools.lru_cache(maxsize=3)
def _decode_case(kind, pt, bs, g, max_keys):
    kvlens, parts = decode_kvlens(pt, g, max_keys)
    seqs = [(kv, 1) for kv in kvlens]
    if kind == "needle":
        return needle_case(seqs, bs, g, edges=(pt, 64), seed=pt + g), parts
    return census_case(seqs, bs, g, kind, seed=pt + g), parts


def _decode_cases(pt, bs, g, dtype):
    """(label, case, partitions, absolute tolerance) of the three constructions."""
    cap = census_max_keys(dtype)
    if decode_kvlens(pt, g, cap) == decode_kvlens(pt, g):
        cap = 65536  # nothing cut: both types share the built case
    for kind in ("A", "B"):
        case, parts = _decode_case(kind, pt, bs, g, cap)
        yield "census" + kind, case, parts, 0.0
    case, parts = _decode_case("needle", pt, bs, g, 65536)
    yield "needle", case, parts, NEEDLE_ATOL


@functools.lru_cache(maxsize=4)
def _prefill_case(kind, which, bs, g):
    seqs = PREFILL_SEQS if which == "prefill" else SPLIT_SEQS
    if kind == "needle":
        return needle_case(seqs, bs, g, edges=(64,), seed=bs + g)
    return census_case(seqs, bs, g, kind, seed=bs + g)


def _prefill_cases(which, bs, g):
    for kind in ("A", "B"):
        yield "census" + kind, _prefill_case(kind, which, bs, g), 0.0
    yield "needle", _prefill_case("needle", which, bs, g), NEEDLE_ATOL


# =========================================================================================
# CPU tier: the builders
# =========================================================================================
@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_reference_reproduces_closed_forms(dtype):
    """The project's fp32 reference, through the CPU path of ops.attention_prefill and
    ops.attention_decode_v2, gives the closed-form answers of both constructions within the
    tolerances the kernels are held to."""
    for bs, g in ((16, 2), (64, 3)):
        for label, case, atol in _prefill_cases("prefill", bs, g):
            q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cpu")
            ts, to = prefill_tiles(case.seqs, 16)
            got = ops.attention_prefill(q, k, v, bt.clamp(min=0), kvlen, qstart, ts, to, ATT_SCALE)
            assert_exact(got, case.expected, dtype, atol, f"reference prefill {label} G={g}")
    for pt, bs, g in ((64, 16, 2), (128, 32, 4)):
        for label, case, parts, atol in _decode_cases(pt, bs, g, dtype):
            q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cpu")
            out = torch.full_like(q, 7.0)
            ops.attention_decode_v2(q, k, v, bt.clamp(min=0), kvlen, qstart, ATT_SCALE, None, None,
                                    None, parts, pt, out=out)
            assert_exact(out[case.live_rows], case.expected[case.live_rows], dtype, atol,
                         f"reference decode {label} G={g}")
            assert bool((out[~case.live_rows] == 7.0).all())


def _check_needle_case(case):
    """Off-target mass, distinct targets inside a GQA group, every kind of target asked for."""
    assert needle_off_mass(case) <= NEEDLE_OFF_MASS
    assert case.kinds == {"first", "diag", "tile16", "edge_last", "edge_first", "random"}
    g = case.g
    for i, (kv, ql) in enumerate(case.seqs):
        r0, r1 = case.rows(i)
        if kv == 0:
            continue
        tg = case.targets[r0:r1]
        pos = torch.arange(kv - ql, kv)[:, None]
        assert bool(((tg >= 0) & (tg <= pos)).all()), "a target must be visible"
        for hk in range(ATT_HKV):
            grp = tg[:, hk * g:(hk + 1) * g].sort(dim=1).values
            distinct = (grp[:, 1:] != grp[:, :-1]).all(dim=1) if g > 1 else torch.ones(ql, dtype=bool)
            assert bool(distinct[pos[:, 0] + 1 >= g].all()), "heads of a group share a target"


def _check_census_lengths(lengths, dtype):
    """Deleting any visible key moves some element (of code A's or code B's answer) by at least
    4x the tolerance, for every number of visible keys in ``lengths``."""
    need = 4 * attn_rtol(dtype)
    for n in sorted(set(lengths)):
        if n < 1:
            continue
        margin = max(census_drop_margin(n, "A"), census_drop_margin(n, "B"))
        assert margin >= need, f"{n} keys: one key moves the census by {margin:.3g} < {need:.3g}"


@pytest.mark.parametrize("pt", PART_TOKENS)
def test_decode_conditions(pt):
    """Every decode shape of the GPU tests: the grid holds the longest sequence in at most 64
    partitions, the long sequence sends the merge loop on a second trip where 64 partitions
    allow one, the census is sensitive to every single key at every length, and every needle
    row leaves at most 2^-20 of its softmax mass off its target."""
    for cpt, bs, g in DECODE_CFG:
        if cpt != pt:
            continue
        for dtype in DT:
            kvlens, parts = decode_kvlens(pt, g, census_max_keys(dtype))
            assert parts <= 64 and max(kvlens) <= parts * pt and 0 in kvlens
            assert set(range(1, pt + 18)) <= set(kvlens)
            assert max(kvlens) <= census_max_keys(dtype)
            _check_census_lengths(kvlens, dtype)
        kvlens, parts = decode_kvlens(pt, g)
        trip = decode_merge_trip(pt, g)
        if trip < 64:
            assert parts == trip + 1 and math.ceil(max(kvlens) / pt) > trip
        case, _ = _decode_case("needle", pt, bs, g, 65536)
        _check_needle_case(case)
    assert decode_merge_trip(pt, 8) == 32 or pt == 64  # 8 GQA columns: 33 partitions do it
    # the V rows of a sequence are pairwise distinct (the longest one of this partition size)
    i = max(range(len(case.seqs)), key=lambda s: case.seqs[s][0])
    _, v = case.dense(i)
    v = v[:case.seqs[i][0]]
    for hk in range(ATT_HKV):
        assert len(torch.unique(v[:, hk], dim=0)) == v.shape[0]
    assert float(v.abs().max()) <= 2.0 and bool((v * 8 == (v * 8).round()).all())


def test_prefill_conditions():
    """The same conditions for every prefill and split-KV shape."""
    for which, seqs in (("prefill", PREFILL_SEQS), ("split", SPLIT_SEQS)):
        visible = [pos + 1 for kv, ql in seqs for pos in range(kv - ql, kv)]
        for dtype in DT:
            assert max(visible) <= census_max_keys(dtype)
            _check_census_lengths(visible, dtype)
        for g in ATT_GROUPS:
            for bs in BLOCK_SIZES if which == "prefill" else [16]:
                _check_needle_case(_prefill_case("needle", which, bs, g))


def _longest(dtype, kind):
    cap = census_max_keys(dtype) if kind == "census" else 65536
    return max(max(decode_kvlens(pt, g, cap)[0]) for pt, _, g in DECODE_CFG)


def _loose_close(got, exp):
    """The comparator of the random-data tests (test_kernels_gpu.close at 1.5e-2 / 2e-2)."""
    got, exp = got.double(), exp.double()
    return bool(((got - exp).abs() <= 1.5e-2 + 2e-2 * exp.abs()).all())


@pytest.mark.parametrize("dtype", DT, ids=_name)
def test_wrong_references_are_caught(dtype):
    """A dense fp64 attention rounded to the output type passes the sharp comparator on a short
    sequence and on the longest one the GPU tests use; with one visible key dropped, the causal
    limit moved by one either way, or two keys of a 16-key group swapped in V only, it fails -
    on both lengths.  The census sees every change to the set of keys (and is blind to a
    permutation of V, its weights being uniform); the needle sees V and the target's
    addressing (and is blind to a key that gains ~e^-50 of the mass).  At the longest length
    the 1.5e-2 tolerance of the random-data tests accepts the dropped key."""
    g, bs = 2, 16
    rtol = attn_rtol(dtype)

    def run(case, i, h, **wrong):
        kv = case.seqs[i][0]
        r0, _ = case.rows(i)
        k, v = case.dense(i)
        got = dense_attention64(case.q[r0:r0 + 1, h].double(), k[:, h // g], v[:, h // g],
                                torch.tensor([kv - 1]), ATT_SCALE, **wrong)
        return got.to(dtype), case.expected[r0:r0 + 1, h]

    for kind in ("census", "needle"):
        longest = _longest(dtype, kind)
        # the key past the end is the stale slot behind a sequence in its last page: where the
        # longest sequence fills its page, one key less stands in for the raised limit
        seqs = [(37, 1), (longest, 1), (longest - 1, 1)]
        cases = ([census_case(seqs, bs, g, "A"), census_case(seqs, bs, g, "B")]
                 if kind == "census" else [needle_case(seqs, bs, g, edges=(512, 64))])
        atol = 0.0 if kind == "census" else NEEDLE_ATOL
        for i, (kv, _) in enumerate(seqs[:2]):
            caught = {}
            for h in range(ATT_HKV * g):
                for case in cases:
                    got, exp = run(case, i, h)
                    assert_exact(got, exp, dtype, atol, f"dense fp64 {kind} {kv} keys")
                    t = int(case.targets[case.rows(i)[0], h]) if kind == "needle" else kv // 2
                    mate = t ^ 1 if (t ^ 1) < kv else t - 1  # same 16-key group, visible
                    variants = {"drop": dict(drop=t), "drop_last": dict(drop=kv - 1),
                                "shift_down": dict(shift=-1), "shift_up": dict(shift=1),
                                "swap_v": dict(swap=(t, mate))}
                    for name, wrong in variants.items():
                        at = i if name != "shift_up" or kv % bs else 2
                        got, exp = run(case, at, h, **wrong)
                        bad, _ = exact_errors(got, exp, rtol, atol)
                        caught[name] = caught.get(name, False) or bad > 0
                        if kind == "census" and name == "drop" and i == 1 and case is cases[0]:
                            assert _loose_close(got, exp), "the loose tolerance was expected to pass"
            if kind == "census":
                assert all(caught[n] for n in ("drop", "drop_last", "shift_down", "shift_up")), caught
                assert not caught["swap_v"]  # uniform weights: any permutation of V sums the same
            else:
                # the heads ask for the diagonal among others, so shift_down hides a target
                assert all(caught[n] for n in ("drop", "shift_down", "swap_v")), caught


# =========================================================================================
# GPU: decode
# =========================================================================================
def _cfg_id(c):
    return f"pt{c[0]}-bs{c[1]}-g{c[2]}"


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("cfg", DECODE_CFG, ids=_cfg_id)
def test_decode_exact(native, cfg, dtype):
    """One launch of one-token sequences - every kvlen up to a partition and a tile more,
    lengths around partition edges up to the grid's last partition, one long enough for a
    second trip of the merge loop, one kvlen = 0 dummy row - through the in-kernel-combine
    decode at this partition size (NaN workspaces, run twice, counters back to 0) and the
    two-kernel decode (the same partitions, and one partition over everything)."""
    pt, bs, g = cfg
    for label, case, parts, atol in _decode_cases(pt, bs, g, dtype):
        q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cuda")
        live = case.live_rows.cuda()
        exp = case.expected[case.live_rows]
        S = len(case.seqs)
        po = torch.full((S * ATT_HKV * parts * 16 * 128,), float("nan"), device="cuda")
        pl = torch.full((S * ATT_HKV * parts * 16,), float("nan"), device="cuda")
        cnt = torch.zeros(S * ATT_HKV, dtype=torch.int32, device="cuda")
        tag = f"G={g} bs={bs} pt={pt} {label}"
        for _ in range(2):
            out = torch.full_like(q, 7.0)
            ops.attention_decode_v2(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, parts, pt,
                                    out=out)
            assert_exact(out[live], exp, dtype, atol, f"decode_v2 {tag}")
            assert bool((out[~live] == 7.0).all()), "the dummy row was written"
            assert bool((cnt == 0).all())
        whole = 64 * math.ceil(max(kv for kv, _ in case.seqs) / 64)
        for nparts, ptok in ((parts, pt), (1, whole)):
            po.fill_(float("nan"))
            pl.fill_(float("nan"))
            out = torch.full_like(q, 7.0)
            ops.attention_decode(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, nparts, ptok,
                                 out=out)
            assert_exact(out[live], exp, dtype, atol, f"decode_2k parts={nparts} {tag}")
            # this path writes a kvlen = 0 row as zeros (test_attention_decode_padded_and_subset)
            assert bool((out[~live] == 0).all())


# =========================================================================================
# GPU: prefill
# =========================================================================================
def _set_impl(impl):
    """-> the impl name ops takes; "flash4" / "flash8" also set the flash wave count."""
    if impl.startswith("flash"):
        ops.set_flash_waves(int(impl[5:]))
        return "flash"
    return "v1"


def _restore_flash_waves():
    ops.set_flash_waves(int(os.environ.get("ATTA_FLASH_WAVES", "4")))


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("g", ATT_GROUPS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("impl", PREFILL_IMPLS)
def test_prefill_exact(native, impl, bs, g, dtype):
    """Full prompts of 1 .. 200 tokens and chunks of 1 .. 130 tokens after cached prefixes of
    1 .. 100 keys (tile, 64-key block and page edges on both axes), flash at 4 and 8 waves
    and the v1 kernel."""
    try:
        name = _set_impl(impl)
        tile = ops.prefill_tile_tokens(g, name)
        for label, case, atol in _prefill_cases("prefill", bs, g):
            q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cuda")
            ts, to = (t.cuda() for t in prefill_tiles(case.seqs, tile))
            got = ops.attention_prefill(q, k, v, bt, kvlen, qstart, ts, to, ATT_SCALE, impl=name)
            assert_exact(got, case.expected, dtype, atol, f"prefill_{impl} G={g} bs={bs} {label}")
    finally:
        _restore_flash_waves()


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("g", ATT_GROUPS)
@pytest.mark.parametrize("splits", [1, 2, 3, 8])
def test_flash_split_kv_exact(native, splits, g, dtype):
    """The split-KV merge at small size: with one 64-key block per split allowed, 17 new rows
    over 64 b + r keys run 1 .. 8 key ranges per tile, at 4 and 8 waves; the arrival counters
    are back at zero afterwards."""
    try:
        torch.ops.atta.set_flash_split_blocks(1)
        for nw in (4, 8):
            ops.set_flash_waves(nw)
            tile = ops.prefill_tile_tokens(g, "flash")
            for label, case, atol in _prefill_cases("split", 16, g):
                q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cuda")
                ts, to = (t.cuda() for t in prefill_tiles(case.seqs, tile))
                for _ in range(2):
                    got = ops.attention_prefill(q, k, v, bt, kvlen, qstart, ts, to, ATT_SCALE,
                                                impl="flash", kv_splits=splits)
                    assert_exact(got, case.expected, dtype, atol,
                                 f"flash{nw}_split{splits} G={g} {label}")
                c = ops._FLASH_COUNTERS.get(torch.cuda.current_device())
                assert c is None or int(c.abs().sum()) == 0
    finally:
        torch.ops.atta.set_flash_split_blocks(ops.FLASH_SPLIT_BLOCKS)
        _restore_flash_waves()


@gpu
def test_block_size_128(native):
    """Pages of 128 keys: the flash kernel stages 64-key blocks at a fixed offset inside a page
    and cannot address the odd blocks of a longer page, so its launcher refuses them; the
    per-lane lookups of the v1 prefill and of both decode kernels take them."""
    dtype, g, bs, pt = torch.bfloat16, 4, 128, 128
    for label, case, atol in _prefill_cases("prefill", bs, g):
        q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cuda")
        ts, to = (t.cuda() for t in prefill_tiles(case.seqs, ops.prefill_tile_tokens(g, "v1")))
        got = ops.attention_prefill(q, k, v, bt, kvlen, qstart, ts, to, ATT_SCALE, impl="v1")
        assert_exact(got, case.expected, dtype, atol, f"prefill_v1 G={g} bs={bs} {label}")
        ts, to = (t.cuda() for t in prefill_tiles(case.seqs, ops.prefill_tile_tokens(g, "flash")))
        with pytest.raises((ValueError, RuntimeError)):
            ops.attention_prefill(q, k, v, bt, kvlen, qstart, ts, to, ATT_SCALE, impl="flash")
    for label, case, parts, atol in _decode_cases(pt, bs, g, dtype):
        q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cuda")
        live = case.live_rows.cuda()
        S = len(case.seqs)
        po = torch.full((S * ATT_HKV * parts * 16 * 128,), float("nan"), device="cuda")
        pl = torch.full((S * ATT_HKV * parts * 16,), float("nan"), device="cuda")
        cnt = torch.zeros(S * ATT_HKV, dtype=torch.int32, device="cuda")
        out = torch.full_like(q, 7.0)
        ops.attention_decode_v2(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, parts, pt,
                                out=out)
        assert_exact(out[live], case.expected[case.live_rows], dtype, atol,
                     f"decode_v2 G={g} bs={bs} pt={pt} {label}")
        out = torch.full_like(q, 7.0)
        ops.attention_decode(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, parts, pt, out=out)
        assert_exact(out[live], case.expected[case.live_rows], dtype, atol,
                     f"decode_2k G={g} bs={bs} pt={pt} {label}")
