"""Multi-query decode attention (ops.attention_decode_mq, the verify step of speculative
decoding) against the closed-form answers of tests/helpers.py: the key census and the needle,
with 1 .. 16 // G query tokens per sequence in one launch.

Token j of a sequence's qlen rows sees the keys < kvlen - (qlen - 1 - j), so every row of a
census case counts a different number of keys and every needle row has its own diagonal: a
causal bound off by one, a column served from the wrong row or a partition that publishes a
weight for a column that saw no key all move some element by at least 4x the tolerance.
"""
import functools
import math

import pytest
import torch

from agentic_traffic_testing_amd import ops
from helpers import (ATT_HKV, ATT_SCALE, NEEDLE_ATOL, NEEDLE_OFF_MASS, assert_exact, census_case,
                     census_max_keys, decode_kvlens, needle_case, needle_off_mass)

DT = [torch.bfloat16, torch.float16]
# (part_tokens, block size, G)
MQ_CFG = [(64, 16, 4), (128, 16, 3), (64, 32, 8), (128, 16, 1), (256, 16, 2)]
NEEDLE_KINDS = {"first", "diag", "tile16", "edge_last", "edge_first", "random"}
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert ops.native_available(), ops._load_error


def _name(dtype):
    return str(dtype).split(".")[-1]


def _cfg_id(c):
    return f"pt{c[0]}-bs{c[1]}-g{c[2]}"


def mq_seqs(pt: int, g: int):
    """(kvlen, qlen) of the base launch: kv == qlen, one key, partition edges (pt + 1: the
    second partition is empty for all tokens but the last; pt + qmax - 1: empty for the first
    token only), tile and page edges; qlen cycles qmax, 1, qmax // 2, clipped to the keys."""
    qmax = 16 // g
    kvs = [qmax, 1, pt - 1, pt, pt + 1, pt + qmax - 1, 2 * pt + 1, 3 * pt + 17, 49, 15, 17]
    cyc = [qmax, 1, max(1, qmax // 2)]
    return [(kv, min(cyc[i % 3], kv)) for i, kv in enumerate(kvs)]


def combine_seqs(pt: int, g: int, max_keys: int):
    """The lengths of the one-token decode tests (every kvlen up to a partition and a tile
    more, partition edges, a many-partition sequence, one kvlen = 0 dummy) with qlen = qmax."""
    qmax = 16 // g
    kvlens, _ = decode_kvlens(pt, g, max_keys)
    return [(kv, min(qmax, max(kv, 1))) for kv in kvlens]


@functools.lru_cache(maxsize=3)
def _case(kind, pt, bs, g, max_keys):
    seqs = mq_seqs(pt, g)
    if max_keys:
        seqs = seqs + combine_seqs(pt, g, max_keys)
    if kind == "needle":
        return needle_case(seqs, bs, g, edges=(pt, 64), seed=pt + g)
    return census_case(seqs, bs, g, kind, seed=pt + g)


def _cases(pt, bs, g, max_keys=0):
    for kind in ("A", "B"):
        yield "census" + kind, _case(kind, pt, bs, g, max_keys), 0.0
    yield "needle", _case("needle", pt, bs, g, max_keys and 65536), NEEDLE_ATOL


def _parts(case, pt):
    return max(1, math.ceil(max(kv for kv, _ in case.seqs) / pt))


# =========================================================================================
# CPU tier
# =========================================================================================
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("cfg", MQ_CFG, ids=_cfg_id)
def test_reference_reproduces_closed_forms_mq(cfg, dtype):
    """The CPU path of the new op gives the closed forms within the kernels' tolerances, the
    needle rows leave at most 2^-20 of their mass off target and ask for every kind of key."""
    pt, bs, g = cfg
    qmax = 16 // g
    assert ops.mq_max_qlen(g) == qmax
    seqs = mq_seqs(pt, g)
    assert {ql for _, ql in seqs} >= {qmax, 1} and (qmax, qmax) in seqs
    for label, case, atol in _cases(pt, bs, g):
        q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cpu")
        out = torch.full_like(q, 7.0)
        ops.attention_decode_mq(q, k, v, bt.clamp(min=0), kvlen, qstart, ATT_SCALE, None, None,
                                None, _parts(case, pt), pt, out=out)
        assert_exact(out, case.expected, dtype, atol, f"reference mq {label} {_cfg_id(cfg)}")
        if label == "needle":
            off = needle_off_mass(case)
            print(f"needle off-mass {off:.3e}")
            assert off <= NEEDLE_OFF_MASS
            assert case.kinds == NEEDLE_KINDS


def test_mq_host_validation():
    """G * qlen > 16, a partition size without a kernel, a bad partition count and an
    unsupported GQA group raise on the host, with or without the caller's max_qlen."""
    case = census_case([(40, 4), (9, 1)], 16, 4, "A")
    q, k, v, bt, kvlen, qstart = case.tensors(torch.bfloat16, "cpu")
    args = (q, k, v, bt, kvlen, qstart, ATT_SCALE, None, None, None)
    ops.attention_decode_mq(*args, 1, 64)
    ops.attention_decode_mq(*args, 1, 64, max_qlen=4)
    with pytest.raises(ValueError):
        ops.attention_decode_mq(*args, 1, 512)
    with pytest.raises(ValueError):
        ops.attention_decode_mq(*args, 1, 100)
    with pytest.raises(ValueError):
        ops.attention_decode_mq(*args, 65, 64)
    with pytest.raises(ValueError):
        ops.attention_decode_mq(*args, 1, 64, max_qlen=5)
    case8 = census_case([(40, 3)], 16, 8, "A")   # 3 tokens x 8 heads = 24 columns
    q, k, v, bt, kvlen, qstart = case8.tensors(torch.bfloat16, "cpu")
    with pytest.raises(ValueError):
        ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, None, None, None, 1, 64)
    with pytest.raises(ValueError):  # G = 16
        ops.attention_decode_mq(q, k[:, :1], v[:, :1], bt, kvlen, qstart, ATT_SCALE, None, None,
                                None, 1, 64)


def test_mq_debug_checks(monkeypatch):
    """ATTA_DEBUG_CHECKS covers the new op: a page id outside the cache, and a seq_qstart that
    holds a longer qlen than the caller declared."""
    monkeypatch.setattr(ops, "DEBUG_CHECKS", True)
    case = census_case([(40, 4), (9, 1)], 16, 4, "A")
    q, k, v, bt, kvlen, qstart = case.tensors(torch.bfloat16, "cpu")
    ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, None, None, None, 1, 64,
                            max_qlen=4)
    with pytest.raises(ops.PagedArgsError):
        ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, None, None, None, 1, 64,
                                max_qlen=2)
    with pytest.raises(ops.PagedArgsError):
        ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, None, None, None, 1, 64,
                                max_qlen=4, min_qlen=2)
    bad = bt.clone()
    bad[0, 1] = k.shape[0]
    with pytest.raises(ops.PagedArgsError):
        ops.attention_decode_mq(q, k, v, bad, kvlen, qstart, ATT_SCALE, None, None, None, 1, 64)


# =========================================================================================
# GPU tier
# =========================================================================================
def _workspace(S, parts):
    po = torch.full((S * ATT_HKV * parts * 16 * 128,), float("nan"), device="cuda")
    pl = torch.full((S * ATT_HKV * parts * 16,), float("nan"), device="cuda")
    cnt = torch.zeros(S * ATT_HKV, dtype=torch.int32, device="cuda")
    return po, pl, cnt


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("cfg", MQ_CFG, ids=_cfg_id)
def test_decode_mq_exact(native, cfg, dtype):
    """One launch of mixed qlen: the base cases (kv == qlen, a partition that is empty for the
    early tokens only, tile and page edges) and, with qlen = qmax, every length of the one-token
    decode tests up to the many-partition combine and a kvlen = 0 dummy.  NaN workspaces, run
    twice, counters back at zero, dummy rows untouched."""
    pt, bs, g = cfg
    cap = census_max_keys(dtype)
    if decode_kvlens(pt, g, cap) == decode_kvlens(pt, g):
        cap = 65536  # nothing cut: both types share the built case
    for label, case, atol in _cases(pt, bs, g, cap):
        assert len({ql for _, ql in case.seqs}) > 1 and any(kv == 0 for kv, _ in case.seqs)
        q, k, v, bt, kvlen, qstart = case.tensors(dtype, "cuda")
        live = case.live_rows.cuda()
        exp = case.expected[case.live_rows]
        parts = _parts(case, pt)
        po, pl, cnt = _workspace(len(case.seqs), parts)
        for _ in range(2):
            out = torch.full_like(q, 7.0)
            ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, parts, pt,
                                    out=out, max_qlen=16 // g)
            assert_exact(out[live], exp, dtype, atol, f"decode_mq {_cfg_id(cfg)} {label}")
            assert bool((out[~live] == 7.0).all()), "a dummy sequence's rows were written"
            assert bool((cnt == 0).all())


@gpu
@pytest.mark.parametrize("dtype", DT, ids=_name)
@pytest.mark.parametrize("cfg", MQ_CFG, ids=_cfg_id)
def test_decode_mq_one_token_is_decode_v2(native, cfg, dtype):
    """With qlen = 1 everywhere the output is bit-identical to attention_decode_v2, through
    the single-partition path and the last arriver's combine alike: the op runs one-token
    sequences on the one-token kernel (the multi-query kernel's own one-token columns differed
    from it in 3 of 94208 elements by one fp16 ulp in one of these ten cases: the compiler
    contracts the combine's folds into other FMA forms there)."""
    pt, bs, g = cfg
    kvlens, parts = decode_kvlens(pt, g)
    seqs = [(kv, 1) for kv in kvlens]
    gen = torch.Generator().manual_seed(pt + g)
    nblk = [max(1, math.ceil(kv / bs)) for kv in kvlens]
    nb = sum(nblk) + 4
    perm = torch.randperm(nb, generator=gen).to(torch.int32)
    bt = torch.zeros(len(seqs), max(nblk), dtype=torch.int32)
    o = 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[o:o + n]
        o += n
    k = torch.randn(nb, ATT_HKV, bs, 128, generator=gen).to(dtype).cuda()
    v = torch.randn(nb, ATT_HKV, 128, bs, generator=gen).to(dtype).cuda()
    q = torch.randn(len(seqs), ATT_HKV * g, 128, generator=gen).to(dtype).cuda()
    kvlen = torch.tensor(kvlens, dtype=torch.int32).cuda()
    qstart = torch.arange(len(seqs) + 1, dtype=torch.int32).cuda()
    bt = bt.cuda()
    po, pl, cnt = _workspace(len(seqs), parts)
    ref = torch.full_like(q, 7.0)
    ops.attention_decode_v2(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, parts, pt, out=ref)
    po.fill_(float("nan"))
    pl.fill_(float("nan"))
    got = torch.full_like(q, 7.0)
    ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, parts, pt, out=got,
                            max_qlen=1)
    diff = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
    print(f"MQ-vs-v2 {_cfg_id(cfg)} {_name(dtype)}: {diff} of {got.numel()} elements differ")
    assert diff == 0
    assert bool((cnt == 0).all())


@gpu
def test_decode_mq_refuses_out_of_range(native):
    """Nothing is launched for G * qlen > 16 or the 512-token partition shape."""
    case = census_case([(40, 3)], 16, 8, "A")
    q, k, v, bt, kvlen, qstart = case.tensors(torch.bfloat16, "cuda")
    po, pl, cnt = _workspace(1, 1)
    out = torch.full_like(q, 7.0)
    with pytest.raises(ValueError):
        ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, 1, 64, out=out)
    with pytest.raises(ValueError):
        ops.attention_decode_mq(q, k, v, bt, kvlen, qstart, ATT_SCALE, po, pl, cnt, 1, 512,
                                out=out, max_qlen=2)
    assert bool((out == 7.0).all())
