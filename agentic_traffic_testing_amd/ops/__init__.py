"""Op layer: CDNA4 HIP kernels (``torch.ops.atta``) with device-strict dispatch.

* GPU tensors always run the hand-written HIP kernels from ``_atta_kernels.so``.  If the
  library is missing or fails to load, GPU calls raise ``NativeKernelsUnavailable`` -
  there is no silent eager fallback on a GPU.
* CPU tensors run ``reference.py`` (the same math in fp32 PyTorch) so the whole engine can
  be exercised in the CPU test tier.
"""
from __future__ import annotations

import os
from pathlib import Path

import torch

from . import reference as ref

_LIB = Path(__file__).resolve().parent / "_atta_kernels.so"
_loaded = False
_load_error: str | None = None


class NativeKernelsUnavailable(RuntimeError):
    pass


def library_build_hash(path: Path = _LIB) -> str | None:
    """Source hash embedded in a built kernel library (ops/build.py), or None."""
    import ctypes

    try:
        fn = ctypes.CDLL(str(path)).atta_build_hash
    except (OSError, AttributeError):
        return None
    fn.restype = ctypes.c_char_p
    return fn().decode()


def _lib_embeds(digest: str) -> bool:
    try:
        return digest.encode() in _LIB.read_bytes()
    except OSError:
        return False


def load_native(build_if_missing: bool = True) -> bool:
    """Load the HIP kernel library.  With ``build_if_missing`` the library is (re)built
    in-tree when missing or when its sources changed (content-hash stamps); without it a
    library whose embedded source hash does not match the sources is refused."""
    global _loaded, _load_error
    if _loaded:
        return True
    try:
        from . import build

        want = build.kernel_source_hash()
        # a library that embeds the current source hash is used as is (checked on the file
        # bytes, without loading it): the object files and their stamps need not exist - a
        # gpurun snapshot ships the .so only, and N ranks importing at once must not rebuild
        if build_if_missing and not _lib_embeds(want):
            build.build_kernels()  # serialised across processes by a file lock
        got = library_build_hash()
        if got != want:
            raise RuntimeError(f"stale kernel library {_LIB}: built from sources {got}, "
                               f"tree has {want}")
        torch.ops.load_library(str(_LIB))
        _loaded = True
        _load_error = None
        torch.ops.atta.set_flash_waves(FLASH_WAVES)  # the host tiles follow this setting
        torch.ops.atta.set_splitk_half(SPLITK_HALF)
        torch.ops.atta.set_flash_split_blocks(FLASH_SPLIT_BLOCKS)
        if WIDE_MAX_M <= SKINNY_MAX_M:  # wide kernel off: no <= 32-row call may take it
            set_wide_min_rows(SKINNY_ROWS + 1, SKINNY_ROWS + 1)
    except Exception as e:  # pragma: no cover - depends on environment
        _load_error = f"{type(e).__name__}: {e}"
    return _loaded


def native_available() -> bool:
    return load_native(build_if_missing=os.environ.get("ATTA_NO_BUILD", "0") != "1")


def _native():
    if not native_available():
        raise NativeKernelsUnavailable(
            f"atta HIP kernels not loadable from {_LIB}: {_load_error}. "
            "Run `python -m agentic_traffic_testing_amd.ops.build`.")
    return torch.ops.atta


# ---------------------------------------------------------------------------------------
def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, out: torch.Tensor | None = None):
    if not x.is_cuda:
        r = ref.rms_norm(x, w, eps)
        if out is not None:
            out.copy_(r)
            return out
        return r
    out = torch.empty_like(x) if out is None else out
    _native().rms_norm(out, x, w, eps)
    return out


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                       out: torch.Tensor | None = None):
    """residual <- x + residual (in place); returns rmsnorm(residual) * w."""
    if not x.is_cuda:
        n, r = ref.fused_add_rms_norm(x, residual, w, eps)
        residual.copy_(r)
        if out is not None:
            out.copy_(n)
            return out
        return n
    out = torch.empty_like(x) if out is None else out
    _native().fused_add_rms_norm(out, residual, x, w, eps)
    return out


def silu_and_mul(x: torch.Tensor, out: torch.Tensor | None = None):
    if not x.is_cuda:
        r = ref.silu_and_mul(x)
        if out is not None:
            out.copy_(r)
            return out
        return r
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1] // 2, dtype=x.dtype, device=x.device)
    _native().silu_and_mul(out, x)
    return out


def embed(table: torch.Tensor, ids: torch.Tensor, prev: torch.Tensor | None = None,
          feed_prev: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """Token-embedding gather.  With the int32 device flag ``feed_prev[0]`` set, row r takes
    token ``prev[r]`` (the previous step's device samples) instead of ``ids[r]`` - how an
    async-decode look-ahead step gets inputs the host has not seen yet."""
    T = ids.shape[0]
    if not table.is_cuda:
        src = ids
        if prev is not None and feed_prev is not None and int(feed_prev[0]) != 0:
            src = prev[:T]
        r = torch.nn.functional.embedding(src.long().clamp(0, table.shape[0] - 1), table)
        if out is not None:
            out.copy_(r)
            return out
        return r
    if out is None:
        out = torch.empty(T, table.shape[1], dtype=table.dtype, device=table.device)
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    if prev is None or feed_prev is None:
        prev = feed_prev = None
    _native().embed(out, table, ids.contiguous(), prev, feed_prev)
    return out


# Bounds-checked debug mode: ATTA_DEBUG_CHECKS=1 validates every paged-KV
# launch's block-table / slot / length arguments against the cache before the kernel runs
# (the kernels themselves index unchecked: a bad page id there is an out-of-bounds HBM access
# that can fault the GPU).  Checks synchronise with the device, so they are skipped inside
# hipGraph capture; combine with HIP_LAUNCH_BLOCKING=1 to pin a fault to its launch.
DEBUG_CHECKS = os.environ.get("ATTA_DEBUG_CHECKS", "0") == "1"


class PagedArgsError(ValueError):
    pass


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def check_paged_args(k_cache, block_tables, seq_kvlen, num_seqs: int = -1, what: str = ""):
    """Every block-table entry a sequence's kvlen reaches names a cache page, and the table
    row is long enough.  Raises PagedArgsError (debug mode only; no-op while capturing)."""
    if not DEBUG_CHECKS or _capturing(block_tables):
        return
    n = seq_kvlen.shape[0] if num_seqs < 0 else num_seqs
    nb, bs = k_cache.shape[0], k_cache.shape[2]
    bt = block_tables[:n].long()
    kv = seq_kvlen[:n].long()
    need = (kv + bs - 1) // bs
    if n and int(need.max()) > bt.shape[1]:
        raise PagedArgsError(f"{what}: kvlen {int(kv.max())} needs {int(need.max())} pages, "
                             f"block table has {bt.shape[1]} columns")
    used = torch.arange(bt.shape[1], device=bt.device)[None, :] < need[:, None]
    bad = used & ((bt < 0) | (bt >= nb))
    if bool(bad.any()):
        s, c = (int(i) for i in bad.nonzero()[0])
        raise PagedArgsError(f"{what}: sequence {s} page slot {c} = {int(bt[s, c])} outside "
                             f"the cache's {nb} pages")


def check_slots(k_cache, slots, what: str = ""):
    """KV-write slots are -1 (skip) or inside the cache.  Debug mode only."""
    if not DEBUG_CHECKS or _capturing(slots) or slots.numel() == 0:
        return
    cap = k_cache.shape[0] * k_cache.shape[2]
    sl = slots.long()
    if bool(((sl < -1) | (sl >= cap)).any()):
        raise PagedArgsError(f"{what}: slot ids outside [-1, {cap}): "
                             f"min {int(sl.min())}, max {int(sl.max())}")


def rope_cache(qkv, positions, slot_mapping, cos_sin, k_cache, v_cache, n_q_heads, n_kv_heads,
               head_dim, q_out: torch.Tensor | None = None):
    """Rotate q/k, write k/v to the paged cache; returns q [T, Hq, D]."""
    check_slots(k_cache, slot_mapping, "rope_cache")
    if not qkv.is_cuda:
        q = ref.rope_cache(qkv, positions, slot_mapping, cos_sin, k_cache, v_cache, n_q_heads,
                           n_kv_heads, head_dim)
        if q_out is not None:
            q_out.copy_(q)
            return q_out
        return q
    if q_out is None:
        q_out = torch.empty(qkv.shape[0], n_q_heads, head_dim, dtype=qkv.dtype, device=qkv.device)
    _native().rope_cache(q_out, k_cache, v_cache, qkv, positions, slot_mapping, cos_sin,
                         n_q_heads, n_kv_heads, head_dim)
    return q_out


# Prefill attention kernel: "flash" = LDS-staged 32x32x16-MFMA flash kernel
# (flash_prefill.hip, tiles of 128 / G tokens); "v1" = the round-1 per-wave kernel
# (attention.hip, tiles of 64 / G ... 8 tokens; kept for A/B runs).
PREFILL_IMPL = os.environ.get("ATTA_PREFILL_IMPL", "flash")
# the flash kernel stages a sequence's whole block-table row in LDS (kBtLds entries: 32k
# tokens at block size 16); wider tables take the v1 kernel
FLASH_MAX_BT = 2048
# ... and 64-key blocks at a fixed offset inside a page: pages of at most 64 keys
FLASH_MAX_BLOCK_SIZE = 64
# waves per flash-prefill workgroup (ops/csrc/flash_prefill.hip NW)
FLASH_WAVES = int(os.environ.get("ATTA_FLASH_WAVES", "4"))
if FLASH_WAVES not in (4, 8):  # the host tiles must match what the kernel covers
    raise ValueError(f"ATTA_FLASH_WAVES={FLASH_WAVES}: flash prefill runs 4 or 8 waves")


def prefill_impl(bt_width: int = 0, impl: str | None = None) -> str:
    """The prefill attention kernel for block tables of ``bt_width`` entries: the configured
    default falls back to v1 past FLASH_MAX_BT; an explicit "flash" there is an error (the
    caller's tiles would not match the kernel that runs)."""
    if impl == "flash" and bt_width > FLASH_MAX_BT:
        raise ValueError(f"flash prefill stages at most {FLASH_MAX_BT} block-table entries "
                         f"per sequence (got {bt_width}); use impl=None or 'v1'")
    impl = impl or PREFILL_IMPL
    return "v1" if impl == "flash" and bt_width > FLASH_MAX_BT else impl


def prefill_tile_tokens(g: int, impl: str | None = None, bt_width: int = 0) -> int:
    """Query tokens per prefill attention workgroup for GQA group ``g``."""
    impl = prefill_impl(bt_width, impl)
    # FLASH_WAVES x (32 // g) tokens (flash: 32 columns per wave) or 4 x (16 // g) (v1: 16) -
    # the G heads of a token share a wave; G = 3 (Llama-3.2-3B) leaves 2 resp. 1 columns idle
    if (impl or PREFILL_IMPL) == "flash":
        return FLASH_WAVES * (32 // g)
    return 4 * (16 // g)


def set_flash_waves(nw: int) -> None:
    """Waves per flash-prefill workgroup (4, or 8: each staged K/V block serves 256 columns).
    Engines build their prefill tiles from prefill_tile_tokens at start: set this before."""
    global FLASH_WAVES
    if nw not in (4, 8):
        raise ValueError("flash prefill runs 4 or 8 waves per workgroup")
    FLASH_WAVES = nw
    if native_available():
        _native().set_flash_waves(nw)


def attention_prefill(q, k_cache, v_cache, block_tables, seq_kvlen, seq_qstart, tile_seq,
                      tile_qoff, scale, out=None, impl: str | None = None,
                      kv_splits: int | None = None):
    """Causal varlen prefill attention over the paged cache.  ``tile_seq`` / ``tile_qoff``
    must come from tiles of ``prefill_tile_tokens(G, impl)`` tokens.  ``kv_splits`` (flash
    only): workgroups per (tile, KV head) over disjoint key ranges; None = ``flash_kv_splits``."""
    check_paged_args(k_cache, block_tables, seq_kvlen, what="attention_prefill")
    if not q.is_cuda:
        return ref.paged_attention(q, k_cache, v_cache, block_tables, seq_kvlen, seq_qstart,
                                   scale, out=out)
    out = torch.empty_like(q) if out is None else out
    if prefill_impl(block_tables.shape[1], impl) != "flash":
        _native().attention_prefill(out, q, k_cache, v_cache, block_tables, seq_kvlen,
                                    seq_qstart, tile_seq, tile_qoff, q.shape[1],
                                    k_cache.shape[1], scale)
        return out
    if k_cache.shape[2] > FLASH_MAX_BLOCK_SIZE:
        raise ValueError(f"flash prefill takes KV block sizes 16 .. {FLASH_MAX_BLOCK_SIZE} "
                         f"(got {k_cache.shape[2]}); use impl='v1' (ATTA_PREFILL_IMPL=v1)")
    pairs = tile_seq.shape[0] * k_cache.shape[1]
    ns = flash_kv_splits(pairs) if kv_splits is None else int(kv_splits)
    part = counters = None
    if ns > 1:
        part = torch.empty(pairs * ns * flash_part_floats(), dtype=torch.float32,
                           device=q.device)
        counters = _flash_counters(q.device, pairs)
    _native().flash_prefill(out, q, k_cache, v_cache, block_tables, seq_kvlen, seq_qstart,
                            tile_seq, tile_qoff, q.shape[1], k_cache.shape[1], scale, ns, part,
                            counters)
    return out


# split-KV flash prefill: steps with few (tile, KV head) pairs over long cached prefixes (a short
# suffix on a multi-thousand-token context leaves most CUs idle while each workgroup walks every
# key block in turn) run up to FLASH_KV_SPLITS workgroups per pair over contiguous key ranges of
# >= 8 blocks (decided per tile on the device) merged by the last arriver.  At the fan-out
# bursts' ~600 keys it measured a wash (5 x 17 rows: 18.2 -> 16.5 us at 32 heads, 19.9 -> 21.2 at
# 64; planning 10.1 -> 11.4 us), so those stay unsplit.  Long prefixes: 17 new rows over 4113
# keys 91.3 -> 34.7 us, 33 over 8209 keys 188.6 -> 65.4 us at 4 splits
# (profiles/r6_flash_split_kv.txt).
# ATTA_FLASH_KV_SPLITS: 0 = auto, 1 = off, n = at most n
FLASH_KV_SPLITS = int(os.environ.get("ATTA_FLASH_KV_SPLITS", "0"))
# fewest 64-key blocks per split (ATTA_FLASH_SPLIT_BLOCKS; a tile splits nblocks // this ways)
FLASH_SPLIT_BLOCKS = int(os.environ.get("ATTA_FLASH_SPLIT_BLOCKS", "8"))
_FLASH_COUNTERS: dict = {}


def flash_part_floats() -> int:
    """fp32 words of one split's partial: per workgroup column (32 per wave) 128 O values and
    an (m, l) pair (ops/csrc/flash_prefill.hip part_bytes)."""
    return FLASH_WAVES * 32 * (128 + 2)


def flash_kv_splits(pairs: int) -> int:
    if FLASH_KV_SPLITS == 1 or pairs > 128:
        return 1
    cap = FLASH_KV_SPLITS if FLASH_KV_SPLITS > 1 else 8
    return max(1, min(cap, 8, 256 // max(pairs, 1)))


def _flash_counters(device, n: int) -> torch.Tensor:
    """Zeroed arrival counters of the split-KV merge (re-armed by the kernel's last arrivers)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    c = _FLASH_COUNTERS.get(idx)
    if c is None or c.numel() < n:
        c = torch.zeros(max(n, 4096), dtype=torch.int32, device=device)
        _FLASH_COUNTERS[idx] = c
    return c


def attention_decode(q, k_cache, v_cache, block_tables, seq_kvlen, seq_qstart, scale,
                     part_out, part_lse, num_parts, part_tokens, out=None, num_seqs: int = -1):
    """Decode attention for sequences [0, num_seqs) (one query token each)."""
    check_paged_args(k_cache, block_tables, seq_kvlen, num_seqs, "attention_decode")
    if not q.is_cuda:
        n = seq_kvlen.shape[0] if num_seqs < 0 else num_seqs
        return ref.paged_attention(q, k_cache, v_cache, block_tables[:n], seq_kvlen[:n],
                                   seq_qstart[:n + 1], scale, out=out)
    out = torch.empty_like(q) if out is None else out
    _native().attention_decode(out, part_out, part_lse, q, k_cache, v_cache, block_tables,
                               seq_kvlen, seq_qstart, num_seqs, num_parts, part_tokens, q.shape[1],
                               k_cache.shape[1], scale)
    return out


def sample_topkp(logits, temperature, top_p, top_k, seeds, steps, out=None):
    """top-k / top-p sampling, one workgroup per row (ops/csrc/sampling.hip): exact radix-select
    thresholds, the same seeded Gumbel draw as ``sample`` (rows with both filters off get the
    same token), device-side parameters - graph-capturable."""
    if not logits.is_cuda:
        r = ref.sample_topkp(logits, temperature, top_p, top_k, seeds, steps)
        if out is not None:
            out[:r.shape[0]].copy_(r)
            return out[:r.shape[0]]
        return r
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    _native().sample_topkp(out, logits, temperature, top_p, top_k, seeds, steps)
    return out[:logits.shape[0]]


def sample(logits, temperature, seeds, steps, out=None):
    if not logits.is_cuda:
        r = ref.sample(logits, temperature, seeds, steps)
        if out is not None:
            out.copy_(r)
            return out
        return r
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    _native().sample(out, logits, temperature, seeds, steps)
    return out



# skinny-GEMM (decode) dispatch: rows <= SKINNY_MAX_M use the MFMA weight-streaming kernel,
# larger M (prefill) goes to hipBLASLt through F.linear.
SKINNY_MAX_M = int(os.environ.get("ATTA_SKINNY_MAX_M", "32"))
# 33..WIDE_MAX_M rows over PRE-SHUFFLED 16-bit weights run the wide small-M kernel
# (csrc/wide.hip: x staged once per workgroup in LDS and shared by its tiles, split-K for the
# narrow projections), with the same fused epilogues - burst prefills and decode batches of
# up to 128 sequences.  0 (or anything <= SKINNY_MAX_M) turns it off.
WIDE_MAX_M = int(os.environ.get("ATTA_WIDE_MAX_M", "128"))
# 129..MIDM_MAX_M rows over pre-shuffled 16-bit weights run the mid-M kernel (csrc/midm.h:
# row-blocked BM x 128 tiles, ~256 workgroups, the same fused epilogues) - the uncached burst
# and planning prefills.  Needs the wide kernel on up to 128 rows; 0 turns it off.
MIDM_MAX_M = int(os.environ.get("ATTA_MIDM_MAX_M", "1024"))
# the three above are routing policy; these are the rows the kernels themselves take
# (csrc/skinny.h: kSkinnyMaxM, kWideMaxM, kMidmMaxM)
SKINNY_ROWS, WIDE_ROWS, MIDM_ROWS = 32, 128, 8192
# pre-shuffled 16-bit calls run the wide kernel from this many rows (gate_up + SiLU: the
# second); set_wide_min_rows keeps the pair in step with the library's
_wide_min_rows = [17, 12]


def _policy_tops() -> tuple[int, int, int]:
    """Most rows the policy limits let the 16-row-tile GEMV, the wide and the mid-M kernel
    take (0: kernel off).  The mid-M kernel needs the wide kernel on up to its 128 rows."""
    wide_top = min(WIDE_MAX_M, WIDE_ROWS) if WIDE_MAX_M > SKINNY_MAX_M else 0
    midm_top = min(MIDM_MAX_M, MIDM_ROWS) if wide_top == WIDE_ROWS else 0
    return min(SKINNY_MAX_M, SKINNY_ROWS), wide_top, (midm_top if midm_top > WIDE_ROWS else 0)


def fused_kernel(m: int, preshuffled: bool, fp8: bool = False, epi: str = "plain",
                 mxfp4: bool = False, wide_w4: bool = False) -> str | None:
    """Which hand-written weight-streaming kernel runs ``m`` rows over this weight layout with
    this epilogue ("plain" | "resadd" | "qkv" | "silu" | "sample" | "sample_lp" | "score" |
    "push"; "sample_lp", the sampler with the logprob record, and "score", the teacher-forced
    scorer, route as "sample" does but have no fp8 build): "skinny" (the
    16-row-tile GEMV), "wide", "midm", or None (no kernel: the native call would fail).  The
    routing table of csrc/gemv.hip ``route()`` (written out there and in docs/kernels.md)
    under the policy limits above.  ``mxfp4``: the 4-bit copies (``preshuffle_mxfp4``), which
    only the 16-row-tile GEMV streams - unless the caller chooses ``wide_w4``, the wide
    kernel's 4-bit builds for 33-128 rows (the same keyword on ``linear`` /
    ``decode_qkv_rope`` / ``decode_gate_up_silu``).  Pure: no native call, usable without a
    GPU."""
    skinny_top, wide_top, midm_top = _policy_tops()
    if m < 1 or (epi in ("sample_lp", "score") and fp8):
        return None
    if epi in ("sample_lp", "score"):
        epi = "sample"
    if mxfp4:
        if epi in ("sample", "push"):
            return None
        if m <= SKINNY_ROWS:
            return "skinny" if m <= skinny_top else None
        return "wide" if wide_w4 and m <= wide_top else None
    if not (preshuffled or fp8) or epi == "push" or not wide_top:
        return "skinny" if m <= skinny_top else None
    if m <= SKINNY_ROWS and (fp8 or m < _wide_min_rows[1 if epi == "silu" else 0]):
        return "skinny"
    if epi == "sample" and fp8:
        return None
    if m <= wide_top:
        return "wide"
    return "midm" if epi != "sample" and WIDE_ROWS < m <= midm_top else None


def fused_max_rows(preshuffled: bool = True, mxfp4: bool = False, wide_w4: bool = False) -> int:
    """Most rows a projection (any epilogue but the sampler's) may have to run on the
    hand-written weight-streaming kernels: row-major weights or the MXFP4 copies (the
    16-row-tile GEMV alone; with ``wide_w4`` the wide kernel's 4-bit builds too), or
    pre-shuffled 16-bit / fp8."""
    tops = _policy_tops()
    if mxfp4:
        return max(tops[:2]) if wide_w4 else tops[0]
    return max(tops) if preshuffled else tops[0]


SKINNY_WAVES = int(os.environ.get("ATTA_SKINNY_WAVES", "8"))
# per-projection wave counts from the MI355X sweep (profiles/r1_microbench_v3_plain.txt):
# 8 waves x 2-deep stages for the small qkv / o projections, 16 waves for the large ones.
WAVES_SMALL = int(os.environ.get("ATTA_WAVES_SMALL", "8"))
WAVES_LARGE = int(os.environ.get("ATTA_WAVES_LARGE", "16"))

# Workgroup waves per decode projection and weight format, from cold-cache sweeps on MI355X
# (profiles/r1_microbench_v5_cold_preshuffle.txt, r1_microbench_v6_fp8.txt, and the
# pre-shuffled unroll sweep): "rm" row-major 16-bit, "ps" pre-shuffled 16-bit, "fp8".
# "mxfp4": not swept - a wave owns whole 128-wide loads, so K 4096 is 32 loads (4 per wave at
# 8 waves) and the 8B down projection 112 (7 per wave at 16); the library halves the count
# when a slice has fewer loads than waves.
DECODE_WAVES = {
    "qkv": {"rm": 8, "ps": 4, "fp8": 8, "mxfp4": 8},
    "o": {"rm": 8, "ps": 8, "fp8": 8, "mxfp4": 8},
    "gate_up": {"rm": 16, "ps": 16, "fp8": 8, "mxfp4": 8},
    "down": {"rm": 16, "ps": 8, "fp8": 16, "mxfp4": 16},
    "lm_head": {"rm": 16, "ps": 16, "fp8": 16},
}
# tuning override: ATTA_DECODE_WAVES="qkv.ps=8,down.fp8=16"
for _item in filter(None, os.environ.get("ATTA_DECODE_WAVES", "").split(",")):
    _key, _, _val = _item.partition("=")
    _proj, _, _fmt = _key.strip().partition(".")
    DECODE_WAVES[_proj][_fmt] = int(_val)


# 17-32 rows (two MFMA row blocks: the fused small-prefill path) stream gate_up best with 8
# waves - half the per-workgroup cross-wave reduction per weight byte: 71.8 -> 59.2 us at 17
# rows, while 16 waves stay best at <= 16 rows (profiles/r4_skinny_mt_probe.txt)
DECODE_WAVES_MT2 = {"gate_up": 8}


def decode_waves(proj: str, preshuffled: bool = False, fp8: bool = False, m: int = 0,
                 mxfp4: bool = False) -> int:
    if mxfp4:
        return DECODE_WAVES[proj]["mxfp4"]
    if m > 16 and preshuffled and not fp8 and proj in DECODE_WAVES_MT2:
        return DECODE_WAVES_MT2[proj]
    return DECODE_WAVES[proj]["fp8" if fp8 else ("ps" if preshuffled else "rm")]


# Split-K factor per decode projection: gridDim.y slices of K per 16-column tile so grids
# that leave CUs idle (qkv: 384 tiles, o / down: 256 tiles on 256 CUs) stream from every CU;
# the tile's last slice combines the fp32 partials in slice order (ops/csrc/gemv.hip).
# 0 = auto (``auto_ksplit``).  The MI355X sweep (profiles/r2_microbench_splitk.txt) shows the
# in-launch combine costs ~1.5-2 us, so splitting only pays when the grid is far below the
# CU count: Llama-3.1-8B shapes (>= 256 tiles) all run fastest unsplit, the 70B TP=8 qkv
# shard (80 tiles, K 8192) runs 14.7 -> 8.7 us at split 2.
DECODE_KSPLIT = {"qkv": 0, "o": 0, "gate_up": 0, "down": 0}
for _item in filter(None, os.environ.get("ATTA_DECODE_KSPLIT", "").split(",")):
    _key, _, _val = _item.partition("=")
    DECODE_KSPLIT[_key.strip()] = int(_val)


def auto_ksplit(tiles: int, K: int) -> int:
    """Split so a small grid reaches >= ~160 workgroups, keeping >= 2048 of K per slice."""
    ks = 1
    while tiles * ks < 160 and K // (ks * 2) >= 2048:
        ks *= 2
    return ks

# wide-kernel split-K slabs in bf16 (ATTA_SPLITK_HALF=1): half the slab traffic of the
# qkv / o / down launches at 33-128 rows, each slice's partial rounded to bf16 once before the
# fp32 slice-ordered sum
SPLITK_HALF = int(os.environ.get("ATTA_SPLITK_HALF", "0"))


def set_splitk_half(on: bool) -> None:
    """bf16 (True) or fp32 (False) split-K slabs for the wide kernel's following launches."""
    global SPLITK_HALF
    SPLITK_HALF = int(bool(on))
    _native().set_splitk_half(SPLITK_HALF)


SPLITK_WS_FLOATS = 16 << 20  # 64 MiB: tiles x split x rows x 16 fp32 slots (mid-M splits)
SPLITK_COUNTERS = 8192
_SPLITK_WS: dict = {}


def ensure_splitk_workspace(device) -> None:
    """Allocate + register the split-K workspace of ``device`` once (before any capture:
    captured launches keep its address for the life of the graph)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _SPLITK_WS:
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("split-K workspace must be allocated before hipGraph capture")
    ws = torch.zeros(SPLITK_WS_FLOATS, dtype=torch.float32, device=f"cuda:{idx}")
    counters = torch.zeros(SPLITK_COUNTERS, dtype=torch.int32, device=f"cuda:{idx}")
    _native().set_splitk_workspace(ws, counters)
    _SPLITK_WS[idx] = (ws, counters)


def _ksplit(proj: str, x: torch.Tensor, ksplit: int | None, tiles: int) -> int:
    k = DECODE_KSPLIT.get(proj, 0) if ksplit is None else ksplit
    if k <= 0:
        k = auto_ksplit(tiles, x.shape[1])
    if k > 1:
        ensure_splitk_workspace(x.device)
    return k


def skinny_ok(x: torch.Tensor, w: torch.Tensor, preshuffled: bool = False,
              fp8: bool = False, mxfp4: bool = False, wide_w4: bool = False) -> bool:
    """Does ``x @ w.T`` run on the hand-written MFMA kernels?  Shapes they take, and a row
    count ``fused_kernel`` names a kernel for.  ``mxfp4``: ``w`` holds the packed codes
    [N, K / 2] of ``preshuffle_mxfp4``; ``wide_w4``: the caller chose the wide kernel's 4-bit
    builds for 33-128 rows."""
    m, k = x.shape
    if mxfp4 and (w.dtype != torch.uint8 or w.shape[1] * 2 != k):
        return False
    return (x.is_cuda and fused_kernel(m, preshuffled, fp8, mxfp4=mxfp4,
                                       wide_w4=wide_w4) is not None
            and w.shape[0] % 16 == 0 and k % 128 == 0 and x.stride(1) == 1
            and w.is_contiguous())


def set_wide_plan(waves: int = 0, ksplit: int = 0) -> None:
    """Override the (waves = 16-column tiles per workgroup, K split) plan of the NEXT wide
    small-M launch (tuning sweeps); 0 = the kernel library's own plan."""
    _native().set_wide_plan(int(waves), int(ksplit))


def set_midm_plan(bmt: int = 0, ksplit: int = 0) -> None:
    """Override the (row-block height 16 * bmt, K slices) plan of the NEXT mid-M launch
    (tuning sweeps, warm-up); 0 = the kernel library's own plan."""
    _native().set_midm_plan(int(bmt), int(ksplit))


def midm_plan(m: int, ntiles: int, k: int, epi: int) -> tuple[int, int]:
    """(bmt, K slices) the mid-M kernel plans for m rows x ntiles 16-column tiles x K (epi:
    0 plain, 1 residual add, 2 qkv + RoPE, 3 gate_up + SiLU)."""
    b, s = _native().midm_plan(int(m), int(ntiles), int(k), int(epi), SPLITK_WS_FLOATS)
    return int(b), int(s)


MIDM_BUILT = (3, 4, 5, 6, 8, 10, 12)  # row-block heights / 16 (csrc/midm_b<N>.hip)


def warm_wide_kernels(device, dtype=torch.bfloat16, wide_w4: bool = False,
                      expand: bool = True) -> None:
    """Launch one tiny GEMM from every translation unit of the wide (wide_mt<N>.hip: one per
    16-row block count the limits allow) and mid-M kernels (midm_b<N>.hip per row-block
    height, midm.hip's split-K reduce), so every code object is loaded at engine start: HIP
    loads a translation unit's code object at the first launch of one of its kernels, which
    otherwise lands inside a timed prefill (1.5-2.5 ms per object: burst TTFT 4.7 -> 6.3 / 7.3
    ms the first time a 50 / 95-row burst ran, scripts/gpu/probe_fanout_ttft.py).  Only
    kernels the configured limits can route to are launched, and the caller's wide row
    thresholds are restored afterwards.  ``wide_w4`` (the weights-only MXFP4 mode): the wide
    kernel's 4-bit translation units (wide_w4_mt<N>.hip) and - unless ``expand`` is off: with
    mxfp4_fp8_activations no step expands - the expand kernel as well."""
    dev = torch.device(device)
    top = fused_max_rows()
    if dev.type != "cuda" or top <= SKINNY_MAX_M:
        return
    ensure_splitk_workspace(dev)
    w = preshuffle(torch.zeros(128, 256, dtype=dtype, device=dev))
    prev = list(_wide_min_rows)
    set_wide_min_rows(1, 1)
    try:
        for rows in range(16, min(top, WIDE_ROWS) + 1, 16):
            linear(torch.zeros(rows, 256, dtype=dtype, device=dev), w, preshuffled=True)
        if top > WIDE_ROWS:
            x = torch.zeros(144, 256, dtype=dtype, device=dev)
            for b in MIDM_BUILT:
                set_midm_plan(b, 1)
                linear(x, w, preshuffled=True)
            set_midm_plan(6, 2)  # the split-K reduce launch (midm.hip)
            linear(x, w, preshuffled=True)
        if wide_w4:
            wq = torch.zeros(128, 128, dtype=torch.uint8, device=dev)
            sq = torch.full((128, 8), 127, dtype=torch.uint8, device=dev)
            for rows in range(SKINNY_ROWS + 16, fused_max_rows(mxfp4=True, wide_w4=True) + 1, 16):
                linear(torch.zeros(rows, 256, dtype=dtype, device=dev), wq, w_block_scale=sq,
                       wide_w4=True)
            if expand:
                expand_mxfp4(wq, sq, "plain", torch.empty(128, 256, dtype=dtype, device=dev))
    finally:
        set_wide_min_rows(*prev)
    torch.cuda.synchronize(dev)


def set_wide_min_rows(m: int = 17, m_silu: int = 12) -> None:
    """Pre-shuffled 16-bit GEMV calls of >= ``m`` rows (gate_up + SiLU: ``m_silu``) run the
    wide small-M kernel; calls over 32 rows always do.  Defaults = the measured crossover
    (profiles/r5_wide_vs_skinny.txt); 33 / 33 keeps <= 32 rows on the 16-row-tile GEMVs."""
    _native().set_wide_min_rows(int(m), int(m_silu))
    _wide_min_rows[:] = (max(1, int(m)), max(1, int(m_silu)))  # as the library clamps them


def preshuffle(w: torch.Tensor, rowmap: str = "plain") -> torch.Tensor:
    """Re-lay a [N, K] weight for the decode GEMV: rows permuted into the kernel's tile order
    (``rowmap`` "plain" | "qkv" (RoPE pairs d, d+64 of each 128-dim head in one tile) |
    "silu" (gate_j and up_j in one tile)), then every 16-row x 32-column block stored as the
    1 KiB the 64 MFMA lanes load (lane l: row l & 15, columns 8*(l >> 4)..+7).  Same shape
    and dtype as ``w``; only valid as the ``w`` of ops called with ``preshuffled=True``."""
    N, K = w.shape
    if N % 16 or K % 32:
        raise ValueError(f"preshuffle needs N % 16 == 0 and K % 32 == 0, got {tuple(w.shape)}")
    rows = _rowmap_index(N, rowmap, w.device)
    if rows is not None:
        w = w.index_select(0, rows)
    return (w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
            .reshape(N, K))


# ---- fp8 weight-only quantisation (OCP e4m3fn, per output row) ----------------------------
FP8_MAX = 448.0


def quantize_fp8(w: torch.Tensor, row_amax: torch.Tensor | None = None
                 ) -> tuple[torch.Tensor, torch.Tensor]:
    """[N, K] 16-bit weight -> (uint8 e4m3fn bytes [N, K], fp32 per-row scale [N]).

    ``row_amax`` overrides the per-row |max| the scale is derived from: a TP row-parallel
    shard (o / down, a K slice of every row) passes the FULL row's amax, so every rank
    quantises with the TP=1 scale and TP=N fp8 weights are bit-identical to TP=1's."""
    wf = w.float()
    amax = wf.abs().amax(dim=1) if row_amax is None else row_amax.float().to(wf.device)
    scale = (amax / FP8_MAX).clamp_min(1e-12)
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.contiguous()


def dequantize_fp8(q: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    return (q.view(torch.float8_e4m3fn).float() * scale[:, None].float()).to(dtype)


def preshuffle_fp8(q: torch.Tensor, rowmap: str = "plain") -> torch.Tensor:
    """fp8 analogue of ``preshuffle``: rows permuted by ``rowmap``, then each 16-row x 64-col
    block stored as 64 lanes x 16 bytes, lane l = (row l & 15) holding its 8 k-values of the
    two 32-wide K steps (k = 8*(l >> 4) + j and 32 + 8*(l >> 4) + j)."""
    N, K = q.shape
    if N % 16 or K % 64:
        raise ValueError(f"fp8 preshuffle needs N % 16 == 0 and K % 64 == 0, got {tuple(q.shape)}")
    rows = _rowmap_index(N, rowmap, q.device)
    if rows is not None:
        q = q.index_select(0, rows)
    return (q.reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous()
            .reshape(N, K))


# ---- MXFP4 weight-only quantisation (OCP Microscaling: e2m1 elements, e8m0 block scales) ----
MXFP4_BLOCK = ref.MXFP4_BLOCK
quantize_mxfp4 = ref.quantize_mxfp4
dequantize_mxfp4 = ref.dequantize_mxfp4


def preshuffle_mxfp4(codes: torch.Tensor, scales: torch.Tensor, rowmap: str = "plain"
                     ) -> tuple[torch.Tensor, torch.Tensor]:
    """MXFP4 analogue of ``preshuffle``: (codes uint8 [N, K], scales uint8 [N, K / 32]) ->
    (wq uint8 [N, K / 2], sq uint8 [N, K / 32]) as the 4-bit decode GEMV streams them.  Rows
    permuted by ``rowmap``; per 16-row tile and 128-wide K chunk c, lane l's 16 bytes are row
    l & 15 of the chunk's four 32-wide K steps: dword j holds k = 128 c + 32 j + 8 (l >> 4) + i,
    code i in bits 4i .. 4i + 3.  ``sq``: 64 B per tile and chunk, one dword per row, byte j =
    the scale of K step j.  ``unshuffle_mxfp4`` inverts it."""
    N, K = codes.shape
    if N % 16 or K % 128 or scales.shape != (N, K // MXFP4_BLOCK):
        raise ValueError(f"mxfp4 preshuffle needs N % 16 == 0, K % 128 == 0 and scales "
                         f"[N, K / 32], got {tuple(codes.shape)} / {tuple(scales.shape)}")
    rows = _rowmap_index(N, rowmap, codes.device)
    if rows is not None:
        codes, scales = codes.index_select(0, rows), scales.index_select(0, rows)
    # (tile, row, chunk, step j, lane group g, element i) -> (tile, chunk, g, row, j, i)
    c = codes.reshape(N // 16, 16, K // 128, 4, 4, 8).permute(0, 2, 4, 1, 3, 5)
    wq = (c[..., 0::2] | (c[..., 1::2] << 4)).contiguous().reshape(N, K // 2)
    sq = scales.reshape(N // 16, 16, K // 128, 4).permute(0, 2, 1, 3).contiguous()
    return wq, sq.reshape(N, K // MXFP4_BLOCK)


def unshuffle_mxfp4(wq: torch.Tensor, sq: torch.Tensor, rowmap: str = "plain"
                    ) -> tuple[torch.Tensor, torch.Tensor]:
    """Inverse of ``preshuffle_mxfp4``: (codes uint8 [N, K], scales uint8 [N, K / 32])."""
    N, K = wq.shape[0], wq.shape[1] * 2
    p = wq.reshape(N // 16, K // 128, 4, 16, 4, 4)
    c = torch.stack([p & 15, p >> 4], -1).reshape(N // 16, K // 128, 4, 16, 4, 8)
    codes = c.permute(0, 3, 1, 4, 2, 5).contiguous().reshape(N, K)
    scales = (sq.reshape(N // 16, K // 128, 16, 4).permute(0, 2, 1, 3).contiguous()
              .reshape(N, K // MXFP4_BLOCK))
    rows = _rowmap_index(N, rowmap, wq.device)
    if rows is not None:
        inv = torch.empty_like(rows)
        inv[rows] = torch.arange(N, device=rows.device)
        codes, scales = codes.index_select(0, inv), scales.index_select(0, inv)
    return codes, scales


ROWMAPS = {"plain": 0, "qkv": 1, "silu": 2}


def expand_mxfp4(wq: torch.Tensor, sq: torch.Tensor, rowmap: str, out: torch.Tensor
                 ) -> torch.Tensor:
    """``out`` [N, K] bf16 / fp16 (row-major) := the 16-bit values of one projection's 4-bit
    copy (``wq`` / ``sq`` of ``preshuffle_mxfp4`` with this ``rowmap``): bit for bit
    ``dequantize_mxfp4(*unshuffle_mxfp4(wq, sq, rowmap), out.dtype)`` wherever every value is
    a normal number of ``out.dtype`` (scale bytes 97..157 for bf16, 114..140 for fp16), with
    the convert the 4-bit GEMMs use.  One streaming HIP kernel, no allocation: the
    weights-only MXFP4 mode runs it into its scratch inside steps and graph captures."""
    if rowmap not in ROWMAPS:
        raise ValueError(f"unknown rowmap {rowmap}")
    if not (out.is_cuda and wq.is_cuda and sq.is_cuda):
        raise ValueError("expand_mxfp4 is a HIP kernel: GPU tensors only")
    _native().expand_mxfp4(out, wq, sq, ROWMAPS[rowmap])
    return out


def _rowmap_index(N: int, rowmap: str, dev):
    if rowmap == "plain":
        return None
    if rowmap == "qkv":
        if N % 128:
            raise ValueError("qkv rowmap needs whole 128-dim heads")
        t = torch.arange(N // 16, device=dev)
        c = torch.arange(16, device=dev)
        head, j = (t >> 3)[:, None], (t & 7)[:, None]
        return (head * 128 + j * 8 + (c & 7)[None, :] + ((c & 8) != 0)[None, :] * 64).reshape(-1)
    if rowmap == "silu":
        inter = N // 2
        if inter % 8:
            raise ValueError("silu rowmap needs inter % 8 == 0")
        t = torch.arange(inter // 8, device=dev)[:, None]
        c = torch.arange(16, device=dev)[None, :]
        return torch.where(c < 8, t * 8 + c, inter + t * 8 + c - 8).reshape(-1)
    raise ValueError(f"unknown rowmap {rowmap}")


# fp8 activation quantisation modes (ops/csrc/quant_fp8.hip)
QUANT_NORM, QUANT_SILU, QUANT_PLAIN, QUANT_ADDNORM = 0, 1, 2, 3


def quant_rows_fp8(x: torch.Tensor, mode: int = QUANT_PLAIN, w: torch.Tensor | None = None,
                   eps: float = 1e-5, residual: torch.Tensor | None = None
                   ) -> tuple[torch.Tensor, torch.Tensor]:
    """Row-wise e4m3fn quantisation of ``x`` (``QUANT_PLAIN``), of rmsnorm(x) * w
    (``QUANT_NORM``), of silu(gate) * up for gate | up rows (``QUANT_SILU``), or - with
    ``QUANT_ADDNORM`` - ``residual += x`` (in place) then rmsnorm(residual) * w, fused in one
    HIP kernel.  Returns (uint8 codes [M, width], fp32 scales [M, 1])."""
    M = x.shape[0]
    width = x.shape[1] // 2 if mode == QUANT_SILU else x.shape[1]
    if not x.is_cuda:
        if mode == QUANT_ADDNORM:
            residual.copy_((x.float() + residual.float()).to(residual.dtype))
            x, mode = residual, QUANT_NORM
        if mode == QUANT_NORM:
            v = ref.rms_norm(x, w, eps).float()
        elif mode == QUANT_SILU:
            v = ref.silu_and_mul(x).float()
        else:
            v = x.float()
        s = (v.abs().amax(dim=1, keepdim=True) / FP8_MAX)
        s = torch.where(s > 0, s, torch.ones_like(s))
        q = (v / s).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
        return q, s
    q = torch.empty(M, width, dtype=torch.uint8, device=x.device)
    s = torch.empty(M, 1, dtype=torch.float32, device=x.device)
    _native().quant_rows_fp8(q, s, x, w if mode in (QUANT_NORM, QUANT_ADDNORM) else None, mode,
                             eps, residual if mode == QUANT_ADDNORM else None)
    return q, s


def gemm_fp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor,
             out_dtype=torch.bfloat16) -> torch.Tensor:
    """y[m, n] = xs[m] ws[n] sum_k fp8(xq)[m, k] fp8(wq)[n, k]: one hipBLASLt fp8 GEMM with
    row-wise scales on both operands (torch._scaled_mm, CDNA4 fp8 MFMA), bf16 out, no torch
    passes around it.  Failures raise: there is no silent dequantise fallback on a GPU."""
    if not xq.is_cuda:
        x = xq.view(torch.float8_e4m3fn).float() * xs
        w = wq.view(torch.float8_e4m3fn).float() * ws.reshape(-1, 1)
        return (x @ w.t()).to(out_dtype)
    return torch._scaled_mm(xq.view(torch.float8_e4m3fn), wq.view(torch.float8_e4m3fn).t(),
                            scale_a=xs, scale_b=ws.reshape(1, -1), out_dtype=out_dtype)


def linear_fp8(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """y = x @ dequant(q).T for 16-bit activations and row-major fp8 weights: the fused
    row-wise activation quantiser, then ``gemm_fp8``."""
    xq, xs = quant_rows_fp8(x, QUANT_PLAIN)
    return gemm_fp8(xq, xs, q, scale, x.dtype)


GEMM_PLAIN, GEMM_RESADD, GEMM_SILU = 0, 1, 2


def prefill_gemm_ok(x: torch.Tensor, w: torch.Tensor, mode: int = GEMM_PLAIN) -> bool:
    """Shapes the hand-written prefill GEMM (ops/csrc/prefill_gemm.hip) takes: bf16 or fp8
    (uint8 e4m3fn) operands, K a multiple of 64 bytes, output width a multiple of 256 (128
    for the SiLU mode), 16-B aligned rows."""
    return (w.dtype == x.dtype and x.dim() == 2 and x.shape[1] == w.shape[1]
            and prefill_gemm_shape_ok(x.dtype, x.shape[1], w.shape[0], mode)
            and x.stride(1) == 1 and (x.stride(0) * x.element_size()) % 16 == 0
            and w.is_contiguous())


def prefill_gemm_shape_ok(dtype: torch.dtype, k: int, w_rows: int, mode: int = GEMM_PLAIN) -> bool:
    """The shape rule of ``prefill_gemm_ok`` for contiguous ``dtype`` operands x [M, k] and
    w [w_rows, k], without the tensors (models/step_plan.py)."""
    n = w_rows // 2 if mode == GEMM_SILU else w_rows
    return (dtype in (torch.bfloat16, torch.uint8) and (k * dtype.itemsize) % 64 == 0
            and n % (128 if mode == GEMM_SILU else 256) == 0)


_PG_SCHEDULES = {"hybrid": 0, "streamk": 1, "dp": 2, "splitk": 3}


def prefill_gemm(x: torch.Tensor, w: torch.Tensor, mode: int = GEMM_PLAIN,
                 residual: torch.Tensor | None = None, out: torch.Tensor | None = None,
                 xs: torch.Tensor | None = None, ws: torch.Tensor | None = None,
                 schedule: str | None = None, bm: int = 0) -> torch.Tensor:
    """Hand-written CDNA4 prefill GEMM: ``x @ w.T`` (GEMM_PLAIN), ``residual += x @ w.T`` in
    place (GEMM_RESADD; returns ``residual``) or ``silu(x @ gate.T) * (x @ up.T)`` for
    ``w = [gate; up]`` (GEMM_SILU).  bf16 operands, or fp8: uint8 e4m3fn ``x`` / ``w`` with
    fp32 row scales ``xs`` [M, 1] / ``ws`` [rows of w] (applied in the epilogue).  fp32
    accumulate, one rounding to bf16.  ``schedule`` (hybrid / streamk / dp / splitk) and ``bm``
    (tile height 64 / 128 / 256; 0 = by row count) apply to this call only - nothing
    process-wide changes.  CPU tensors run the PyTorch reference of the op."""
    n = w.shape[0] // 2 if mode == GEMM_SILU else w.shape[0]
    fp8 = x.dtype == torch.uint8
    if fp8 and (xs is None or ws is None):
        raise ValueError("prefill_gemm: fp8 operands need row scales xs and ws")
    if not x.is_cuda:
        if fp8:
            xf = x.view(torch.float8_e4m3fn).float() * xs.reshape(-1, 1)
            wf = w.view(torch.float8_e4m3fn).float() * ws.reshape(-1, 1)
        else:
            xf, wf = x.float(), w.float()
        y = xf @ wf.t()
        if mode == GEMM_SILU:
            y = torch.nn.functional.silu(y[:, :n]) * y[:, n:]
        if mode == GEMM_RESADD:
            residual.copy_((y + residual.float()).to(residual.dtype))
            return residual
        y = y.to(torch.bfloat16)
        if out is not None:
            out.copy_(y)
            return out
        return y
    sched = -1 if schedule is None else _PG_SCHEDULES[schedule]
    xs_ = xs.reshape(-1) if fp8 else None
    ws_ = ws.reshape(-1) if fp8 else None
    if mode == GEMM_RESADD:
        _native().prefill_gemm(residual, x, w, residual, mode, xs_, ws_, sched, bm)
        return residual
    if out is None:
        out = torch.empty(x.shape[0], n, dtype=torch.bfloat16, device=x.device)
    _native().prefill_gemm(out, x, w, None, mode, xs_, ws_, sched, bm)
    return out


def gemm_w4a8_shape_ok(k: int, n: int, mode: int = GEMM_PLAIN, rowmap: str | None = None) -> bool:
    """The shape rule of ``gemm_w4a8`` for a weight of ``n`` rows and ``k`` columns, without the
    tensors: K in whole 128-wide chunks of the resident layout, N in whole 32-row MFMA
    fragments (the "qkv" rowmap: whole 128-dim heads); the SiLU mode is the "silu" rowmap's."""
    if mode not in (GEMM_PLAIN, GEMM_SILU) or (mode == GEMM_SILU and rowmap not in (None, "silu")):
        return False
    return k >= 128 and k % 128 == 0 and n >= 32 and n % (128 if rowmap == "qkv" else 32) == 0


def gemm_w4a8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, sq: torch.Tensor,
              rowmap: str, mode: int = GEMM_PLAIN, out: torch.Tensor | None = None
              ) -> torch.Tensor:
    """MXFP4 W4A8 GEMM: ``y[m, n] = xs[m] * sum_k e4m3(xq[m, k]) * w[n, k]`` with ``w`` the
    values of one projection's 4-bit copy (``wq`` / ``sq`` exactly as ``preshuffle_mxfp4(codes,
    scales, rowmap)`` returns them), fp32 accumulation, one rounding to bf16.  ``xq`` uint8
    [M, K] e4m3fn with fp32 row scales ``xs`` [M] or [M, 1] (``quant_rows_fp8``).
    ``GEMM_PLAIN``: [M, N] in the ORIGINAL weight-row order (the row map undone);
    ``GEMM_SILU`` ("silu" rowmap): ``silu(gate) * up`` -> [M, N / 2].  GPU tensors run the
    block-scaled MFMA kernel
    (csrc/prefill_gemm_w4a8.hip); CPU tensors compute the same from
    ``dequantize_mxfp4(*unshuffle_mxfp4(wq, sq, rowmap))`` in fp32.  A shape outside
    ``gemm_w4a8_shape_ok`` raises ValueError."""
    if rowmap not in ROWMAPS:
        raise ValueError(f"unknown rowmap {rowmap}")
    if xq.dim() != 2 or wq.dim() != 2 or xq.dtype != torch.uint8 or wq.dtype != torch.uint8:
        raise ValueError("gemm_w4a8: uint8 xq [M, K] and wq [N, K / 2]")
    n, k = wq.shape[0], wq.shape[1] * 2
    if not gemm_w4a8_shape_ok(k, n, mode, rowmap) or xq.shape[1] != k:
        raise ValueError(f"gemm_w4a8: K % 128 == 0, N % 32 == 0 (qkv rowmap: N % 128 == 0), the "
                         f"SiLU mode with the silu rowmap; got x {tuple(xq.shape)}, N {n}, K {k}, "
                         f"mode {mode}, rowmap {rowmap}")
    if xs.numel() != xq.shape[0]:
        raise ValueError("gemm_w4a8: one scale per row of xq")
    width = n // 2 if mode == GEMM_SILU else n
    if not xq.is_cuda:
        w = dequantize_mxfp4(*unshuffle_mxfp4(wq, sq, rowmap), torch.float32)
        y = (xq.view(torch.float8_e4m3fn).float() @ w.t()) * xs.reshape(-1, 1).float()
        if mode == GEMM_SILU:
            y = torch.nn.functional.silu(y[:, :width]) * y[:, width:]
        y = y.to(torch.bfloat16)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if out is None:
        out = torch.empty(xq.shape[0], width, dtype=torch.bfloat16, device=xq.device)
    _native().gemm_w4a8(out, xq, xs.reshape(-1), wq, sq, ROWMAPS[rowmap], mode)
    return out


W4A8_TILE = 64  # activation rows per tile of csrc/prefill_gemm_w4a8.hip


_PG_SCHEDULE = "hybrid"  # the configured (process-wide) default schedule


def prefill_gemm_config(schedule: str = "hybrid", group_m: int = 4, ablate: int = 0) -> None:
    """Process-wide defaults of the prefill GEMM: schedule "hybrid" (data-parallel rounds +
    Stream-K remainder), "streamk", "dp" or "splitk" (co-resident K slices of a few whole
    tiles with a parallel reduction, where T * S fits the CUs); ``group_m`` M tiles per raster
    group; ``ablate`` (measurement only, bf16 plain GEMMs): 1 no MFMA, 2 no LDS-DMA, 3 no
    ds_read; 4 (tests): every cross-workgroup wait gives up at once (recompute fallback)."""
    global _PG_SCHEDULE
    _native().prefill_gemm_config(_PG_SCHEDULES[schedule], group_m, ablate)
    _PG_SCHEDULE = schedule


def prefill_gemm_auto_bm(m: int) -> int:
    """Tile height the library picks for m rows (fewest padding rows)."""
    return int(_native().prefill_gemm_auto_bm(m))


def prefill_gemm_error() -> int:
    """Nonzero once a cross-workgroup wait of the prefill GEMM timed out (bit 1 stream-K,
    bit 2 split-K); bit 4 says the waiting workgroup recomputed its tile itself, so the
    outputs are still exact."""
    return int(_native().prefill_gemm_error())


def prefill_gemm_error_to(host: torch.Tensor, clear: bool = True) -> None:
    """Enqueue a copy of the prefill GEMM's error word into ``host`` (pinned int32) on the
    current stream; read it after the next synchronisation (no extra sync of its own).
    ``clear``: zero the word behind the copy, so each read covers the calls since the last."""
    _native().prefill_gemm_error_to(host, bool(clear))


def prefill_gemm_error_reset() -> None:
    """Zero the prefill GEMM's error word."""
    _native().prefill_gemm_error_reset()


def _need_cuda(x, preshuffled):
    if preshuffled and not x.is_cuda:
        raise ValueError("pre-shuffled weights are only consumed by the HIP decode kernels")


def linear(x: torch.Tensor, w: torch.Tensor, residual: torch.Tensor | None = None,
           out: torch.Tensor | None = None, waves: int | None = None,
           preshuffled: bool = False, w_scale: torch.Tensor | None = None,
           ksplit: int | None = 1, proj: str = "",
           w_block_scale: torch.Tensor | None = None, wide_w4: bool = False) -> torch.Tensor:
    """y = x @ w.T.  With ``residual`` the product is added to ``residual`` IN PLACE and
    ``residual`` is returned (residual-stream update).  Decode-sized M runs the MFMA skinny
    GEMM; everything else (prefill, CPU) runs F.linear (hipBLASLt on the GPU).
    ``preshuffled``: ``w`` comes from ``preshuffle`` (skinny path only).
    ``w_scale``: ``w`` is fp8 (uint8, ``preshuffle_fp8`` layout) with this per-row scale.
    ``w_block_scale``: ``w`` / this are the MXFP4 codes / block scales of
    ``preshuffle_mxfp4`` (at most 32 rows: the 16-row-tile GEMV alone streams them - unless
    ``wide_w4`` chooses the wide kernel's 4-bit builds for 33-128 rows)."""
    mxfp4 = w_block_scale is not None
    wide_w4 = wide_w4 and mxfp4
    _need_cuda(x, preshuffled or w_scale is not None or mxfp4)
    fp8 = w_scale is not None
    if fp8 or mxfp4:
        preshuffled = True
    fused = skinny_ok(x, w, preshuffled, fp8, mxfp4, wide_w4)
    if preshuffled and not fused:
        raise ValueError("pre-shuffled weights need the skinny (decode) path")
    if fused:
        ksplit = _ksplit(proj, x, ksplit, w.shape[0] // 16)
        if wide_w4:
            ensure_splitk_workspace(x.device)  # the wide kernel plans its own split
        if residual is not None:
            _native().skinny_gemm(residual, x, w, residual, waves or SKINNY_WAVES, preshuffled,
                                  w_scale, ksplit, w_block_scale, wide_w4)
            return residual
        if out is None:
            out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        _native().skinny_gemm(out, x, w, None, waves or SKINNY_WAVES, preshuffled, w_scale,
                              ksplit, w_block_scale, wide_w4)
        return out
    if residual is not None:
        # hipBLASLt C-matrix epilogue: residual = residual + x @ w.T in one GEMM (fp32
        # accumulate, one rounding), no separate add pass over the residual stream
        if residual.is_cuda:
            return residual.addmm_(x, w.t())
        residual.copy_((torch.nn.functional.linear(x, w).float() + residual.float())
                       .to(residual.dtype))
        return residual
    y = torch.nn.functional.linear(x, w)
    if out is not None:
        out.copy_(y)
        return out
    return y


def linear_push_reduce(x: torch.Tensor, w: torch.Tensor, residual: torch.Tensor, ipc,
                       waves: int | None = None, preshuffled: bool = False,
                       w_scale: torch.Tensor | None = None, proj: str = "") -> torch.Tensor:
    """TP row-parallel projection with the all-reduce push fused into the decode GEMV
    (SURVEY §2.5 X1 / X2): the GEMV epilogue writes this rank's partial product into every
    rank's IPC receive slot, then one receive kernel adds the rank-order sum into
    ``residual`` (returned).  ``ipc``: the TP group's IpcAllReduce."""
    if w_scale is not None:
        preshuffled = True
    if not skinny_ok(x, w):
        raise ValueError("linear_push_reduce: decode-sized rows only")
    n_out = w.shape[0]
    ksplit = _ksplit(proj, x, None, n_out // 16)
    ipc.gemv_push(x, w, n_out, waves or SKINNY_WAVES, preshuffled, w_scale, ksplit)
    return ipc.push_reduce(residual, n_out)


# ---- fused decode-step ops (norm weight folded into W on the host) -----------------------
def decode_qkv_rope(x, w, eps, positions, slots, cos_sin, k_cache, v_cache, n_q_heads,
                    n_kv_heads, q_out=None, preshuffled=False, w_scale=None, ksplit=None,
                    w_block_scale=None, waves=None, wide_w4=False):
    """RMSNorm(x) -> QKV GEMM -> RoPE -> q out + paged K/V write, one kernel on the GPU.
    ``w_block_scale``: MXFP4 weights (``preshuffle_mxfp4``, row map "qkv"); ``wide_w4``: as
    ``linear``'s."""
    mxfp4 = w_block_scale is not None
    wide_w4 = bool(wide_w4 and mxfp4 and x.is_cuda)
    if wide_w4:
        ensure_splitk_workspace(x.device)
    _need_cuda(x, preshuffled or w_scale is not None or mxfp4)
    check_slots(k_cache, slots[:x.shape[0]], "decode_qkv_rope")
    if q_out is None:
        q_out = torch.empty(x.shape[0], n_q_heads, 128, dtype=x.dtype, device=x.device)
    if not x.is_cuda:
        n = ref.rms_norm(x, torch.ones(x.shape[1], dtype=x.dtype), eps)
        q = ref.rope_cache(torch.nn.functional.linear(n, w), positions, slots, cos_sin, k_cache,
                           v_cache, n_q_heads, n_kv_heads, 128)
        q_out.copy_(q)
        return q_out
    _native().fused_qkv_rope(q_out, k_cache, v_cache, x, w, positions, slots, cos_sin,
                             n_q_heads, n_kv_heads, eps,
                             waves or decode_waves("qkv", preshuffled, w_scale is not None,
                                                   mxfp4=mxfp4),
                             preshuffled or w_scale is not None or mxfp4, w_scale,
                             _ksplit("qkv", x, ksplit, w.shape[0] // 16), w_block_scale,
                             wide_w4)
    return q_out


def decode_gate_up_silu(x, w, eps, out=None, preshuffled=False, w_scale=None, ksplit=None,
                        w_block_scale=None, waves=None, wide_w4=False):
    """RMSNorm(x) -> gate_up GEMM -> SiLU(gate) * up, one kernel on the GPU.
    ``w_block_scale``: MXFP4 weights (``preshuffle_mxfp4``, row map "silu"); ``wide_w4``: as
    ``linear``'s."""
    mxfp4 = w_block_scale is not None
    wide_w4 = bool(wide_w4 and mxfp4 and x.is_cuda)
    if wide_w4:
        ensure_splitk_workspace(x.device)
    _need_cuda(x, preshuffled or w_scale is not None or mxfp4)
    inter = w.shape[0] // 2
    if out is None:
        out = torch.empty(x.shape[0], inter, dtype=x.dtype, device=x.device)
    if not x.is_cuda:
        n = ref.rms_norm(x, torch.ones(x.shape[1], dtype=x.dtype), eps)
        out.copy_(ref.silu_and_mul(torch.nn.functional.linear(n, w)))
        return out
    waves = waves or decode_waves("gate_up", preshuffled, w_scale is not None, m=x.shape[0],
                                  mxfp4=mxfp4)
    _native().fused_gate_up_silu(out, x, w, eps, waves,
                                 preshuffled or w_scale is not None or mxfp4, w_scale,
                                 _ksplit("gate_up", x, ksplit, w.shape[0] // 16), w_block_scale,
                                 wide_w4)
    return out


MAX_TOP_LOGPROBS = 20  # most alternatives per position (csrc/logprobs.hip, SamplingParams)


def token_logprobs(logits, tokens, n_top: int = 0, out=None):
    """Logprobs of ``tokens`` (int64, one per row) under the raw ``logits`` rows (bf16 / fp32:
    before temperature, noise and top-k / top-p), in fp32, and the ``n_top`` (0 .. 20) most
    likely ids of each row with theirs - higher logit first, equal logits by lower id
    (csrc/logprobs.hip: one workgroup per row; ids and logits are read on the device and
    ``n_top`` is fixed per call, so the launch is graph-capturable).  Returns (lp [rows] fp32,
    top_ids [rows, n_top] int32, top_lp [rows, n_top] fp32); ``out``: that triple to fill."""
    rows = logits.shape[0]
    if not 0 <= n_top <= MAX_TOP_LOGPROBS:
        raise ValueError(f"token_logprobs: n_top {n_top} not in 0 .. {MAX_TOP_LOGPROBS}")
    if not logits.is_cuda:
        r = ref.token_logprobs(logits, tokens, n_top)
        if out is not None:
            for o, v in zip(out, r):
                o.view(-1)[:v.numel()].copy_(v.reshape(-1))
            return tuple(o.view(-1)[:v.numel()].view(v.shape) for o, v in zip(out, r))
        return r
    if out is None:
        out = (torch.empty(rows, dtype=torch.float32, device=logits.device),
               torch.empty(rows, n_top, dtype=torch.int32, device=logits.device),
               torch.empty(rows, n_top, dtype=torch.float32, device=logits.device))
    lp, top_ids, top_lp = out
    _native().token_logprobs(lp, top_ids, top_lp, logits, tokens, n_top)
    return (lp.view(-1)[:rows], top_ids.view(-1)[:rows * n_top].view(rows, n_top),
            top_lp.view(-1)[:rows * n_top].view(rows, n_top))


PENALTY_BIAS_ENTRIES = ref.PENALTY_BIAS_ENTRIES  # logit_bias entries per slot (csrc/penalties.hip)


def _i32(ids, device) -> torch.Tensor:
    if isinstance(ids, torch.Tensor):
        return ids.to(device=device, dtype=torch.int32).contiguous().view(-1)
    return torch.tensor(list(ids), dtype=torch.int32).to(device)


def penalty_seed(state_row, prompt_ids, output_ids, bias_ids_row, bias_vals_row,
                 bias_ids=(), bias_vals=()):
    """Reset one slot of the penalty state (csrc/penalties.hip): zero ``state_row`` [vocab]
    int32, set bit 31 of every prompt token, add one per occurrence of every output token
    (atomics: duplicates count), and write the slot's bias rows [300] (ids padded with -1).  The
    id lists are sequences or int32 tensors; ids outside the vocabulary are skipped.  Ordered
    on the current stream; called when a sequence is admitted, never on the decode path."""
    if not state_row.is_cuda:
        return ref.penalty_seed(state_row, prompt_ids, output_ids, bias_ids_row, bias_vals_row,
                                bias_ids, bias_vals)
    dev = state_row.device
    b_ids = _i32(bias_ids, dev)
    if isinstance(bias_vals, torch.Tensor):
        b_vals = bias_vals.to(device=dev, dtype=torch.float32).contiguous().view(-1)
    else:
        b_vals = torch.tensor(list(bias_vals), dtype=torch.float32).to(dev)
    _native().penalty_seed(state_row, bias_ids_row, bias_vals_row, _i32(prompt_ids, dev),
                           _i32(output_ids, dev), b_ids, b_vals)


def penalty_apply(out, logits, state, row_slot, rep, freq, pres, bias_ids, bias_vals):
    """``out`` [R, V] fp32 <- the penalised logits of ``logits`` [R, V] (bf16 / fp16 / fp32, any
    row stride): row r with slot s = row_slot[r] >= 0 reads state[s] (bit 31: in the prompt,
    bits 0-30: times generated) - seen tokens are divided (l > 0) or multiplied by rep[r], then
    l -= freq[r] * count + pres[r] * (count > 0), then the slot's bias entries are added; a row
    with a negative slot is copied through.  One dense pass and one launch for the bias entries;
    every parameter is a device tensor (graph-capturable)."""
    if not logits.is_cuda:
        return ref.penalty_apply(out, logits, state, row_slot, rep, freq, pres, bias_ids,
                                 bias_vals)
    _native().penalty_apply(out, logits, state, row_slot, rep, freq, pres, bias_ids, bias_vals)
    return out


def penalty_update(state, row_slot, tokens):
    """count[row_slot[r], tokens[r]] += 1 for the rows with a slot (after the sampler)."""
    if not state.is_cuda:
        return ref.penalty_update(state, row_slot, tokens)
    _native().penalty_update(state, row_slot, tokens)


def guide_apply(out, logits, next_table, state, row_slot):
    """``out`` [R, V] fp32 <- the masked logits of ``logits`` [R, V] (bf16 / fp16 / fp32, any row
    stride; may be ``out`` itself, fp32): row r with slot s = row_slot[r] in [0, slots) reads
    its pool state st = state[s] and gets -inf wherever next_table[st][v] < 0 (csrc/guided.hip);
    any other row is the raw logits in fp32.  Every parameter is a device tensor
    (graph-capturable)."""
    if not logits.is_cuda:
        return ref.guide_apply(out, logits, next_table, state, row_slot)
    _native().guide_apply(out, logits, next_table, state, row_slot)
    return out


def guide_advance(state, next_table, row_slot, tokens):
    """state[row_slot[r]] <- next_table[state[row_slot[r]]][tokens[r]] for the rows with a slot
    (after the sampler); a disallowed or out-of-range token leads to state 0."""
    if not state.is_cuda:
        return ref.guide_advance(state, next_table, row_slot, tokens)
    _native().guide_advance(state, next_table, row_slot, tokens)


def guide_seed(state, slot: int, value: int):
    """state[slot] <- value: one int32, ordered on the current stream (admission and
    re-admission of a guided sequence; never inside a graph)."""
    state[slot:slot + 1].fill_(int(value))


def decode_lm_head_sample(x, w, eps, temperature, seeds, steps, keys, tokens=None,
                          finalize=True, vocab_offset=0, preshuffled=False, logprobs=None,
                          lp_ws=None):
    """Final RMSNorm -> LM head -> greedy / Gumbel-max sample without materialising logits.
    ``keys`` (int64, >= M * vocab/16 entries) is scratch for the per-tile packed
    (value, index) maxima; no initialisation is needed.

    ``finalize``: True -> ``tokens`` gets token ids; ``"key"`` -> ``tokens`` gets each row's
    signed-orderable packed key (TP: MAX all-reduce them, then ``key_to_token``); False ->
    partials only.  ``vocab_offset`` is this shard's first vocab id.

    ``logprobs`` (fp32, >= M entries): also filled with each sampled token's logprob,
    ``l_tok - logsumexp(l)`` in fp32 over the raw logits the sampler sees (the LM-head product
    rounded to the model dtype, before temperature and noise) - the SAMPLE_LP epilogue, whose
    keys and tokens are bit-identical to the plain launch's.  Needs ``lp_ws``, fp32 scratch of
    4 words per ``keys`` entry, ``finalize=True`` and a whole vocabulary (``vocab_offset`` 0);
    16-bit weights only."""
    _need_cuda(x, preshuffled)
    if tokens is None:
        tokens = torch.empty(x.shape[0], dtype=torch.long, device=x.device)
    if logprobs is not None:
        if finalize is not True or vocab_offset != 0:
            raise ValueError("decode_lm_head_sample: logprobs need finalize=True on one shard")
        if not x.is_cuda:
            t, lp = ref.lm_head_sample_logprobs(x, w, eps, temperature, seeds, steps)
            tokens.copy_(t)
            logprobs[:lp.shape[0]].copy_(lp)
            return tokens
        if lp_ws is None:
            raise ValueError("decode_lm_head_sample: logprobs need the lp_ws workspace")
        _native().fused_lm_head_sample_lp(tokens, logprobs, keys, lp_ws, x, w, eps, temperature,
                                          seeds, steps, decode_waves("lm_head", preshuffled),
                                          preshuffled)
        return tokens
    if not x.is_cuda:
        n = ref.rms_norm(x, torch.ones(x.shape[1], dtype=x.dtype), eps)
        logits = torch.nn.functional.linear(n, w)
        if finalize == "key":
            tokens.copy_(ref.sample_keys(logits, temperature, seeds, steps, vocab_offset))
        else:
            tokens.copy_(ref.sample(logits, temperature, seeds, steps, vocab_offset))
        return tokens
    mode = 2 if finalize == "key" else (1 if finalize else 0)
    _native().fused_lm_head_sample(tokens, keys, x, w, eps, temperature, seeds, steps, mode,
                                   vocab_offset, decode_waves("lm_head", preshuffled),
                                   preshuffled)
    return tokens


def lm_head_score(x, w, eps, targets, ws, out=None, preshuffled=False):
    """Teacher-forced scoring in the fused LM head, no logits materialised: lp[m] = the logprob
    of token ``targets[m]`` (int32, inside the vocabulary: the caller's contract) in row m,
    ``l_tok - logsumexp(l)`` in fp32 over the LM-head product rounded to the model dtype, as a
    sampled token's logprob is defined (``eps`` > 0: the final RMSNorm first, its weight folded
    into ``w``).  The SCORE epilogue and its finalize (csrc/skinny.h): at most 128 rows over
    pre-shuffled weights, else 32; 16-bit weights; one GPU.  ``ws``: fp32 scratch of 4 words
    per (row, 16-column tile), i.e. ``M * vocab / 4`` floats.  Returns fp32 [M] (``out``'s
    first M entries when given)."""
    _need_cuda(x, preshuffled)
    m = x.shape[0]
    if targets.dtype != torch.int32 or targets.numel() < m:
        raise ValueError("lm_head_score: targets must be int32 with one id per row")
    if not x.is_cuda:
        lp = ref.lm_head_score(x, w, eps, targets[:m])
        if out is None:
            return lp
        out[:m].copy_(lp)
        return out[:m]
    kernel = fused_kernel(m, preshuffled, False, "score")
    if kernel is None:
        raise ValueError(f"lm_head_score: no fused kernel for {m} rows "
                         f"({'pre-shuffled' if preshuffled else 'row-major'} weights)")
    if ws is None:
        raise ValueError("lm_head_score: needs the ws workspace")
    if out is None:
        out = torch.empty(m, dtype=torch.float32, device=x.device)
    if kernel == "wide":  # its planner may split K
        ensure_splitk_workspace(x.device)
    _native().fused_lm_head_score(out, ws, x, w, eps, targets,
                                  decode_waves("lm_head", preshuffled), preshuffled)
    return out[:m]


def key_to_token(keys: torch.Tensor) -> torch.Tensor:
    """Decode signed-orderable packed sampler keys (``finalize="key"``) to token ids."""
    return 0xFFFFFFFF - (keys & 0xFFFFFFFF)


def set_attention_trace(trace=None):
    """Per-workgroup timeline of the decode attention launches that follow (int64 CUDA tensor
    of 4 words per workgroup of the (seqs, kv heads, partitions) grid: past round trip 1,
    computed, published, end - 100 MHz wall clock); None switches it off."""
    _native().set_attention_trace(trace)


def set_gemv_trace(trace=None):
    """Per-workgroup [start, end] timeline (100 MHz wall clock, int64 CUDA tensor of 2 words
    per workgroup) of the NEXT decode GEMV launch only; None clears it."""
    _native().set_gemv_trace(trace)


def attention_decode_v2(q, k_cache, v_cache, block_tables, seq_kvlen, seq_qstart, scale,
                        part_out, part_lse, counters, max_parts, part_tokens, out=None,
                        num_seqs: int = -1):
    """Decode attention with in-kernel split-K combine (one launch)."""
    check_paged_args(k_cache, block_tables, seq_kvlen, num_seqs, "attention_decode_v2")
    if not q.is_cuda:
        n = seq_kvlen.shape[0] if num_seqs < 0 else num_seqs
        return ref.paged_attention(q, k_cache, v_cache, block_tables[:n], seq_kvlen[:n],
                                   seq_qstart[:n + 1], scale, out=out)
    out = torch.empty_like(q) if out is None else out
    _native().attention_decode_v2(out, part_out, part_lse, counters, q, k_cache, v_cache,
                                  block_tables, seq_kvlen, seq_qstart, num_seqs, max_parts,
                                  part_tokens, q.shape[1], k_cache.shape[1], scale)
    return out


# partition sizes of the multi-query decode kernel (attention_decode_mq.hip): the 16-wave
# 512-token shape of the one-token kernel has no multi-query twin
MQ_PART_TOKENS = (64, 128, 256)
MQ_GROUPS = (1, 2, 3, 4, 8)


def mq_max_qlen(g: int) -> int:
    """Query tokens per sequence one multi-query decode launch takes: the GQA group's G heads
    of each token share the kernel's 16 MFMA columns."""
    return 16 // g


def mq_split_kvlen(seq_kvlen, seq_qstart, num_seqs: int = -1):
    """(kvlen of the one-token sequences, kvlen of the others), 0 elsewhere: the two kernels
    of ``attention_decode_mq`` each skip the sequences whose kvlen is 0.  Device ops; a caller
    that launches the op once per layer computes this once per step."""
    n = seq_kvlen.shape[0] if num_seqs < 0 else num_seqs
    one = (seq_qstart[1:n + 1] - seq_qstart[:n]) == 1
    kv = seq_kvlen[:n]
    zero = torch.zeros_like(kv)
    return torch.where(one, kv, zero), torch.where(one, zero, kv)


def attention_decode_mq(q, k_cache, v_cache, block_tables, seq_kvlen, seq_qstart, scale,
                        part_out, part_lse, counters, max_parts, part_tokens, out=None,
                        num_seqs: int = -1, max_qlen: int | None = None,
                        min_qlen: int | None = None, split=None):
    """Decode attention over 1 .. 16 // G query tokens per sequence (the verify step of
    speculative decoding): sequence s owns rows seq_qstart[s] .. seq_qstart[s + 1] - 1, row j
    of its qlen sits at position kvlen - qlen + j (``seq_kvlen`` counts this step's rows).
    Same arguments as ``attention_decode_v2``.

    Two launches over disjoint sequences: the one-token sequences run the one-token kernel
    (``attention_decode_v2``'s) - a sequence without drafts gets what a plain decode step
    computes, bit for bit - and the others the multi-query kernel; each kernel sees kvlen 0 for
    the other's sequences and leaves their rows alone.  ``split`` = ``mq_split_kvlen(...)`` of
    this step (computed here when None).  ``max_qlen`` / ``min_qlen``: the longest / shortest
    qlen as the host built the launch - a kernel with no sequence is not launched; without
    ``max_qlen`` it is read back from ``seq_qstart`` (a device synchronisation).  Out-of-range
    shapes raise here: nothing is launched."""
    g = q.shape[1] // k_cache.shape[1]
    n = seq_kvlen.shape[0] if num_seqs < 0 else num_seqs
    if q.shape[1] % k_cache.shape[1] or g not in MQ_GROUPS:
        raise ValueError(f"attention_decode_mq: GQA group {q.shape[1]} / {k_cache.shape[1]} "
                         f"not in {MQ_GROUPS}")
    if part_tokens not in MQ_PART_TOKENS:
        raise ValueError(f"attention_decode_mq: partitions of {MQ_PART_TOKENS} tokens "
                         f"(got {part_tokens})")
    if not 1 <= max_parts <= 64:
        raise ValueError(f"attention_decode_mq: 1 .. 64 partitions (got {max_parts})")
    if seq_qstart.shape[0] < n + 1:
        raise ValueError("attention_decode_mq: seq_qstart needs num_seqs + 1 entries")
    read_back = max_qlen is None or (DEBUG_CHECKS and not _capturing(seq_qstart))
    if read_back and n:
        qs = seq_qstart[:n + 1].long()
        ql = qs[1:] - qs[:-1]
        lo, hi, first, last = int(ql.min()), int(ql.max()), int(qs[0]), int(qs[-1])
        if lo < 0 or first < 0 or last > q.shape[0]:
            raise PagedArgsError(f"attention_decode_mq: query rows {first} .. {last} of "
                                 f"{q.shape[0]}, shortest qlen {lo}")
        if max_qlen is not None and hi > max_qlen:
            raise PagedArgsError(f"attention_decode_mq: qlen {hi} in seq_qstart, caller said "
                                 f"{max_qlen}")
        if min_qlen is not None and lo < min_qlen:
            raise PagedArgsError(f"attention_decode_mq: qlen {lo} in seq_qstart, caller said "
                                 f">= {min_qlen}")
        max_qlen = hi
    if n and g * max_qlen > 16:
        raise ValueError(f"attention_decode_mq: G * qlen = {g} * {max_qlen} > 16 MFMA columns")
    check_paged_args(k_cache, block_tables, seq_kvlen, num_seqs, "attention_decode_mq")
    if not q.is_cuda:
        return ref.paged_attention(q, k_cache, v_cache, block_tables[:n], seq_kvlen[:n],
                                   seq_qstart[:n + 1], scale, out=out)
    out = torch.empty_like(q) if out is None else out
    if n == 0:
        return out
    args = (q.shape[1], k_cache.shape[1], scale)
    if max_qlen == 1:  # nothing but one-token sequences: a plain decode launch
        _native().attention_decode_v2(out, part_out, part_lse, counters, q, k_cache, v_cache,
                                      block_tables, seq_kvlen, seq_qstart, n, max_parts,
                                      part_tokens, *args)
        return out
    if min_qlen is not None and min_qlen > 1:
        kv_one, kv_multi = None, seq_kvlen
    else:
        kv_one, kv_multi = mq_split_kvlen(seq_kvlen, seq_qstart, n) if split is None else split
    if kv_one is not None:
        _native().attention_decode_v2(out, part_out, part_lse, counters, q, k_cache, v_cache,
                                      block_tables, kv_one, seq_qstart, n, max_parts,
                                      part_tokens, *args)
    _native().attention_decode_mq(out, part_out, part_lse, counters, q, k_cache, v_cache,
                                  block_tables, kv_multi, seq_qstart, n, max_parts,
                                  part_tokens, *args)
    return out
