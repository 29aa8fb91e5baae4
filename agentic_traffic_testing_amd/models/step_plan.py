"""Which backend runs each projection of a T-row prefill / mixed step of the Llama forward.

``step_plan(T, facts)`` is the one place that decides it, once per ``LlamaModel.forward`` (the
same for every layer) and for the runner's row padding.  Pure: no native call, no tensor,
usable without a GPU.  Backends:

* ``fused``        the hand-written weight-streaming kernel ``ops.fused_kernel`` names (16-row-tile
                   GEMV, wide, mid-M) with its epilogue: RMSNorm + qkv + RoPE + KV write
                   (``ops.decode_qkv_rope``), RMSNorm + gate_up + SiLU-mul
                   (``ops.decode_gate_up_silu``), o / down + residual (``_row_parallel``)
* ``gemm``         the hand-written prefill GEMM (``ops.prefill_gemm``; o / down add the residual
                   and gate_up multiplies SiLU in its epilogue), separate norm / RoPE kernels
* ``gemm_splitk``  the same with the split-K schedule (o / down)
* ``lib``          the library GEMM (``ops.linear``, which itself sends at most 32 row-major rows
                   to the GEMV, or ``ops.gemm_fp8``) with separate norm / RoPE / SiLU kernels
* ``gemm_w4a8``    the MXFP4 W4A8 GEMM (``ops.gemm_w4a8``): row-quantised e4m3 activations times
                   the resident 4-bit weights on the block-scaled MFMA, inside the
                   activation-quantised chain ([4]); gate_up multiplies SiLU in its epilogue

The table, for a GPU model with the defaults (``prefill_gemm="auto"``, ``small_prefill_fused``
and ``fused_decode`` on, every projection's K in whole wave steps, ``ATTA_WIDE_MAX_M`` 128,
``ATTA_MIDM_MAX_M`` 1024); first matching row:

| weights              | TP  | rows               | qkv   | o           | gate_up     | down     |
|----------------------|-----|--------------------|-------|-------------|-------------|----------|
| 16-bit row-major     | any | 1-32               | fused | fused       | fused       | fused    |
| 16-bit pre-shuffled  | any | 1-128              | fused | fused       | fused       | fused    |
| 16-bit pre-shuffled  | 1   | 129-188, 448-640   | fused | fused       | lib         | fused    |
| 16-bit pre-shuffled  | 1   | 189-447            | fused | lib         | lib         | fused    |
| 16-bit               | any | the rest           | lib   | lib         | lib [1]     | lib [2]  |
| fp8                  | > 1 | 1-128              | fused | fused       | fused       | fused    |
| fp8, hidden 8192     | 1   | 1-48               | fused | fused       | fused       | fused    |
| fp8, hidden 8192     | 1   | 49-96              | fused | fused       | lib [3]     | fused    |
| fp8, hidden 4096     | 1   | 1-112              | fused | fused       | fused       | fused    |
| fp8, hidden 4096     | 1   | 113-128            | fused | fused       | lib [3]     | fused    |
| fp8, other widths    | 1   | 1-128              | fused | fused       | fused       | fused    |
| fp8                  | 1   | MIDM_FP8_ROWS (off)| fused | fused       | lib [3]     | fused    |
| fp8                  | any | the rest [4]       | lib   | lib         | lib [1]     | lib      |
| mxfp4                | 1   | 1-32               | fused | fused       | fused       | fused    |
| mxfp4                | 1   | the rest [5]       | as the 16-bit rows above                      |
| mxfp4, weights only  | 1   | 1-32               | fused | fused       | fused       | fused    |
| mxfp4, weights only  | 1   | 33-128 [6]         | fused | fused       | fused       | fused    |
| mxfp4, weights only  | 1   | the rest [6]       | expand + the "16-bit, the rest" row           |
| mxfp4, w4a8 [7]      | 1   | 129 and more       | ``gemm_w4a8`` on all four                     |

[1] no tuned library table loaded: ``gemm`` from 2048 rows (bf16) / 2560 rows (fp8).
[2] no tuned library table loaded, TP = 1, bf16: ``gemm_splitk`` at 448-1152 rows.
[3] inside a fused step: ``ops.gemm_fp8`` on the row-quantised (norm fused into the quantiser)
    activations, then bf16 SiLU-mul for the fused down.
[4] the activation-quantised fp8 chain (``fp8_chain``): every GEMM's activation operand comes
    quantised out of the norm / SiLU-mul kernel before it, and each down product is deferred
    into the next norm + quant kernel.

[5] ``quantization="mxfp4"`` keeps the projections dequantised in 16 bits, so a step past the
    4-bit GEMV's 32 rows is planned exactly as the same model without quantisation (pre-shuffled
    or row-major, whichever 16-bit copies exist); at most 32 rows stream the 4-bit copies.

[6] ``mxfp4_weights_only`` holds the projections in 4 bits alone: 33-128 rows run the wide
    kernel's 4-bit builds (``ops.fused_kernel(..., mxfp4=True, wide_w4=True)``); every other
    step expands each projection into the model's shared 16-bit scratch (``ops.expand_mxfp4``)
    just before its GEMM and is planned as the same model without quantisation and without
    pre-shuffled copies (library GEMMs, ``gemm`` where [1] / [2] route it, rows padded).

[7] ``w4a8`` (``mxfp4_fp8_activations``, either memory mode; it goes before the two "the
    rest" rows above): a step of more than 128 rows - and a smaller one that would otherwise
    expand, or run padded library GEMMs because the fused path is off - runs the chain of [4]
    with every GEMM on ``ops.gemm_w4a8``: no expand pass, no 16-bit scratch, rows not padded.
    The CPU reference gets the same plan and runs the chain's arithmetic on the dequantised
    weights.

fp8 weights are always pre-shuffled on a GPU (without the copies no fp8 step runs fused).  With
the fused path off (either switch, a K that is not whole wave steps, the kernel limits) a step
takes "the rest" rows; 16-bit weights other than bf16 never take ``gemm``.
``prefill_gemm="hipblaslt"`` drops [1] and [2]; ``"atta"`` turns every ``lib`` above into
``gemm`` from ``prefill_gemm_min_rows`` rows where the GEMM takes the shape
(``ops.prefill_gemm_shape_ok``).  Rows are padded to the tuned library buckets by the runner
(``pad_rows``) unless a step of <= 128 rows runs fused.  On the CPU everything is ``lib``
(but [7]).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field, replace

import torch

from .. import ops

PROJS = ("qkv", "o", "gate_up", "down")
# tile row map of each projection's 4-bit copy (ops.preshuffle_mxfp4)
W4_ROWMAPS = {"qkv": "qkv", "o": "plain", "gate_up": "silu", "down": "plain"}
FUSED, GEMM, GEMM_SPLITK, LIB = "fused", "gemm", "gemm_splitk", "lib"
GEMM_W4A8 = "gemm_w4a8"

# "auto" routing of the prefill projections: (weight dtype, projection) -> the smallest row count
# from which the hand-written GEMM beat hipBLASLt in the cold-weight A/B on the 8B shapes.
# Round 4 re-measured against the library as the engine now runs it
# (profiles/r4_prefill_gemm_largem_ab.txt): bf16 on the tuned table (gemm_tuning) wins every
# projection at 2048-4096 rows (the hand-written gate_up+SiLU 0.84-0.88x), so bf16 routes
# here only when no tuned table is loaded (round 3: 1.06-1.10x over the untuned heuristic at
# 2600); fp8 gate_up+SiLU 1.08x at 3200, parity at 2048, 0.82-0.92x below; fp8 down
# 0.89-0.93x (was routed from 2048 in round 3).
# Against the shipped tuned tables the hand-written prefill GEMM wins nowhere that the
# workload reaches (round 5, profiles/r5_prefill_gemm_vs_tuned.txt: fp8 gate_up+SiLU
# 0.88-0.95x at 2560-3200 rows, bf16 down split-K 0.59-1.03x at 448-1152), so with a table
# loaded nothing is routed to it; without one (models with no shipped table) it keeps the
# shapes where it beat the untuned library (r3 / r4)
PG_AUTO: dict = {}
PG_AUTO_UNTUNED = {(torch.bfloat16, "gate_up"): 2048, (torch.uint8, "gate_up"): 2560}
# row ranges where the split-K schedule (co-resident K slices of the few 256 x 256 tiles,
# parallel reduction) beat the UNTUNED hipBLASLt: bf16 down+residual 1.12-1.15x at M 512 /
# 1024, parity at 400 (profiles/r3_prefill_gemm_ab_bf16_splitk.txt); not used with a table.
# Split-K needs its T * S workgroups co-resident: TP = 1 only (one process per GPU)
PG_SPLITK = {(torch.bfloat16, "down"): (448, 1152)}

# Per-projection row ranges where the mid-M kernel (fused epilogues included) beat the tuned
# library GEMM plus its separate norm / RoPE / SiLU kernels at the 8B shapes, cold weights,
# library rows padded to the tuning buckets as the engine runs them
# (profiles/r6_midm_vs_tuned.txt): qkv + RoPE 1.05-1.48x at 129-640 rows, down + residual
# 1.03-1.41x at 129-640, o + residual 1.05-1.17x at 129-188 and 1.06-1.12x at 448-640;
# gate_up + SiLU loses everywhere (0.59-0.93x: the kernel streams ~52 GB/s per CU at ~35 %
# MFMA, the library's 256-wide tiles run ~41 %).  Measured at TP = 1 shapes only.
MIDM_ROUTES = {"qkv": ((129, 640),), "o": ((129, 188), (448, 640)), "gate_up": (),
               "down": ((129, 640),)}

# fp8 (weight-only) steps of these rows run qkv / o / down on the mid-M kernel's W8 builds
# instead of the row-quantised library fp8 GEMMs (ATTA_MIDM_FP8_ROWS="lo-hi"); gate_up is past
# its crossover below and runs the library fp8 GEMM.  All or nothing for the other three: the
# library fp8 chain defers each down product into the next layer's norm-quant kernel, which a
# fused qkv cannot take.  Off by default: the library's fp8 MFMA GEMMs win from 274 rows on at
# the 8B shapes (bench fp8 uncached planning 274 rows 5.68 vs 7.47 ms, burst 392 rows 6.42 vs
# 9.35 ms, profiles/r6_midm_fp8_negative.txt) - the W8 builds run bf16 MFMAs at ~35 % busy
_fp8_rows = os.environ.get("ATTA_MIDM_FP8_ROWS", "0")
MIDM_FP8_ROWS = ((0, -1) if _fp8_rows in ("", "0") else
                 tuple(int(v) for v in _fp8_rows.split("-")))

# fp8 weights, TP = 1: most rows of a fused-path step whose gate_up + SiLU still runs the
# wide kernel's W8 build, by hidden size; past it the library fp8 GEMM wins (cold weights,
# bench_wide --fp8 --tuned, profiles/r6_wide_fp8.txt: 8B 38.4 vs 47.4 us at 75 rows, 50.9
# vs 47.4 at 128; 70B 106 vs 117 at 33 rows, 123 vs 118 at 64).  qkv / o / down keep the
# W8 builds to 128 rows (1.14-1.9x at <= 96 rows, 0.93-0.97x at 128 on the 70B shapes).
# TP > 1: the shards' library GEMMs are launch-bound, not measured past the wide kernel's rows
FP8_GATE_UP_WIDE_MAX = {4096: 112, 8192: 48}
# and the whole fused step: 70B fp8 prefill 33 / 76 / 112 / 128 rows 15.4 / 21.4 / 23.8 /
# 24.3 ms fused vs 20.6 / 22.4 / 23.2 / 23.3 on the library chain
# (profiles/r6_70b_fp8_planning_prefill.txt)
FP8_FUSED_MAX_ROWS = {8192: 96}


@dataclass(frozen=True)
class StepFacts:
    """What decides a step's plan besides its rows: fixed for a step, the same for every layer.
    Widths are this TP rank's."""
    gpu: bool                   # a GPU model (the CPU reference runs the library ops)
    quant: str                  # "" | "fp8" | "mxfp4"
    wdtype: torch.dtype         # the projections' storage dtype (fp8 on a GPU: torch.uint8)
    tp_size: int
    preshuffled: bool           # prepare_decode_weights() built the pre-shuffled copies
    hidden: int
    q_width: int                # n_heads * head_dim
    kv_width: int               # n_kv_heads * head_dim
    inter: int
    gemm_tuned: bool = False    # a tuned library table is loaded
    prefill_gemm: str = "auto"  # "hipblaslt" | "auto" | "atta"
    prefill_gemm_min_rows: int = 128
    small_prefill_fused: bool = True
    fused_decode: bool = True
    w4_only: bool = False       # mxfp4_weights_only: no 16-bit projections exist
    w4a8: bool = False          # mxfp4_fp8_activations: steps past the 4-bit fused kernels run
                                # the activation-quantised chain on ops.gemm_w4a8
    # the measured tables above
    midm_routes: dict = field(default_factory=lambda: MIDM_ROUTES)
    pg_auto: dict = field(default_factory=lambda: PG_AUTO)
    pg_auto_untuned: dict = field(default_factory=lambda: PG_AUTO_UNTUNED)
    pg_splitk: dict = field(default_factory=lambda: PG_SPLITK)
    midm_fp8_rows: tuple = MIDM_FP8_ROWS
    fp8_gate_up_wide_max: dict = field(default_factory=lambda: FP8_GATE_UP_WIDE_MAX)
    fp8_fused_max_rows: dict = field(default_factory=lambda: FP8_FUSED_MAX_ROWS)

    @property
    def dims_ok(self) -> bool:
        return proj_dims_ok(self.gpu, self.quant, self.hidden, self.q_width, self.inter)

    def kn(self, proj: str) -> tuple[int, int]:
        """(K, weight rows) of a projection."""
        return {"qkv": (self.hidden, self.q_width + 2 * self.kv_width),
                "o": (self.q_width, self.hidden), "gate_up": (self.hidden, 2 * self.inter),
                "down": (self.inter, self.hidden)}[proj]


@dataclass(frozen=True)
class StepPlan:
    qkv: str
    o: str
    gate_up: str
    down: str
    fp8_chain: bool  # the activation-quantised library fp8 chain ([4] above)
    pad_rows: bool   # the runner pads this step's rows to the tuned library buckets


def proj_dims_ok(gpu: bool, quant: str, hidden: int, q_width: int, inter: int) -> bool:
    """Every projection's K in whole wave steps of the weight-streaming kernels (16-bit GEMVs:
    K % 128 = 4 waves x 32; fp8: K % 256 = 4 waves x 64; mxfp4: K % 128 = one 128-wide lane
    load - the loads need not divide evenly among the waves)."""
    step = 256 if quant == "fp8" else 128
    return gpu and hidden % step == 0 and inter % step == 0 and q_width % step == 0


def proj_fusable(T: int, dims_ok: bool, tp_size: int, preshuffled: bool, quant: str,
                 w4_only: bool = False) -> bool:
    """LlamaModel.proj_fusable."""
    if w4_only:  # the 4-bit copies are all there is
        kernel = ops.fused_kernel(T, True, mxfp4=True, wide_w4=True)
    else:
        kernel = ops.fused_kernel(T, preshuffled, preshuffled and quant == "fp8")
        if kernel is None and quant == "mxfp4":
            kernel = ops.fused_kernel(T, True, mxfp4=True)
    return dims_ok and (tp_size == 1 or T <= ops.WIDE_ROWS) and kernel is not None


def _lib_or_gemm(T: int, f: StepFacts, proj: str, mode: int) -> str:
    """The backend of a projection that no fused kernel runs: the library, or the hand-written
    prefill GEMM with ``prefill_gemm == "atta"`` (from ``prefill_gemm_min_rows`` rows) or
    ``"auto"`` (the measured winners: PG_SPLITK for the residual-add mode, PG_AUTO), for
    shapes it takes."""
    if not f.gpu or not ops.prefill_gemm_shape_ok(f.wdtype, *f.kn(proj), mode):
        return LIB
    if f.prefill_gemm != "auto":
        return GEMM if f.prefill_gemm == "atta" and T >= f.prefill_gemm_min_rows else LIB
    key = (f.wdtype, proj)
    if mode == ops.GEMM_RESADD and f.tp_size == 1 and not f.gemm_tuned:
        lo, hi = f.pg_splitk.get(key, (1, 0))
        if lo <= T <= hi:
            return GEMM_SPLITK
    m = f.pg_auto.get(key)
    if m is None and not f.gemm_tuned:
        m = f.pg_auto_untuned.get(key)
    return GEMM if m is not None and T >= m else LIB


def step_plan(T: int, f: StepFacts) -> StepPlan:
    """The plan of a T-row prefill / mixed step (the table in the module comment)."""
    if f.quant == "mxfp4":
        if (f.gpu and f.tp_size == 1 and f.small_prefill_fused and f.fused_decode and f.dims_ok
                and ops.fused_kernel(T, True, mxfp4=True, wide_w4=f.w4_only) is not None):
            return StepPlan(FUSED, FUSED, FUSED, FUSED, fp8_chain=False, pad_rows=False)
        # w4a8: past the wide kernel's rows, and wherever the step would otherwise expand
        # (weights only) or leave the small fused step of the 16-bit copies for padded library
        # GEMMs; the CPU reference follows the row rule alone, as a GPU with the defaults does
        if f.w4a8 and (f.w4_only or T > ops.WIDE_ROWS
                       or (f.gpu and step_plan(T, replace(f, quant="")).pad_rows)):
            # every shape the resident layout admits (K % 128, 16-row tiles in pairs) is one the
            # GEMM takes; a GPU model whose shapes it does not take cannot run this mode at all
            if f.gpu and not all(
                    ops.gemm_w4a8_shape_ok(*f.kn(p), ops.GEMM_SILU if p == "gate_up"
                                           else ops.GEMM_PLAIN, W4_ROWMAPS[p]) for p in PROJS):
                raise ValueError("mxfp4_fp8_activations: a projection shape ops.gemm_w4a8 does "
                                 "not take (K % 128 == 0, N % 32 == 0)")
            return StepPlan(GEMM_W4A8, GEMM_W4A8, GEMM_W4A8, GEMM_W4A8, fp8_chain=True,
                            pad_rows=False)
        if f.w4_only:
            # expand + the plan of the unquantised model without pre-shuffled copies, library
            # side only: a row-major GEMV would re-read the scratch it was just expanded into
            return step_plan(T, replace(f, quant="", w4_only=False, preshuffled=False,
                                        small_prefill_fused=False))
        return step_plan(T, replace(f, quant=""))
    fp8 = f.quant == "fp8" and f.gpu
    tp1 = f.tp_size == 1
    wide = ops.WIDE_ROWS
    on = (f.small_prefill_fused and f.fused_decode
          and proj_fusable(T, f.dims_ok, f.tp_size, f.preshuffled, f.quant))
    fp8_max = f.fp8_fused_max_rows.get(f.hidden, wide) if tp1 else wide
    small = on and T <= wide and (f.quant != "fp8" or (f.preshuffled and T <= fp8_max))
    lo, hi = f.midm_fp8_rows
    if small or (on and fp8 and tp1 and T > wide and lo <= T <= hi):
        gate_up = FUSED
        if fp8 and T > (f.fp8_gate_up_wide_max.get(f.hidden, wide) if tp1 else wide):
            gate_up = _lib_or_gemm(T, f, "gate_up", ops.GEMM_PLAIN)
        return StepPlan(FUSED, FUSED, gate_up, FUSED, fp8_chain=False, pad_rows=not small)
    if fp8:
        return StepPlan(_lib_or_gemm(T, f, "qkv", ops.GEMM_PLAIN),
                        _lib_or_gemm(T, f, "o", ops.GEMM_PLAIN),
                        _lib_or_gemm(T, f, "gate_up", ops.GEMM_SILU),
                        _lib_or_gemm(T, f, "down", ops.GEMM_PLAIN), fp8_chain=True, pad_rows=True)
    midm = on and tp1 and T > wide

    def pick(proj, mode):
        if midm and any(lo <= T <= hi for lo, hi in f.midm_routes.get(proj, ())):
            return FUSED
        return _lib_or_gemm(T, f, proj, mode)

    return StepPlan(pick("qkv", ops.GEMM_PLAIN), pick("o", ops.GEMM_RESADD),
                    pick("gate_up", ops.GEMM_SILU), pick("down", ops.GEMM_RESADD),
                    fp8_chain=False, pad_rows=True)
