"""Model runner: KV-cache allocation, per-step input preparation, hipGraph decode replay.

One step = one forward over a decode-first ``Batch`` (scheduler.py) followed by sampling.

* **KV cache** - one [L, nb, Hkv, BS, D] K tensor and one [L, nb, Hkv, D, BS] V tensor (V
  transposed for the PV MFMA, see ops/csrc/attention.hip).  ``num_blocks`` comes from
  ``gpu_memory_utilization`` of the device's HBM after weights and an activation reserve,
  i.e. ~1.9 M tokens for Llama-3-8B at 0.9 of 288 GB.
* **Metadata** - the native block manager emits int32 arrays which are packed into ONE
  pinned host buffer and moved with ONE async H2D copy per step; every device metadata
  tensor is a view into the matching device buffer.  What a step is beyond its arrays - the
  layout's sizes, graph bucket, variant, scoring and verify fields - is one ``StepHeader``
  (step_msg.py), which ``_run`` executes; its variant is decoded once into a ``SamplePlan``
  and bound to the step's sampling fields as the ``SampleArgs`` of the model's one sampler
  tail (``LlamaModel.sample_tail``).
* **hipGraphs** - decode-only steps are padded to a bucket (1, 2, 4, 8, ...) and replayed
  from a captured graph that contains the whole forward, the LM head and the sampler, so a
  decode step costs one graph launch instead of ~330 kernel launches.
* **Tensor parallelism** - rank 0 owns scheduler + block manager; every step it packs the
  same int32 metadata it uploads into a step message (``StepHeader.words()`` + payload) and
  publishes it on a shared-memory channel (runtime/csrc/shm_channel.cpp).  TP worker ranks
  (``serve_worker``) parse each message back into a ``StepHeader`` and replay exactly the
  same kernel / collective sequence from it, graph captures (OP_CAPTURE) included, so the
  RCCL all-reduces line up.
"""
from __future__ import annotations

import collections
import math
import os
import threading
import time

import numpy as np
import torch

from .. import ops
from ..config import EngineConfig, ModelConfig
from ..models.llama import AttnMeta, LlamaModel, SampleArgs, torch_dtype
from ..ops import reference as ref
from ..runtime import BlockManager
from .scheduler import Batch
from .step_msg import (HDR_WORDS, LP_NONE, LP_SAMPLED, LP_TOPN, OP_BARRIER, OP_CAPTURE, OP_STEP,
                       OP_STOP, SCORE_TOPN, TOP_N, V_GUIDE, V_PENALTY, V_SCORE, V_TOPKP,
                       SamplePlan, StepHeader, sample_plan, variant_code, variant_lp)


def _even(n: int) -> int:
    return n + (n & 1)


class MetaLayout:
    """int32-word layout of the packed per-step metadata buffer."""

    def __init__(self, T: int, S: int, W: int, NT: int, R: int | None = None,
                 penalty: bool = False, guide: bool = False, score: int = 0):
        # R: rows the sampler runs over - one per sequence, or every row of a verify step
        # (speculative decoding), whose sampling fields are row-sized
        # penalty: a step of a penalty variant (V_PENALTY) carries four more per-row fields
        # behind the others; every other step's layout is what it was without them
        # guide: a step of a guide variant (V_GUIDE) carries one more per-row field behind those
        # score: rows a scoring step (V_SCORE) scores - two more fields of that many entries
        # behind those, present only in such a step
        R = S if R is None else R
        self.T, self.S, self.W, self.NT, self.R = T, S, W, NT, R
        self.penalty = bool(penalty)
        self.guide = bool(guide)
        self.score = int(score)
        o = 0
        self.fields = {}

        def add(name, n, dtype=torch.int32):
            nonlocal o
            words = n * (2 if dtype == torch.int64 else 1)
            if dtype == torch.int64:
                o = _even(o)
            self.fields[name] = (o, n, dtype)
            o += words

        add("input_ids", T)
        add("positions", T)
        add("slot_mapping", T)
        add("block_tables", S * W)
        add("seq_kvlen", S)
        add("seq_qstart", S + 1)
        add("tile_seq", NT)
        add("tile_qoff", NT)
        add("feed_prev", 1)     # 1: decode rows take the previous step's device samples
        add("temperature", R, torch.float32)
        add("top_p", R, torch.float32)  # >= 1: off
        add("top_k", R)                 # <= 0: off
        add("logits_idx", R, torch.int64)
        add("seeds", R, torch.int64)
        add("steps", R, torch.int64)
        if penalty:
            add("pen_slot", R)                  # row of the penalty state; < 0: row unpenalised
            add("pen_rep", R, torch.float32)    # repetition / frequency / presence penalty
            add("pen_freq", R, torch.float32)
            add("pen_pres", R, torch.float32)
        if guide:
            add("guide_slot", R)                # entry of the guide state; < 0: row unguided
        if score:
            # prompt logprobs: the step's rows to score and the token each one predicts - a
            # field of its own, since a chunk's last row predicts the next prompt token, which
            # is not among this step's input_ids
            add("score_idx", score, torch.int64)
            add("score_tgt", score)
        self.size = _even(o)

    def views(self, buf: torch.Tensor) -> dict:
        out = {}
        for name, (o, n, dt) in self.fields.items():
            if dt == torch.int64:
                out[name] = buf[o:o + 2 * n].view(torch.int64)
            elif dt == torch.float32:
                out[name] = buf[o:o + n].view(torch.float32)
            else:
                out[name] = buf[o:o + n]
        out["block_tables"] = out["block_tables"].view(self.S, self.W)
        return out

    def pack(self, host: np.ndarray, arrays: dict):
        for name, (o, n, dt) in self.fields.items():
            a = arrays.get(name)
            if a is None:
                continue
            if dt == torch.int64:
                host[o:o + 2 * n].view(np.int64)[:len(a)] = a
            elif dt == torch.float32:
                host[o:o + n].view(np.float32)[:len(a)] = a
            else:
                host[o:o + n][:a.size] = a.reshape(-1)


class SlotPool:
    """Rows of a per-sequence device state ("slots"), handed to running sequences (host
    bookkeeping only): ``slots`` maps seq_id -> slot, ``free`` holds the rest."""

    def __init__(self, feature: str, n: int):
        self.feature = feature
        self.slots: dict[int, int] = {}
        self.free = list(range(n - 1, -1, -1))   # slot 0 goes first

    def acquire(self, seq_id: int) -> tuple[int, bool]:
        """(the sequence's slot, whether it is fresh: the caller seeds it)."""
        slot = self.slots.get(seq_id)
        if slot is not None:
            return slot, False
        if not self.free:  # running sequences <= max_num_seqs, each holds at most one
            raise RuntimeError(f"no free {self.feature} slot: a finished, aborted or preempted "
                               "sequence was not released")
        slot = self.slots[seq_id] = self.free.pop()
        return slot, True

    def release(self, seq_id: int) -> None:
        slot = self.slots.pop(seq_id, None)
        if slot is not None:
            self.free.append(slot)


class ModelRunner:
    def __init__(self, cfg: EngineConfig, model_cfg: ModelConfig, device: str = "cuda",
                 comm=None, weights_dir=None):
        self.cfg = cfg
        self.mcfg = model_cfg
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"
        self.dtype = torch_dtype(cfg.dtype)
        self.comm = comm
        tp_rank, tp_size = (comm.rank, comm.size) if comm is not None else (0, 1)
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.publisher = None     # rank 0 of a TP group: ShmChannel to the workers
        t0 = time.perf_counter()
        self.model = LlamaModel(model_cfg, self.dtype, self.device, tp_rank, tp_size, comm,
                                quantization=cfg.quantization,
                                mxfp4_weights_only=cfg.mxfp4_weights_only,
                                mxfp4_fp8_activations=cfg.mxfp4_fp8_activations)
        self.model.prefill_gemm = cfg.prefill_gemm
        self.model.prefill_gemm_min_rows = cfg.prefill_gemm_min_rows
        self.model.small_prefill_fused = cfg.small_prefill_fused
        # tuned library-GEMM table (agentic_traffic_testing_amd/tuning): prefill steps pad
        # their rows to its buckets so their GEMMs hit tuned shapes
        self.gemm_table = None
        if self.device.type == "cuda" and cfg.gemm_tuning:
            from .. import tuning

            self.gemm_table = tuning.load(cfg.gemm_tuning, model_cfg.name)
        self.model.gemm_tuned = self.gemm_table is not None
        if weights_dir and cfg.load_format != "dummy":
            self.model.load_safetensors(weights_dir)
        else:
            self.model.init_random(seed=cfg.seed)
        if self.is_cuda and cfg.quantization == "mxfp4":
            # the 4-bit copies first (always), so the room check below counts them
            self.model.prepare_decode_weights(copies16=False)
        if self.is_cuda and ((cfg.fused_decode and cfg.preshuffle_decode_weights
                              and self._room_for_decode_copies())
                             or cfg.quantization == "fp8"):
            self.model.prepare_decode_weights()
        self.load_seconds = time.perf_counter() - t0
        # device bytes of the weights by kind (LlamaModel.resident_weight_bytes)
        self.resident_weights = self.model.resident_weight_bytes()
        if cfg.mxfp4_weights_only:
            rw = self.resident_weights
            print(f"[atta] weights loaded in {self.load_seconds:.1f} s, resident: 4-bit codes "
                  f"{rw['codes4'] / 2**30:.2f} GiB, block scales {rw['scales4'] / 2**30:.2f} GiB, "
                  f"16-bit rest {rw['w16'] / 2**30:.2f} GiB, expand scratch "
                  f"{rw['scratch'] / 2**30:.2f} GiB", flush=True)
        if cfg.mxfp4_fp8_activations:
            print("[atta] mxfp4 fp8 activations (W4A8): steps without a fused 4-bit kernel run "
                  "e4m3 activations x 4-bit weights (ops.gemm_w4a8)"
                  + (", no expand scratch" if cfg.mxfp4_weights_only else ""), flush=True)
        if self.is_cuda:
            # split-K GEMV workspace up front (32 MiB): a split chosen while a decode graph is
            # being captured (ATTA_DECODE_KSPLIT, TP shards) must not allocate inside the capture
            ops.ensure_splitk_workspace(self.device)
            if cfg.fused_decode:
                ops.warm_wide_kernels(self.device, self.dtype, wide_w4=cfg.mxfp4_weights_only,
                                      expand=not cfg.mxfp4_fp8_activations)
            if cfg.startup_warmup:
                self.warm_library_gemms()
                if cfg.mxfp4_fp8_activations:
                    self.warm_w4a8_kernels()
        self.block_size = cfg.block_size
        self.bt_width = math.ceil(cfg.max_model_len / cfg.block_size)
        self.part_tokens = cfg.decode_partition_tokens
        self.max_parts = max(1, math.ceil(cfg.max_model_len / self.part_tokens))
        # small decode batches split the context finer (more workgroups in flight for the
        # latency-bound attention): partition tiers by batch size, finest first - the optional
        # tiny tier (<= decode_tiny_batch_max, 64 tokens; off by default, see config.py) and
        # small (<= decode_small_batch_max, 128 tokens); partial buffers are sized for the
        # finest split
        self.part_tiers = []  # (max batch, partition tokens, max partitions, graph buckets)
        for mb, pt in ((cfg.decode_tiny_batch_max, cfg.decode_partition_tokens_tiny),
                       (cfg.decode_small_batch_max, cfg.decode_partition_tokens_small)):
            if mb <= 0 or not pt or pt == self.part_tokens:
                continue
            mp = max(1, math.ceil(cfg.max_model_len / pt))
            if mp > 64:  # in-kernel combine handles <= 64 partitions
                continue
            bk = sorted({p for p in cfg.graph_parts_buckets if p < mp} | {mp})
            self.part_tiers.append((mb, pt, mp, bk))
        # drafts per sequence and verify step (speculative decoding; 0 = off)
        self.spec_tokens = 0
        if cfg.speculative and self.model.g in ops.MQ_GROUPS:
            self.spec_tokens = max(0, min(cfg.spec_tokens, ops.mq_max_qlen(self.model.g) - 1))
        alloc_parts = max([self.max_parts] + [t[2] for t in self.part_tiers])
        if self.spec_tokens and self.part_tokens not in ops.MQ_PART_TOKENS:
            alloc_parts = max(alloc_parts, min(64, math.ceil(cfg.max_model_len / 256)))
        # decode graphs are captured per (batch bucket, partition bucket): the attention grid
        # is (seqs, kv heads, partitions) and every workgroup past a sequence's context still
        # costs a dispatch and a round trip - a 32-partition grid (max_model_len 8192) over
        # 3k-token contexts ran 2.6x the workgroups it needed
        # (profiles/r2_fused_qkv_attn_experiment.txt: B=8 attention 21.9 us vs 10.8 at B=1)
        self.parts_buckets = sorted({p for p in cfg.graph_parts_buckets if p < self.max_parts}
                                    | {self.max_parts})
        self.tile_tokens = ops.prefill_tile_tokens(self.model.g, bt_width=self.bt_width)
        self.graph_sizes = sorted(b for b in cfg.graph_batch_sizes)
        cap = next((b for b in self.graph_sizes if b >= cfg.max_num_seqs), cfg.max_num_seqs)
        self.graph_sizes = [b for b in self.graph_sizes if b <= cap]
        self.max_seqs = max(cfg.max_num_seqs, self.graph_sizes[-1] if self.graph_sizes else 1)
        self.max_tokens = cfg.max_num_batched_tokens + self.max_seqs
        # speculative decoding: a verify step carries 1 + k rows per sequence through the fused
        # decode path, k <= 16 // G - 1 (the multi-query attention kernel's columns); its
        # attention needs a partition shape that kernel has (64, 128, 256 tokens) - a batch
        # whose tier has none verifies at 256, and contexts past 64 such partitions get no
        # drafts.  ws_rows sizes the fused workspaces (q / attn / act / keys / tokens).
        self.ws_rows = self.max_seqs
        if self.spec_tokens:
            self.ws_rows = max(self.max_seqs,
                               min(self.max_seqs * (1 + self.spec_tokens), ops.WIDE_ROWS))
        if self.is_cuda and cfg.gemm_tuning:  # room for prefill row padding (tuning buckets)
            from ..tuning import bucket_rows

            self.max_tokens = bucket_rows(self.max_tokens)
        self._alloc_kv()
        self.bm = BlockManager(self.num_blocks, self.block_size, cfg.enable_prefix_caching)
        # metadata buffers (max layout)
        self.max_layout = MetaLayout(self.max_tokens, self.max_seqs, self.bt_width,
                                     self.max_tokens, max(self.max_seqs, self.ws_rows),
                                     penalty=True, guide=True, score=self.max_tokens)
        pin = self.is_cuda
        # two pinned metadata buffers, used alternately: a step's H2D copy may still be queued
        # while the host packs the next step (async look-ahead decode, TP workers); an event
        # per buffer orders reuse behind the copy that last read it
        self.meta_hosts = [torch.zeros(self.max_layout.size, dtype=torch.int32, pin_memory=pin)
                           for _ in range(2)]
        self.meta_hosts_np = [h.numpy() for h in self.meta_hosts]
        self._mh = 0
        self._h2d_done = [torch.cuda.Event() if self.is_cuda else None for _ in range(2)]
        self.meta_dev = torch.zeros(self.max_layout.size, dtype=torch.int32, device=self.device)
        # sampled tokens of in-flight steps land here (D2H, one slot per in-flight step)
        self.tok_host = [torch.zeros(max(cfg.max_num_seqs, self.ws_rows, 256), dtype=torch.int64,
                                     pin_memory=pin) for _ in range(2)]
        self._tok_done = [torch.cuda.Event() if self.is_cuda else None for _ in range(2)]
        # logprobs of a step (SamplingParams.logprobs) ride the tokens' copy and event: one
        # pinned buffer per token slot, laid out like the device buffer ws["lp_out"] -
        # [lp: R | top ids: R x TOP_N (int32 bits) | top logprobs: R x TOP_N], R = lp_rows
        self.lp_rows = max(cfg.max_num_seqs, self.ws_rows, self.max_seqs)
        self.lp_host = [torch.zeros(self.lp_rows * (1 + 2 * TOP_N), dtype=torch.float32,
                                    pin_memory=pin) for _ in range(2)]
        # logprob arrays of the last execute() / verify()-free step: None, or (lp [n],
        # top ids [n, TOP_N] | None, top logprobs [n, TOP_N] | None) as numpy
        self.last_logprobs = None
        # prompt logprobs of the last execute() (SamplingParams.prompt_logprobs): None, or
        # (lp [rows], top ids [rows, TOP_N] | None, top logprobs | None) as numpy, one row per
        # entry of the step's ``score_rows_of`` list, in its order
        self.last_prompt_logprobs = None
        self.last_scored: list = []   # that step's ``score_rows_of`` list
        # the fused scorer's record workspace, allocated with the first scoring request
        # (ensure_score_state); None for an engine that saw none
        self.score_ws: dict | None = None
        self.score_fused = True  # False: every chunk materialises its logits (bench/scoring.py)
        self._score_dev = None   # (lp, top ids, top logprobs) of the step in flight
        # the prefill GEMM's error word as of the last prefill step (0: every wait succeeded)
        self._err_host = torch.zeros(1, dtype=torch.int32, pin_memory=pin)
        # OR of the words read since the last take_kernel_error() (the device word is cleared
        # on every read), and how many steps ever reported one
        self.kernel_error = 0
        self.kernel_error_steps = 0
        # the engine thread ORs words in, the HTTP loop's /health swaps them out
        self._kernel_error_lock = threading.Lock()
        self._last_collect = 0.0
        nkv = self.model.n_kv_heads
        self.part_out = torch.empty(self.max_seqs * nkv * alloc_parts * 16 * 128,
                                    dtype=torch.float32, device=self.device)
        self.part_lse = torch.empty(self.max_seqs * nkv * alloc_parts * 16,
                                    dtype=torch.float32, device=self.device)
        # fused decode-path workspace (q / attention / activation rows, sampler keys,
        # split-K partials and arrival counters for the decode attention kernel)
        H = self.mcfg.hidden_size
        dt, dev = self.dtype, self.device
        self.ws = {
            "q": torch.empty(self.ws_rows, self.model.n_heads, 128, dtype=dt, device=dev),
            "attn": torch.empty(self.ws_rows, self.model.n_heads, 128, dtype=dt, device=dev),
            "act": torch.empty(self.ws_rows, self.model.inter, dtype=dt, device=dev),
            "keys": torch.zeros(self.ws_rows * (self.model.vocab_shard // 16 + 1),
                                dtype=torch.int64, device=dev),
            "tokens": torch.zeros(self.ws_rows, dtype=torch.int64, device=dev),
            "tp_keys": torch.zeros(self.max_seqs, dtype=torch.int64, device=dev),
            "counters": torch.zeros(self.max_seqs * nkv, dtype=torch.int32, device=dev),
            "part_out": self.part_out, "part_lse": self.part_lse,
            "max_parts": self.max_parts, "part_tokens": self.part_tokens,
        }
        del H
        # logprob outputs (views of one buffer: one D2H copy moves them) and, where the fused
        # LM head + sampler can record them (one GPU), its per-tile record workspace next to
        # "keys": 16 B per key
        R = self.lp_rows
        lp_out = torch.zeros(R * (1 + 2 * TOP_N), dtype=torch.float32, device=dev)
        self.ws.update({
            "lp_out": lp_out, "lp": lp_out[:R],
            "top_ids": lp_out[R:R + R * TOP_N].view(torch.int32).view(R, TOP_N),
            "top_lp": lp_out[R + R * TOP_N:].view(R, TOP_N),
            "lp_ws": (torch.zeros(4 * self.ws["keys"].numel(), dtype=torch.float32, device=dev)
                      if self.is_cuda and self.tp_size == 1 else None),
        })
        # the fused decode attention combines <= 64 partitions in-kernel (<= 16k tokens at
        # 256-token partitions); longer contexts use the two-kernel split-K path
        self.fused_decode = bool(cfg.fused_decode) and self.max_parts <= 64
        self.model.fused_decode = self.fused_decode
        # keyed (batch bucket, partition bucket)
        self.graphs: dict[tuple, torch.cuda.CUDAGraph] = {}
        self.graph_io: dict[tuple, dict] = {}
        self.graph_pool = None
        self.steps = 0
        self.graph_steps = 0
        self.verify_steps = 0
        self.timing = {"graph_prep": 0.0, "graph_run": 0.0}
        self._verify_rows: int | None = None
        # sampling penalties (SamplingParams.penalised): device state allocated with the first
        # such request (ensure_penalty_state), one row ("slot") per penalised running sequence
        self.pen: dict | None = None
        self._pen_pool = SlotPool("penalty", cfg.max_num_seqs)
        self._pen_slot, self._pen_free = self._pen_pool.slots, self._pen_pool.free
        # guided decoding (SamplingParams.guided): device state allocated with the first such
        # request (ensure_guide_state) - the pool of automaton tables, one current state per
        # guided running sequence ("slot") - and the host's bookkeeping of both
        self.guide: dict | None = None
        self._guide_slot_pool = SlotPool("guide", cfg.max_num_seqs)
        self._guide_slots, self._guide_free = (self._guide_slot_pool.slots,
                                               self._guide_slot_pool.free)
        # guides with a range of pool rows, by Guide.key, least recently used first:
        # {"guide", "base", "refs" (sequences holding it), "uploaded"}
        self._guide_pool: "collections.OrderedDict[tuple, dict]" = collections.OrderedDict()
        self._guide_of: dict[int, tuple] = {}     # seq_id -> key of the guide it holds
        self._f32_logits: torch.Tensor | None = None

    # -- prompt logprobs ---------------------------------------------------------------------
    def ensure_score_state(self) -> None:
        """Allocate the fused scorer's workspace on first need - never inside a graph capture
        (the engine calls this when a scoring request is added), never for an engine without
        one: 16 B per (row, 16-column tile) of one ``LlamaModel.score_rows`` chunk."""
        if self.score_ws is not None:
            return
        m = self.model
        if not m.score_fusable(1):  # the CPU, TP shards: every chunk materialises its logits
            self.score_ws = {}
            return
        n = 4 * m.score_chunk_rows() * (self.mcfg.vocab_size // 16)
        print(f"[atta] prompt logprobs: scoring workspace {4 * n / 1e6:.1f} MB "
              f"({m.score_chunk_rows()} rows x {self.mcfg.vocab_size // 16} tiles x 16 B)",
              flush=True)
        self.score_ws = {"rec": torch.zeros(n, dtype=torch.float32, device=self.device)}

    @staticmethod
    def score_rows_of(batch: Batch) -> list:
        """The rows of a step that are scored: (sequence, prompt index it yields, row of the
        step).  The row at position p of a sequence that still owes prompt logprobs predicts
        prompt token p + 1; rows whose entry is already recorded (a prefill restarted after a
        preemption) and the last prompt row (it predicts the first generated token:
        ``logprobs``' business) are not scored."""
        out, row = [], 0
        for seq, s0, n in zip(batch.seqs, batch.q_start, batch.q_len):
            if seq.scoring:
                lo = max(s0 + 1, len(seq.prompt_logprobs))
                hi = min(s0 + n + 1, seq.num_prompt)
                out.extend((seq, i, row + i - 1 - s0) for i in range(lo, hi))
            row += n
        return out

    # -- sampling penalties ------------------------------------------------------------------
    def ensure_penalty_state(self) -> None:
        """Allocate the penalty state on first need - never inside a graph capture (the engine
        calls this when a penalised request is added), never for an engine without one:
        int32 [max_num_seqs, vocab] token words (bit 31: in the prompt, bits 0-30: times
        generated), the [max_num_seqs, 300] bias tables and the fp32 logits buffer the apply
        kernel writes and the sampler reads."""
        if self.pen is not None:
            return
        if self.tp_size > 1:
            raise ValueError("sampling penalties and logit_bias are not served under tensor "
                             "parallelism")
        n, V, dev = self.cfg.max_num_seqs, self.mcfg.vocab_size, self.device
        nb = ops.PENALTY_BIAS_ENTRIES
        self.pen = {
            "state": torch.zeros(n, V, dtype=torch.int32, device=dev),
            "bias_ids": torch.full((n, nb), -1, dtype=torch.int32, device=dev),
            "bias_vals": torch.zeros(n, nb, dtype=torch.float32, device=dev),
            "logits": self._sampler_logits(),
        }

    def _penalty_slot(self, seq) -> int:
        """The slot of a penalised sequence whose next token this step samples; a sequence
        without one (just admitted, or re-admitted after a preemption) gets a free slot, seeded
        on the current stream from its prompt and the tokens it has generated so far."""
        slot, fresh = self._pen_pool.acquire(seq.seq_id)
        if fresh:
            sp, pen = seq.sampling, self.pen
            bias = sp.logit_bias or {}
            ops.penalty_seed(pen["state"][slot], seq.prompt_ids, seq.output_ids,
                             pen["bias_ids"][slot], pen["bias_vals"][slot],
                             list(bias.keys()), [float(b) for b in bias.values()])
        return slot

    def penalty_release(self, seq_id: int) -> None:
        """Give a finished, aborted or preempted sequence's slot back (host bookkeeping only;
        nothing is launched).  The slot's device row is NOT touched here, and kernels already
        queued may still read or count into it - safe, because every step, every seed and every
        graph replay is ordered on one stream and the next owner's first use of the slot is its
        seed, which zeroes the row and rewrites the bias table:

        * a look-ahead step's update of a sequence that stopped on EOS one step earlier: step
          n + 1 was queued with the slot before the host saw step n's EOS; its apply reads and
          its update increments a row nobody owns any more, and its token is discarded by the
          engine.  Any seed of that slot is queued after step n + 1, so it zeroes the stray count.
        * a slot re-used by the next request: the new owner's seed is queued behind every step
          that carried the old owner, so those steps saw the old counts and the new owner's
          first apply sees exactly its seed.
        * an abort in flight: the same - the in-flight steps finish against the old row, their
          tokens are dropped (``_collect`` skips finished sequences), and the row is only handed
          on through a later seed.

        A preempted sequence comes back through ``_penalty_slot``, which re-seeds from its prompt
        and all its outputs so far, so its counts continue across the recompute."""
        self._pen_pool.release(seq_id)

    def _sampler_logits(self) -> torch.Tensor:
        """The fp32 logits buffer the penalty and the guide kernels write and the sampler
        reads: one allocation, shared by both features."""
        if self._f32_logits is None:
            self._f32_logits = torch.empty(self.max_seqs, self.mcfg.vocab_size,
                                           dtype=torch.float32, device=self.device)
        return self._f32_logits

    # -- guided decoding ---------------------------------------------------------------------
    def ensure_guide_state(self) -> None:
        """Allocate the guide state on first need - never inside a graph capture (the engine
        calls this when a guided request is added), never for an engine without one: the pool
        int16 [guided_pool_states, vocab] of automaton rows (row 0: the shared done state), the
        int32 [max_num_seqs] current states and the fp32 logits buffer."""
        if self.guide is not None:
            return
        if self.tp_size > 1:
            raise ValueError("guided decoding is not served under tensor parallelism")
        n, V, dev = self.cfg.max_num_seqs, self.mcfg.vocab_size, self.device
        P = int(self.cfg.guided_pool_states)
        if not 2 <= P <= 32767:
            raise ValueError(f"guided_pool_states must be in 2 .. 32767, got {P}")
        print(f"[atta] guided decoding: {P} pool states x {V} tokens, "
              f"{P * V * 2 / 1e9:.2f} GB of automaton rows", flush=True)
        self.guide = {
            # -1 everywhere: an entry nobody uploaded allows nothing and leads to done
            "next": torch.full((P, V), -1, dtype=torch.int16, device=dev),
            "state": torch.zeros(n, dtype=torch.int32, device=dev),
            "logits": self._sampler_logits(),
            "done_row": False,
        }

    def guide_reserve(self, seq_id: int, guide) -> None:
        """Give ``guide`` a range of pool rows (host bookkeeping: first fit over the gaps
        between the reserved ranges, whole guides no sequence holds evicted least recently
        used first) and count ``seq_id`` among its holders.  ``ValueError`` if the pool has no
        room.  Nothing is uploaded here: ``_guide_slot`` does that on the step stream."""
        self.ensure_guide_state()
        pool, P = self._guide_pool, self.guide["next"].shape[0]
        ent = pool.get(guide.key)
        if ent is None:
            need = guide.num_states
            while True:
                base = self._guide_fit(need, P)
                if base is not None:
                    break
                victim = next((k for k, e in pool.items() if e["refs"] == 0), None)
                if victim is None:
                    raise ValueError(f"no room for a guide of {need} states in the guide pool "
                                     f"({P - 1} states, guided_pool_states): every other guide "
                                     "is in use by a running request")
                del pool[victim]
            ent = pool[guide.key] = {"guide": guide, "base": base, "refs": 0, "uploaded": False}
        pool.move_to_end(guide.key)
        ent["refs"] += 1
        self._guide_of[seq_id] = guide.key

    def _guide_fit(self, need: int, P: int) -> int | None:
        at = 1  # row 0 is the done state
        for e in sorted(self._guide_pool.values(), key=lambda e: e["base"]):
            if e["base"] - at >= need:
                return at
            at = e["base"] + e["guide"].num_states
        return at if P - at >= need else None

    def _guide_slot(self, seq) -> int:
        """The slot of a guided sequence whose next token this step samples; a sequence without
        one (just admitted, or re-admitted after a preemption) gets a free slot, seeded on the
        current stream with the pool row of its host shadow state - so a recomputed sequence
        continues mid-pattern.  The guide's rows are uploaded here, on the same stream, the
        first time one of its sequences needs them."""
        slot, fresh = self._guide_slot_pool.acquire(seq.seq_id)
        if fresh:
            ent = self._guide_pool[self._guide_of[seq.seq_id]]
            g, base, dev = ent["guide"], ent["base"], self.guide
            if not dev["done_row"]:   # row 0 is the same in every guide's table
                dev["next"][0].copy_(torch.from_numpy(g.next[0]))
                dev["done_row"] = True
            if not ent["uploaded"]:
                # local rows 1 .. n -> pool rows base .. base + n - 1; 0 (done) and -1 stay
                t = g.next[1:]
                rows = torch.from_numpy(np.where(t > 0, t + np.int16(base - 1), t))
                dev["next"][base:base + g.num_states].copy_(rows)
                ent["uploaded"] = True
            st = int(seq.guide_state)
            ops.guide_seed(dev["state"], slot, st + base - 1 if st > 0 else 0)
        return slot

    def guide_release(self, seq_id: int, keep_guide: bool = False) -> None:
        """Give a finished, aborted or preempted sequence's slot back, and (unless
        ``keep_guide``: a preempted sequence comes back) drop its hold on its guide's pool rows
        (host bookkeeping only; nothing is launched).  Neither the slot's state word nor the
        pool rows are touched here, and kernels already queued may still read them - safe, by
        the stream-order argument of ``penalty_release``: every step, every seed, every upload
        and every graph replay is ordered on one stream, so

        * a look-ahead step queued behind an end token reads the slot's state (0, done: the
          step before advanced it there), masks its row to the end tokens and advances 0 -> 0;
          its token is discarded by the engine.  A look-ahead step of a sequence cut by length
          or aborted advances a state nobody owns any more;
        * the next owner's first use of a slot is its seed, queued behind every step that
          carried the old owner: those steps saw the old state, the new owner's first apply
          sees exactly its seed;
        * rows of an evicted guide are rewritten by the next guide's upload, queued behind
          every step of the sequences that held the old one (it had no holder left, so no later
          step reads them); until then nothing refers to them.

        A preempted sequence comes back through ``_guide_slot``, which seeds its slot from the
        host shadow state (``Sequence.guide_state``, advanced with every appended token)."""
        self._guide_slot_pool.release(seq_id)
        if not keep_guide:
            key = self._guide_of.pop(seq_id, None)
            if key is not None:
                self._guide_pool[key]["refs"] -= 1

    def _room_for_decode_copies(self) -> bool:
        """The pre-shuffled decode copies double the 16-bit weights (16 GB for Llama-3.1-8B);
        Llama-3-70B bf16 on ONE GPU (141 GB) cannot afford a second copy next to its KV cache,
        so it decodes from the row-major weights instead."""
        need = self.model.decode_copy_bytes()
        torch.cuda.synchronize(self.device)
        free, total = torch.cuda.mem_get_info(self.device)
        keep = max(int(0.15 * total), 24 << 30)  # KV cache + activations + graphs
        ok = int(need <= free - keep)
        if self.comm is not None and self.comm.size > 1:
            # every TP rank must pick the same GEMV layout (ranks sharing a GPU, or loading at
            # different times, see different free memory): the group decides by MIN
            ok = self.comm.min_int(ok, self.device)
        if not ok:
            print(f"[atta] skipping pre-shuffled decode weights: {need / 2**30:.1f} GiB needed, "
                  f"{free / 2**30:.1f} GiB free (row-major decode GEMVs)", flush=True)
            return False
        return True

    # ------------------------------------------------------------------------------------
    def _alloc_kv(self):
        m = self.model
        L = self.mcfg.num_layers
        per_block = 2 * L * m.n_kv_heads * self.block_size * m.head_dim * self.dtype.itemsize
        if self.cfg.num_kv_blocks > 0:
            nb = self.cfg.num_kv_blocks
        elif self.is_cuda:
            torch.cuda.synchronize()
            free, total = torch.cuda.mem_get_info(self.device)
            used = total - free
            # activation / workspace reserve: logits + GEMM intermediates at the token budget
            T = self.cfg.max_num_batched_tokens
            act = T * (self.mcfg.hidden_size * 8 + (m.inter * 2 + m.qkv_width) * 2) * 2
            act += self.max_seqs_estimate() * self.mcfg.vocab_size * 4 * 2 + (2 << 30)
            budget = total * self.cfg.gpu_memory_utilization - used - act
            if self.cfg.tp_same_device and self.tp_size > 1:
                # every rank shares this one device (the one-GPU TP rehearsal): each gets its
                # share of the budget, charged for its own allocations only (the ranks probe
                # free memory at different moments)
                mine = torch.cuda.memory_reserved(self.device)
                budget = total * self.cfg.gpu_memory_utilization / self.tp_size - mine - act
            nb = int(budget // per_block)
        else:
            nb = int(os.environ.get("ATTA_CPU_KV_BLOCKS", "256"))
        nb = max(nb, 2 * self.bt_width)
        if self.comm is not None:  # TP ranks must agree on the page count
            nb = self.comm.min_int(nb, self.device)
        self.num_blocks = nb
        shape_k = (L, nb, m.n_kv_heads, self.block_size, m.head_dim)
        shape_v = (L, nb, m.n_kv_heads, m.head_dim, self.block_size)
        # zero-init (tidy, not required: the attention kernels zero the V of every key past a
        # sequence's end before P.V, so stale or non-finite bytes there are harmless)
        self.k_cache = torch.zeros(shape_k, dtype=self.dtype, device=self.device)
        self.v_cache = torch.zeros(shape_v, dtype=self.dtype, device=self.device)
        self.k_layers = [self.k_cache[i] for i in range(L)]
        self.v_layers = [self.v_cache[i] for i in range(L)]
        self.kv_bytes = per_block * nb

    def max_seqs_estimate(self) -> int:
        return max(self.cfg.max_num_seqs, 16)

    @property
    def kv_total_tokens(self) -> int:
        return self.num_blocks * self.block_size

    # ------------------------------------------------------------------------------------
    def _tier(self, batch_size: int) -> tuple:
        """(partition tokens, max partitions, graph partition buckets) of a decode step of
        ``batch_size`` rows (the graph bucket when replayed)."""
        for mb, pt, mp, bk in self.part_tiers:
            if 0 < batch_size <= mb:
                return pt, mp, bk
        return self.part_tokens, self.max_parts, self.parts_buckets

    def _ws_for(self, batch_size: int) -> dict:
        pt, mp, _ = self._tier(batch_size)
        if pt == self.part_tokens:
            return self.ws
        return {**self.ws, "part_tokens": pt, "max_parts": mp}

    def _prepare(self, batch: Batch, pad_seqs: int = 0, tiles: bool = True):
        ids, qs, ql = batch.arrays()
        pad_tokens = 0
        if tiles and self.gemm_table is not None and batch.num_decode < len(batch.seqs):
            from ..tuning import bucket_rows

            rows = int(np.sum(ql))
            # steps the fused small-prefill path takes (<= SKINNY_MAX_M rows) stay unpadded:
            # its GEMVs read every row of x per weight tile (17 rows padded to 32 doubled
            # gate_up: 80 vs ~40 us)
            if self.model.step_plan(rows).pad_rows:
                pad_tokens = bucket_rows(rows)
        d = self.bm.build_batch(ids, qs, ql, self.bt_width,
                                self.tile_tokens if tiles else 0, batch.num_decode, pad_tokens,
                                pad_seqs)
        T = d["positions"].shape[0]
        S = d["seq_kvlen"].shape[0]
        NT = d["tile_seq"].shape[0]
        penalty = self._penalised(batch)
        guide = self._guided(batch)
        scored = self.last_scored = self.score_rows_of(batch)
        lay = MetaLayout(T, S, self.bt_width, NT, penalty=penalty, guide=guide,
                         score=len(scored))
        input_ids = np.zeros(T, dtype=np.int32)
        row = 0
        temps = np.zeros(S, dtype=np.float32)
        top_p = np.ones(S, dtype=np.float32)
        top_k = np.zeros(S, dtype=np.int32)
        seeds = np.zeros(S, dtype=np.int64)
        steps = np.zeros(S, dtype=np.int64)
        for i, (seq, s0, n) in enumerate(zip(batch.seqs, batch.q_start, batch.q_len)):
            input_ids[row:row + n] = seq.token_array()[s0:s0 + n]
            row += n
            temps[i] = seq.sampling.temperature
            top_p[i] = seq.sampling.top_p
            top_k[i] = seq.sampling.top_k
            seeds[i] = seq.seed
            steps[i] = len(seq.output_ids)
        arrays = dict(d)
        arrays.update(input_ids=input_ids, temperature=temps, top_p=top_p, top_k=top_k,
                      seeds=seeds, steps=steps, feed_prev=np.zeros(1, dtype=np.int32))
        if penalty:
            # per sampled row: the sequence's slot - only where this step samples its next
            # token (a chunk short of the prompt's end has its sample dropped: no slot, no
            # count); unpenalised and padded rows carry -1 and are copied through
            self.ensure_penalty_state()
            slot = np.full(S, -1, dtype=np.int32)
            rep = np.ones(S, dtype=np.float32)
            freq = np.zeros(S, dtype=np.float32)
            pres = np.zeros(S, dtype=np.float32)
            for i, (seq, s0, n) in enumerate(zip(batch.seqs, batch.q_start, batch.q_len)):
                sp = seq.sampling
                if sp.penalised and s0 + n == seq.num_tokens:
                    slot[i] = self._penalty_slot(seq)
                    rep[i] = sp.repetition_penalty
                    freq[i] = sp.frequency_penalty
                    pres[i] = sp.presence_penalty
            arrays.update(pen_slot=slot, pen_rep=rep, pen_freq=freq, pen_pres=pres)
        if guide:
            # per sampled row: the sequence's slot, only where this step samples its next token
            # (as above); unguided and padded rows carry -1 and are copied through
            slot = np.full(S, -1, dtype=np.int32)
            for i, (seq, s0, n) in enumerate(zip(batch.seqs, batch.q_start, batch.q_len)):
                if seq.guide is not None and s0 + n == seq.num_tokens:
                    slot[i] = self._guide_slot(seq)
            arrays.update(guide_slot=slot)
        if scored:
            self.ensure_score_state()
            arrays.update(
                score_idx=np.fromiter((r for _, _, r in scored), dtype=np.int64,
                                      count=len(scored)),
                score_tgt=np.fromiter((s.prompt_ids[i] for s, i, _ in scored), dtype=np.int32,
                                      count=len(scored)))
        return lay, arrays

    @property
    def meta_host(self) -> torch.Tensor:
        return self.meta_hosts[self._mh]

    @property
    def meta_host_np(self) -> np.ndarray:
        return self.meta_hosts_np[self._mh]

    def _next_meta_host(self) -> np.ndarray:
        """Switch to the other pinned metadata buffer (waiting for the H2D copy that last
        read it) and return its numpy view."""
        self._mh ^= 1
        ev = self._h2d_done[self._mh]
        if ev is not None:
            ev.synchronize()
        return self.meta_hosts_np[self._mh]

    def _h2d(self, dst: torch.Tensor, size: int):
        dst.copy_(self.meta_host[:size], non_blocking=True)
        ev = self._h2d_done[self._mh]
        if ev is not None:
            ev.record()

    def _pack(self, lay: MetaLayout, arrays: dict) -> np.ndarray:
        host = self._next_meta_host()[:lay.size]
        lay.pack(host, arrays)
        return host

    def _meta(self, v: dict, num_decode: int, num_tiles: int) -> AttnMeta:
        return AttnMeta(positions=v["positions"], slot_mapping=v["slot_mapping"],
                        block_tables=v["block_tables"], seq_kvlen=v["seq_kvlen"],
                        seq_qstart=v["seq_qstart"], tile_seq=v["tile_seq"],
                        tile_qoff=v["tile_qoff"], logits_idx=v["logits_idx"],
                        num_decode=num_decode, num_tiles=num_tiles)

    def parts_bucket(self, max_kv: int, batch_size: int = 0) -> int:
        """Smallest partition bucket covering a decode step of ``batch_size`` rows whose
        longest context is max_kv (in the partition size that batch size uses)."""
        pt, top, buckets = self._tier(batch_size)
        need = max(1, math.ceil(max_kv / pt))
        return next((p for p in buckets if p >= need), top)

    def _sample_args(self, v: dict, variant: int = 0) -> SampleArgs:
        """A step's sampling fields bound to its decoded variant (``sample_plan``)."""
        plan = sample_plan(variant, self.tp_size)
        # penalty variant: the materialised logits go through ops.penalty_apply into the fp32
        # buffer, the sampler reads that, ops.penalty_update counts its tokens (logprobs stay
        # on the raw logits)
        pen = None
        if plan.penalty:
            pen = {**self.pen, "slot": v["pen_slot"], "rep": v["pen_rep"],
                   "freq": v["pen_freq"], "pres": v["pen_pres"]}
        # guide variant: ops.guide_apply masks the (penalised) logits by each row's automaton
        # state, ops.guide_advance moves the state by the sampled token
        gd = {**self.guide, "slot": v["guide_slot"]} if plan.guide else None
        return SampleArgs(v["temperature"], v["seeds"], v["steps"],
                          v["top_p"] if plan.topkp else None, v["top_k"], plan, pen, gd)

    def _forward_sample(self, v: dict, md: AttnMeta, num_parts: int, variant: int = 0,
                        score_top: int = 0):
        """One step's forward + sampling.  ``variant`` (variant_code): bit 0 - some row uses
        top-p / top-k (logits are materialised and the top-k / top-p kernel samples every
        row); bits 1-2 - the step's logprob mode, whose results land in ws["lp"] (and
        ws["top_ids"] / ws["top_lp"]), one row per sampled row; bit 3 - some sequence is
        penalised (logits materialised, ``LlamaModel.sample_logits``' penalty tail); bit 4 - some
        sequence is guided (logits materialised, its guide tail); bit 5 - the rows
        v["score_idx"] are scored against v["score_tgt"] (``LlamaModel.score_rows`` with
        ``score_top`` alternatives) in launches of their own after the sampler's; the sampled
        rows see exactly what they see without it."""
        m = self.model
        T = v["input_ids"].shape[0]
        args = self._sample_args(v, variant)
        score = args.plan.score
        if (self.fused_decode and md.num_tiles == 0 and not score
                and md.num_decode == T and m.decode_step_fusable(T)):
            ws = self._ws_for(T)
            # grid over this step's partition bucket only (num_parts covers every row, in
            # the partition size of this batch size: parts_bucket)
            ws = {**ws, "max_parts": min(num_parts, ws["max_parts"])}
            return m.forward_decode(v["input_ids"], md, self.k_layers, self.v_layers, ws, args,
                                    prev_tokens=self.ws["tokens"], feed_prev=v["feed_prev"])
        decode_only = md.num_tiles == 0 and md.num_decode == T
        # final norm on the sampled rows only (each sequence's last token)
        last = m.forward(v["input_ids"], md, self.k_layers, self.v_layers, self.part_out,
                         self.part_lse, num_parts, self.part_tokens,
                         prev_tokens=self.ws["tokens"] if decode_only else None,
                         feed_prev=v["feed_prev"] if decode_only else None,
                         rows=(torch.cat([v["logits_idx"], v["score_idx"]]) if score
                               else v["logits_idx"]))
        # one gather and one final norm for both kinds of row: the first rows go to the
        # sampler as ever, the rest are scored
        n = v["logits_idx"].shape[0]
        last, scored = last[:n], last[n:]
        # decode-only steps sample straight into ws["tokens"]: a graph replay (and the next
        # look-ahead step's embed) reads the samples from there, so the captured sampler must
        # write them there too (a fresh tensor would leave the previous step's tokens behind)
        toks = m.sample_tail(last, 0.0, args, self.ws,
                             out=self.ws["tokens"][:n] if decode_only else None,
                             fused_ok=m.sampler_fusable(n) and n <= self.max_seqs)
        if score:
            self._score_dev = m.score_rows(scored, v["score_tgt"], score_top,
                                           self.score_ws or None, fused=self.score_fused)
        return toks

    # ------------------------------------------------------------------------------------
    def _graph_ok(self, bucket: int, variant: int = 0) -> bool:
        """Can a decode step of this bucket be captured?  Every collective inside it must be
        device-side: RCCL, or - on a gloo control group (TP ranks rehearsing on one GPU) - the
        IPC kernels, which carry the fused decode step's X1/X2 sums and X4 key MAX but not the
        logits all-gather of the top-k / top-p sampler, of a logprob variant (every one
        materialises its logits under TP) or of buckets past the fused path."""
        c = self.comm
        if c is None or c.size == 1 or not c.is_gloo:
            return True
        return (c.decode_capturable and variant == 0 and self.fused_decode
                and self.model.decode_step_fusable(bucket))

    def graph_bucket(self, batch: Batch) -> int:
        """Graph bucket a decode-only batch replays from (0: eager step)."""
        n = len(batch.seqs)
        if not (self.is_cuda and self.cfg.use_graphs and batch.num_decode == n and n > 0
                and self.graph_sizes and n <= self.graph_sizes[-1]):
            return 0
        b = next(b for b in self.graph_sizes if b >= n)
        if any(s.scoring for s in batch.seqs) and self.score_rows_of(batch):
            return 0  # (a one-token chunk of a prompt that is being scored)
        return b if self._graph_ok(b, self._variant(batch)) else 0

    @staticmethod
    def _special(batch: Batch) -> bool:
        return any(s.sampling.top_p < 1.0 or s.sampling.top_k > 0 for s in batch.seqs)

    @staticmethod
    def _lp_mode(batch: Batch) -> int:
        """Logprob mode of a step: that of its most demanding sequence (the others' results
        are dropped by the engine)."""
        want = [s.sampling.logprobs for s in batch.seqs if s.sampling.logprobs is not None]
        if not want:
            return LP_NONE
        return LP_TOPN if max(want) > 0 else LP_SAMPLED

    @staticmethod
    def _penalised(batch: Batch) -> bool:
        return any(s.sampling.penalised for s in batch.seqs)

    @staticmethod
    def _guided(batch: Batch) -> bool:
        return any(s.guide is not None for s in batch.seqs)

    @classmethod
    def _variant(cls, batch: Batch) -> int:
        return variant_code(cls._special(batch), cls._lp_mode(batch), cls._penalised(batch),
                            cls._guided(batch))

    def _fetch_logprobs(self, variant: int, n: int):
        """Synchronous copy of a step's logprob arrays (eager steps, after the tokens')."""
        mode = variant_lp(variant)
        if mode == LP_NONE:
            return None
        lp = self.ws["lp"][:n].cpu().numpy()
        if mode != LP_TOPN:
            return lp, None, None
        return lp, self.ws["top_ids"][:n].cpu().numpy(), self.ws["top_lp"][:n].cpu().numpy()

    def _fetch_prompt_logprobs(self):
        """Synchronous copy of a scoring step's arrays, after the tokens' (None: no scoring)."""
        dev, self._score_dev = self._score_dev, None
        if dev is None:
            return None
        return tuple(None if t is None else t.cpu().numpy() for t in dev)

    def execute(self, batch: Batch) -> np.ndarray:
        """Run one step; returns sampled token ids (one per sequence in batch order).  A
        step in which a sequence asked for logprobs leaves them in ``last_logprobs``."""
        n = len(batch.seqs)
        bucket = self.graph_bucket(batch)
        if bucket:
            h = self.launch(batch)
            toks = self.collect(h)
            self.last_logprobs = self.collect_logprobs(h)
            self.last_prompt_logprobs = None
            return toks
        self.steps += 1
        variant = self._variant(batch)
        lay, arrays = self._prepare(batch)
        topn = False
        if lay.score:
            variant |= V_SCORE
            topn = any(s.sampling.prompt_logprobs for s in batch.seqs if s.scoring)
        max_kv = int(arrays["seq_kvlen"][:batch.num_decode].max()) if batch.num_decode else 0
        if batch.num_decode == n and lay.NT == 0:
            # decode-only: in the partition size of this batch size (>= the 256-token count
            # the unfused path needs, within the allocated partials)
            num_parts = self.parts_bucket(max_kv, n)
        else:
            num_parts = max(1, math.ceil(max_kv / self.part_tokens))
        host = self._pack(lay, arrays)
        hdr = StepHeader(OP_STEP, lay.T, lay.S, lay.W, lay.NT, batch.num_decode, num_parts, 0,
                         variant, n, lay.size, score_rows=lay.score, score_topn=topn)
        self._publish(hdr, host)
        toks = self._run(hdr)
        if self.is_cuda and lay.T > n and self.model.prefill_gemm != "hipblaslt":
            # prefill rows ran: fetch the hand-written GEMM's error word with the tokens'
            # own sync (a cross-workgroup wait that timed out - outputs are still exact, the
            # workgroup recomputed; it signals a GPU shared with other work) - ADVICE r3
            self._err_host.zero_()
            ops.prefill_gemm_error_to(self._err_host, clear=True)
        out = toks[:n].cpu().numpy()
        self.last_logprobs = self._fetch_logprobs(variant, n)
        self.last_prompt_logprobs = self._fetch_prompt_logprobs()
        word = int(self._err_host[0]) if self.is_cuda else 0
        if word:
            self._err_host.zero_()
            with self._kernel_error_lock:
                self.kernel_error |= word
                self.kernel_error_steps += 1
            print(f"[model_runner] prefill GEMM error word {word:#x}: a "
                  "cross-workgroup wait timed out (tiles recomputed, outputs exact; the GPU "
                  "is shared or oversubscribed)", flush=True)
        return out

    # -- speculative decoding: verify steps --------------------------------------------------
    def verify_rows(self) -> int:
        """Most rows (sequences + drafts) one verify step takes; 0: this runner cannot verify.
        On the GPU that is the largest row count the fused decode step runs (<= 128 rows on
        pre-shuffled 16-bit weights, <= 32 on fp8 and mxfp4, <= 128 on mxfp4 weights-only with a
        pre-shuffled LM head) inside the workspace; the CPU backend runs
        verify steps through the reference ops."""
        if self._verify_rows is None:
            rows = 0
            if self.spec_tokens > 0 and self.tp_size == 1:
                rows = self.ws_rows
                if self.is_cuda:
                    ok = self.fused_decode and self.model.g in ops.MQ_GROUPS
                    while ok and rows > 1 and not self.model.decode_step_fusable(rows):
                        rows -= 1
                    if self.model.quant == "mxfp4":  # verify steps stream the 4-bit copies
                        rows = min(rows, ops.fused_max_rows(mxfp4=True,
                                                            wide_w4=self.model.w4_only))
                    rows = rows if ok and rows > 1 else 0
            self._verify_rows = rows
        return self._verify_rows

    def _verify_tier(self, batch_size: int) -> tuple:
        """(partition tokens, partitions allocated) of a verify step of ``batch_size``
        sequences: the decode tier of that batch size where the multi-query kernel has its
        shape, else 256-token partitions."""
        pt, mp, _ = self._tier(batch_size)
        if pt not in ops.MQ_PART_TOKENS:
            pt = 256
            mp = min(64, max(1, math.ceil(self.cfg.max_model_len / pt)))
        return pt, mp

    def verify_max_kv(self, batch_size: int) -> int:
        """Longest context (drafts included) a sequence of such a verify step may have."""
        pt, mp = self._verify_tier(batch_size)
        return pt * mp

    def verify(self, batch: Batch, drafts: list) -> list:
        """One verify step over a decode-only batch: sequence i's rows are its pending token
        and ``drafts[i]`` (``batch.q_len[i] == 1 + len(drafts[i])``, KV room ensured by the
        caller), every row is sampled with step = len(output_ids) + row.  Returns the samples
        per sequence.  Runs eagerly (no graph, no look-ahead)."""
        S = len(batch.seqs)
        if not (0 < S == batch.num_decode and self.verify_rows() >= batch.num_tokens):
            raise ValueError("verify() needs a decode-only batch within verify_rows()")
        if self.is_cuda and self._special(batch):
            raise ValueError("verify(): top-k / top-p rows take no drafts")
        self.steps += 1
        self.verify_steps += 1
        ids, qs, ql = batch.arrays()
        d = self.bm.build_batch(ids, qs, ql, self.bt_width, 0, S, 0, 0)
        T = d["positions"].shape[0]
        lay = MetaLayout(T, S, self.bt_width, 0, T)
        input_ids = np.zeros(T, dtype=np.int32)
        temps = np.zeros(T, dtype=np.float32)
        seeds = np.zeros(T, dtype=np.int64)
        steps = np.zeros(T, dtype=np.int64)
        row = 0
        for seq, s0, n, dr in zip(batch.seqs, batch.q_start, batch.q_len, drafts):
            assert n == 1 + len(dr) and s0 == seq.num_tokens - 1
            input_ids[row] = seq.token_array()[s0]
            input_ids[row + 1:row + n] = dr
            temps[row:row + n] = seq.sampling.temperature
            seeds[row:row + n] = seq.seed
            steps[row:row + n] = len(seq.output_ids) + np.arange(n)
            row += n
        arrays = dict(d)
        arrays.update(input_ids=input_ids, temperature=temps, top_p=np.ones(T, dtype=np.float32),
                      top_k=np.zeros(T, dtype=np.int32), seeds=seeds, steps=steps,
                      logits_idx=np.arange(T, dtype=np.int64),
                      feed_prev=np.zeros(1, dtype=np.int32))
        pt, mp = self._verify_tier(S)
        num_parts = max(1, math.ceil(int(arrays["seq_kvlen"].max()) / pt))
        if num_parts > mp:
            raise ValueError("verify(): context past verify_max_kv()")
        self._pack(lay, arrays)
        hdr = StepHeader(OP_STEP, lay.T, lay.S, lay.W, 0, S, num_parts, 0, 0, S, lay.size,
                         max_qlen=int(max(batch.q_len)), min_qlen=int(min(batch.q_len)))
        toks = self._run(hdr)[:T].cpu().numpy()
        out, row = [], 0
        for n in batch.q_len:
            out.append(toks[row:row + n])
            row += n
        return out

    def _forward_verify(self, v: dict, md: AttnMeta, num_parts: int, max_qlen: int,
                        min_qlen: int):
        m = self.model
        T = v["input_ids"].shape[0]
        if self.is_cuda:
            # the fused decode step or nothing: no fall-back to another path on the GPU
            if not (self.fused_decode and m.decode_step_fusable(T)):
                raise RuntimeError(f"verify step of {T} rows: fused decode path unavailable")
            pt, _ = self._verify_tier(md.num_decode)
            ws = {**self.ws, "part_tokens": pt, "max_parts": num_parts}
            return m.forward_decode(v["input_ids"], md, self.k_layers, self.v_layers, ws,
                                    self._sample_args(v), max_qlen=max_qlen, min_qlen=min_qlen)
        hidden = m.forward(v["input_ids"], md, self.k_layers, self.v_layers, self.part_out,
                           self.part_lse, num_parts, self.part_tokens)
        return m.sample_tail(hidden, 0.0, self._sample_args(v), self.ws, fused_ok=False)

    def take_kernel_error(self) -> int:
        """Error words seen since the previous call (the /health check), then cleared."""
        with self._kernel_error_lock:
            w, self.kernel_error = self.kernel_error, 0
        return w

    def launchable(self, batch: Batch) -> bool:
        """Decode-only batches can be launched asynchronously (every sampler runs on the
        device and leaves its tokens in ws["tokens"])."""
        n = len(batch.seqs)
        if any(s.scoring for s in batch.seqs) and self.score_rows_of(batch):
            return False  # a scoring step runs through execute(), which fetches its results
        return 0 < n <= self.max_seqs and batch.num_decode == n

    def launch(self, batch: Batch, lookahead: bool = False) -> dict:
        """Enqueue one decode-only step (graph replay when a bucket fits, else eager) and its
        token D2H copy; returns a handle for ``collect``.  ``lookahead``: the batch continues
        the previous launch row for row and its input tokens are that step's device samples
        (``ws["tokens"]``, not yet seen by the host), so the host never waits between steps
        (async look-ahead decode)."""
        if not self.launchable(batch):
            raise ValueError("launch() needs a decode-only batch")
        n = len(batch.seqs)
        bucket = self.graph_bucket(batch)
        variant = self._variant(batch)
        self.steps += 1
        t0 = time.perf_counter()
        if bucket:
            lay, arrays = self._prepare(batch, pad_seqs=bucket, tiles=False)
            num_parts = self.parts_bucket(int(arrays["seq_kvlen"][:n].max()), bucket)
            if (bucket, num_parts, variant) not in self.graphs:
                self.capture(bucket, num_parts, variant)
                t0 = time.perf_counter()
            assert lay.size == self.graph_io[(bucket, num_parts, variant)]["layout"].size
        else:
            lay, arrays = self._prepare(batch, tiles=False)
            num_parts = self.parts_bucket(int(arrays["seq_kvlen"][:n].max()), n)
        arrays["feed_prev"] = np.array([1 if lookahead else 0], dtype=np.int32)
        host = self._pack(lay, arrays)
        hdr = StepHeader(OP_STEP, lay.T, lay.S, lay.W, lay.NT, batch.num_decode, num_parts,
                         bucket, variant, n, lay.size)
        self._publish(hdr, host)
        t1 = time.perf_counter()
        self._run(hdr)
        dev_toks = self.ws["tokens"]  # _run leaves decode samples here (graph or eager)
        slot = self._mh  # one token slot per metadata buffer: same reuse distance
        ev = self._tok_done[slot]
        if ev is not None:
            ev.synchronize()
        self.tok_host[slot][:n].copy_(dev_toks[:n], non_blocking=self.is_cuda)
        lp_mode = variant_lp(variant)
        if lp_mode != LP_NONE:
            # the logprobs ride the same event: the sampled tokens' alone are the head of the
            # buffer, a top-N step moves all of it
            k = n if lp_mode == LP_SAMPLED else self.lp_host[slot].numel()
            self.lp_host[slot][:k].copy_(self.ws["lp_out"][:k], non_blocking=self.is_cuda)
        if ev is not None:
            ev.record()
        if bucket:
            self.timing["graph_prep"] += t1 - t0
        return {"n": n, "slot": slot, "t_launch": t1, "graph": bool(bucket), "lp_mode": lp_mode}

    def collect(self, h: dict) -> np.ndarray:
        """Wait for a launched step's tokens."""
        ev = self._tok_done[h["slot"]]
        if ev is not None:
            ev.synchronize()
        now = time.perf_counter()
        if h["graph"]:
            # pipelined steps overlap: charge each step from the later of its launch and the
            # previous collect, so graph_run / graph_steps stays the per-step wall time
            self.timing["graph_run"] += now - max(h["t_launch"], self._last_collect)
        self._last_collect = now
        return self.tok_host[h["slot"]][:h["n"]].numpy().copy()

    def collect_logprobs(self, h: dict):
        """Logprob arrays of a collected step (call after ``collect``): None, or (lp [n], top
        ids [n, TOP_N] | None, top logprobs [n, TOP_N] | None) - row i belongs to token i."""
        mode, n, R = h.get("lp_mode", LP_NONE), h["n"], self.lp_rows
        if mode == LP_NONE:
            return None
        host = self.lp_host[h["slot"]].numpy()
        lp = host[:n].copy()
        if mode != LP_TOPN:
            return lp, None, None
        ids = host[R:R + R * TOP_N].view(np.int32).reshape(R, TOP_N)[:n].copy()
        return lp, ids, host[R + R * TOP_N:].reshape(R, TOP_N)[:n].copy()

    def _publish(self, hdr: StepHeader, payload: np.ndarray | None = None) -> None:
        """Rank 0 of a TP group: send the workers a message (a step's with its metadata)."""
        if self.publisher is not None:
            w = hdr.words()
            self.publisher.publish(w if payload is None else np.concatenate([w, payload]))

    def _run(self, hdr: StepHeader):
        """Execute one step from its header; the packed metadata is in ``meta_host``."""
        T, NT, num_decode, size = hdr.T, hdr.NT, hdr.num_decode, hdr.size
        if hdr.max_qlen:  # verify step: row-sized sampling fields, multi-query attention
            lay = MetaLayout(T, hdr.S, hdr.W, NT, T)
            dev = self.meta_dev[:size]
            self._h2d(dev, size)
            v = lay.views(dev)
            return self._forward_verify(v, self._meta(v, num_decode, NT), hdr.num_parts,
                                        hdr.max_qlen, hdr.min_qlen)
        if hdr.bucket:
            key = (hdr.bucket, hdr.num_parts, hdr.variant)
            io = self.graph_io[key]
            self._h2d(io["dev"], size)
            self.graphs[key].replay()
            self.graph_steps += 1
            return io["out"]
        lay = MetaLayout(T, hdr.S, hdr.W, NT, penalty=bool(hdr.variant & V_PENALTY),
                         guide=bool(hdr.variant & V_GUIDE), score=hdr.score_rows)
        dev = self.meta_dev[:size]
        self._h2d(dev, size)
        v = lay.views(dev)
        md = self._meta(v, num_decode, NT)
        # every rank samples (deterministic kernels over all-gathered logits under TP)
        out = self._forward_sample(v, md, hdr.num_parts, hdr.variant,
                                   TOP_N if hdr.score_topn else 0)
        if NT == 0 and num_decode == T and out is not None:
            # every rank keeps the decode samples where a look-ahead step embeds them from
            dev_toks = self.ws["tokens"]
            if out.data_ptr() != dev_toks.data_ptr():
                dev_toks[:T].copy_(out[:T])
        return out

    # -- TP worker side ------------------------------------------------------------------
    def serve_worker(self, channel, reader: int) -> None:
        """TP rank > 0: replay rank 0's steps until it publishes OP_STOP / closes.

        Liveness: the worker registers its pid on the channel (rank 0 fails its next publish
        naming a dead worker) and waits in 1 s slices, raising when rank 0's process is gone
        so an orphaned worker exits instead of holding its GPU forever."""
        last = 0
        if hasattr(channel, "register_reader"):
            channel.register_reader(reader)
        while True:
            msg = channel.receive(reader, last, 1.0)
            if msg is None:
                if channel.closed:
                    return
                if not getattr(channel, "writer_alive", True):
                    raise RuntimeError(f"TP rank {reader + 1}: rank 0 died; worker exiting")
                continue
            last, data = msg
            hdr = StepHeader.parse(data)
            if hdr.op == OP_STOP:
                return
            if hdr.op == OP_CAPTURE:
                self.capture(hdr.bucket, hdr.num_parts or None, hdr.variant)
                continue
            if hdr.op == OP_BARRIER:
                if self.is_cuda:
                    torch.cuda.synchronize(self.device)
                self.comm.barrier()
                continue
            size = hdr.size
            # alternate pinned buffers: no stream sync per step, only an event wait on the
            # copy two steps back before its buffer is rewritten
            self._next_meta_host()[:size] = data[HDR_WORDS:HDR_WORDS + size]
            self._run(hdr)
            self.steps += 1

    def barrier(self):
        """Synchronise every TP rank (device work drained, then a process-group barrier)."""
        if self.is_cuda:
            torch.cuda.synchronize(self.device)
        self._publish(StepHeader(OP_BARRIER))
        if self.comm is not None:
            self.comm.barrier()

    def stop_workers(self):
        if self.publisher is not None:
            try:
                self.publisher.publish(StepHeader(OP_STOP).words(), 30.0)
            finally:
                self.publisher.close()

    # ------------------------------------------------------------------------------------
    def capture(self, bucket: int, parts: int | None = None, variant: int = 0):
        """Capture a decode step for `bucket` sequences whose contexts fit `parts` attention
        partitions (default: max_model_len) into a hipGraph; ``variant`` (variant_code): the
        top-k / top-p sampler (logits materialised), a logprob mode, the penalty and / or the guide
        tail.
        Variants other than 0 are captured on first use."""
        variant = int(variant)
        parts = parts or self._tier(bucket)[1]
        self._publish(StepHeader(OP_CAPTURE, bucket=bucket, num_parts=parts, variant=variant))
        penalty = bool(variant & V_PENALTY)
        if penalty:
            self.ensure_penalty_state()  # (allocated with the request: a no-op here)
        guide = bool(variant & V_GUIDE)
        if guide:
            self.ensure_guide_state()    # (allocated with the request: a no-op here)
        lay = MetaLayout(bucket, bucket, self.bt_width, 0, penalty=penalty, guide=guide)
        dev = torch.zeros(lay.size, dtype=torch.int32, device=self.device)
        v = lay.views(dev)
        # dummy sequences: kvlen 0, slot -1 -> kernels skip them
        v["seq_qstart"].copy_(torch.arange(bucket + 1, dtype=torch.int32))
        v["slot_mapping"].fill_(-1)
        if penalty:  # no penalty slot either: the warm-up and capture passes count nothing
            v["pen_slot"].fill_(-1)
        if guide:    # nor a guide slot: they advance nothing
            v["guide_slot"].fill_(-1)
        v["logits_idx"].copy_(torch.arange(bucket, dtype=torch.int64))
        md = self._meta(v, bucket, 0)
        # a capture may come between look-ahead steps (a new partition bucket mid-generation):
        # the warm-up passes sample into ws["tokens"], which still holds the in-flight step's
        # tokens the next step embeds - keep them (stream-ordered copy and restore)
        saved_tokens = self.ws["tokens"].clone()
        stream = torch.cuda.Stream(self.device)
        stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(stream):
            for _ in range(2):  # warm up (hipBLASLt heuristics, allocator)
                self._forward_sample(v, md, parts, variant)
        torch.cuda.current_stream(self.device).wait_stream(stream)
        dump_dir = os.environ.get("ATTA_GRAPH_DUMP_DIR")
        # node-level dump of every captured step (scripts/gpu/graph_nodes.py) keeps the
        # hipGraph after instantiation so its nodes can be listed
        g = torch.cuda.CUDAGraph(keep_graph=True) if dump_dir else torch.cuda.CUDAGraph()
        if self.graph_pool is None:
            self.graph_pool = torch.cuda.graph_pool_handle()
        with torch.cuda.graph(g, pool=self.graph_pool, stream=stream):
            out = self._forward_sample(v, md, parts, variant)
            toks = self.ws["tokens"]
            if out.data_ptr() != toks.data_ptr():  # every sampler path ends in ws["tokens"]
                toks[:bucket].copy_(out[:bucket])
                out = toks[:bucket]
        self.ws["tokens"].copy_(saved_tokens)
        torch.cuda.synchronize(self.device)
        key = (bucket, parts, variant)
        if dump_dir:
            os.makedirs(dump_dir, exist_ok=True)
            nodes = ops._native().graph_nodes(int(g.raw_cuda_graph()))
            path = os.path.join(dump_dir, f"tp{self.tp_size}_rank{self.tp_rank}_b{bucket}"
                                          f"_p{parts}_s{variant}.nodes")
            with open(path, "w") as f:
                f.write("\n".join(nodes) + "\n")
        self.graphs[key] = g
        self.graph_io[key] = {"layout": lay, "dev": dev, "out": out}

    def capture_all(self, all_parts: bool = False):
        """Capture every batch bucket at the full partition count (shorter-context partition
        buckets are captured on first use, or here with ``all_parts``)."""
        if not (self.is_cuda and self.cfg.use_graphs):
            return
        for b in self.graph_sizes:
            if not self._graph_ok(b):
                continue
            _, top, buckets = self._tier(b)
            for p in (buckets if all_parts else [top]):
                if (b, p, 0) not in self.graphs:
                    self.capture(b, p)

    def warm_library_gemms(self) -> int:
        """Run every shape of the loaded TunableOp table that this rank's weights have once
        (bf16: plain and residual-add GEMM; fp8: the row-scaled GEMM), so each rocBLAS /
        hipBLASLt solution's code object - and the libraries themselves - load at engine
        start, not inside the first request of that bucket (rocBLAS initialisation alone put
        ~1.1 s into the first 560-row prefill, bench/coldstart.py).  Returns the GEMMs run."""
        if self.gemm_table is None or not self.is_cuda or not self.model.layers:
            return 0
        import re

        L = self.model.layers[0]
        ws = {}
        for name in ("qkv", "o", "gate_up", "down"):
            w = getattr(L, name)
            if w is None:
                if self.model.w4_scratch is None:
                    continue  # with mxfp4_fp8_activations: no library GEMM reads this projection
                # mxfp4_weights_only: the library GEMMs read the expand scratch; for loading
                # their code objects its current contents do as well as any
                n_, k_ = self.model.proj_shape(L, name)
                w = self.model.w4_scratch[:n_ * k_].view(n_, k_)
            ws[tuple(w.shape)] = (w, getattr(L, name + "_s"))
        ws.setdefault(tuple(self.model.lm_head.shape), (self.model.lm_head, None))
        pat = re.compile(r"^(\w+?)_TN,tn_(\d+)_(\d+)_(\d+)_")
        n = 0
        with open(self.gemm_table) as f, torch.inference_mode():
            for line in f:
                mt = pat.match(line)
                if mt is None:
                    continue
                op, N, M, K = mt.group(1), int(mt.group(2)), int(mt.group(3)), int(mt.group(4))
                w, s = ws.get((N, K), (None, None))
                if w is None:
                    continue
                if op.startswith("ScaledGemm") and s is not None:
                    xq = torch.zeros(M, K, dtype=torch.uint8, device=self.device)
                    ops.gemm_fp8(xq, torch.ones(M, 1, device=self.device), w, s, self.dtype)
                elif op.startswith("GemmTunableOp") and s is None and w.dtype == self.dtype:
                    x = torch.zeros(M, K, dtype=w.dtype, device=self.device)
                    torch.nn.functional.linear(x, w)
                    torch.zeros(M, N, dtype=w.dtype, device=self.device).addmm_(x, w.t())
                else:
                    continue
                n += 1
        torch.cuda.synchronize(self.device)
        return n

    def warm_w4a8_kernels(self) -> int:
        """mxfp4_fp8_activations: run both builds of the W4A8 GEMM (plain, SiLU epilogue) once
        on the first layer's 4-bit copies, with the quantiser modes of its chain, so their code
        objects load at engine start.  Returns the launches."""
        if not self.is_cuda or not self.model.layers or self.model.layers[0].qkv_w4 is None:
            return 0
        from ..models.llama import W4_ROWMAPS

        L, n = self.model.layers[0], 0
        with torch.inference_mode():
            for proj, mode in (("qkv", ops.GEMM_PLAIN), ("gate_up", ops.GEMM_SILU)):
                wq, sq = getattr(L, proj + "_w4"), getattr(L, proj + "_b4")
                x = torch.zeros(1, wq.shape[1] * 2, dtype=torch.bfloat16, device=self.device)
                xq, xs = ops.quant_rows_fp8(x)
                ops.gemm_w4a8(xq, xs, wq, sq, W4_ROWMAPS[proj], mode)
                n += 1
            x = torch.zeros(1, self.mcfg.hidden_size, dtype=torch.bfloat16, device=self.device)
            ops.quant_rows_fp8(x, ops.QUANT_NORM, L.input_norm, self.mcfg.rms_norm_eps)
            ops.quant_rows_fp8(x, ops.QUANT_ADDNORM, L.input_norm, self.mcfg.rms_norm_eps,
                               x.clone())
        torch.cuda.synchronize(self.device)
        return n

    def reset_state(self):
        """Drop prefix cache contents (used between benchmark phases)."""
        self.bm.reset_prefix_cache()


__all__ = ["ModelRunner", "MetaLayout", "ref", "HDR_WORDS", "OP_STEP", "OP_CAPTURE", "OP_STOP",
           "OP_BARRIER", "LP_NONE", "LP_SAMPLED", "LP_TOPN", "TOP_N", "V_TOPKP", "V_PENALTY",
           "V_GUIDE", "V_SCORE", "SCORE_TOPN", "StepHeader", "SamplePlan", "sample_plan",
           "SlotPool", "variant_code", "variant_lp"]
