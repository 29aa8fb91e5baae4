"""Llama-3 decoder (8B / 70B / 3.2 shapes) over the atta op layer.

This is the model vLLM executes inside ``AsyncLLMEngine`` for the reference
(llm/serve_llm.py:362-378; model id from infra/docker-compose.yml:26).  MI355X design:

* weights are stored pre-fused: ``qkv`` [(Hq+2Hkv)*D, H], ``gate_up`` [2I, H] so each layer
  runs 4 GEMMs (hipBLASLt via F.linear for prefill-sized M; the decode path can swap in
  the fused GEMV kernels of ``ops``), and every elementwise step is a hand-written kernel:
  fused residual-add+RMSNorm, RoPE+paged-KV write, paged attention (prefill and decode
  variants), SiLU-mul, sampler;
* tensor parallelism is Megatron-style: qkv / gate_up column-parallel, o / down row-parallel
  with one all-reduce each (``parallel.comm``); the embedding is replicated and the LM head
  is vocab-parallel: the fused decode sampler reduces each shard to one packed key per row
  and an int64 MAX all-reduce picks the winner (prefill all-gathers the [B, V/tp] logits);
* weights are either seeded random-init (benchmarks: no network, gated checkpoints) or
  loaded from HF safetensors.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from pathlib import Path

import torch
import torch.nn.functional as F

from .. import ops
from ..config import ModelConfig
from . import step_plan as sp
from .step_plan import FUSED, GEMM, GEMM_SPLITK, GEMM_W4A8
from ..ops import reference as ref

DTYPES = {"bfloat16": torch.bfloat16, "bf16": torch.bfloat16, "float16": torch.float16,
          "fp16": torch.float16, "half": torch.float16, "auto": torch.bfloat16,
          "float32": torch.float32, "fp32": torch.float32}  # fp32: CPU reference runs only


# tile row map of each projection's 4-bit copy (ops.preshuffle_mxfp4)
W4_ROWMAPS = sp.W4_ROWMAPS


def torch_dtype(name: str) -> torch.dtype:
    return DTYPES.get(str(name).replace("torch.", ""), torch.bfloat16)


@dataclass
class AttnMeta:
    """Per-step attention metadata (all device tensors, built by the model runner)."""
    positions: torch.Tensor       # int32 [T]
    slot_mapping: torch.Tensor    # int32 [T]
    block_tables: torch.Tensor    # int32 [S, W]
    seq_kvlen: torch.Tensor       # int32 [S]
    seq_qstart: torch.Tensor      # int32 [S+1]
    tile_seq: torch.Tensor        # int32 [tiles]   (prefill sequences)
    tile_qoff: torch.Tensor       # int32 [tiles]
    logits_idx: torch.Tensor      # int64 [S]
    num_decode: int               # sequences [0, num_decode) have exactly one query token
    num_tiles: int


@dataclass
class SampleArgs:
    """What one step's sampler tail (``LlamaModel.sample_tail``) takes: the per-row device
    tensors, the decoded step variant and the penalty / guide state bound to this step."""
    temperature: torch.Tensor
    seeds: torch.Tensor
    steps: torch.Tensor
    top_p: torch.Tensor | None    # None unless plan.topkp
    top_k: torch.Tensor
    plan: object                  # SamplePlan (engine/step_msg.py)
    penalty: dict | None = None   # the runner's penalty state + "slot" / "rep" / "freq" / "pres"
    guide: dict | None = None     # the runner's guide state + "slot"


@dataclass
class LayerWeights:
    input_norm: torch.Tensor
    qkv: torch.Tensor | None
    o: torch.Tensor | None
    post_norm: torch.Tensor
    gate_up: torch.Tensor | None
    down: torch.Tensor | None
    # decode copies in the GEMV's pre-shuffled layout (ops.preshuffle); None = use the
    # row-major weights above
    qkv_ps: torch.Tensor | None = None
    o_ps: torch.Tensor | None = None
    gate_up_ps: torch.Tensor | None = None
    down_ps: torch.Tensor | None = None
    # fp8 weight-only quantisation (GPU): the projections above are uint8 e4m3fn bytes and
    # these are their fp32 per-output-row scales
    qkv_s: torch.Tensor | None = None
    o_s: torch.Tensor | None = None
    gate_up_s: torch.Tensor | None = None
    down_s: torch.Tensor | None = None
    # MXFP4 weight-only quantisation (GPU): the projections above hold the dequantised 16-bit
    # values; these are the 4-bit decode copies (ops.preshuffle_mxfp4: packed e2m1 codes) and
    # their e8m0 block scales, streamed by steps of at most 32 rows.  mxfp4_weights_only: the
    # four projections (and the *_ps copies) above are None - these are the only copy
    qkv_w4: torch.Tensor | None = None
    o_w4: torch.Tensor | None = None
    gate_up_w4: torch.Tensor | None = None
    down_w4: torch.Tensor | None = None
    qkv_b4: torch.Tensor | None = None
    o_b4: torch.Tensor | None = None
    gate_up_b4: torch.Tensor | None = None
    down_b4: torch.Tensor | None = None


class LlamaModel:
    def __init__(self, cfg: ModelConfig, dtype=torch.bfloat16, device="cuda", tp_rank: int = 0,
                 tp_size: int = 1, tp_group=None, quantization: str = "",
                 mxfp4_weights_only: bool = False, mxfp4_fp8_activations: bool = False):
        # tp_group: parallel.comm.TPComm (required when tp_size > 1)
        # quantization: "" (16-bit weights) | "fp8" (OCP e4m3fn weights, per-row scales; on the
        # CPU reference path the dequantised values are stored instead) | "mxfp4" (OCP
        # Microscaling FP4, weight-only: the projections are stored dequantised in 16 bits - every
        # path computes with exactly the quantised values - and prepare_decode_weights() adds the
        # 4-bit copies that steps of at most 32 rows stream; one GPU only)
        if quantization not in ("", "fp8", "mxfp4"):
            raise ValueError(f"unsupported quantization {quantization!r}")
        if quantization == "mxfp4" and tp_size > 1:
            raise ValueError("quantization 'mxfp4' runs on one GPU: tensor parallelism is not "
                             "supported with it")
        # mxfp4_weights_only: each layer is quantised as it is made and keeps its 4-bit copies
        # alone (no 16-bit projection survives _make_layer); steps without a 4-bit kernel
        # expand a projection into self.w4_scratch just before its GEMM.  GPU only.
        if mxfp4_weights_only and quantization != "mxfp4":
            raise ValueError("mxfp4_weights_only needs quantization 'mxfp4'")
        if mxfp4_weights_only and torch.device(device).type != "cuda":
            raise ValueError("mxfp4_weights_only needs a GPU: the CPU reference computes with "
                             "the dequantised 16-bit weights")
        # mxfp4_fp8_activations (W4A8): a step that no fused 4-bit kernel takes runs the
        # activation-quantised chain with every GEMM on ops.gemm_w4a8 - per-token e4m3
        # activations times the resident 4-bit weights; with mxfp4_weights_only there is then
        # no expand pass and no scratch.  Numerics of its own (as under "fp8": activations of
        # such steps are rounded to e4m3); the CPU reference runs the same arithmetic on the
        # dequantised weights.
        if mxfp4_fp8_activations and quantization != "mxfp4":
            raise ValueError("mxfp4_fp8_activations needs quantization 'mxfp4'")
        if (mxfp4_fp8_activations and torch.device(device).type == "cuda"
                and dtype != torch.bfloat16):
            raise ValueError("mxfp4_fp8_activations needs bfloat16 activations on a GPU "
                             "(ops.gemm_w4a8 writes bf16)")
        self.w4a8 = bool(mxfp4_fp8_activations)
        self.w4_only = bool(mxfp4_weights_only)
        self.w4_scratch = None  # [max N * K] 16-bit, allocated once at load
        self.quant = quantization
        # prefill projections: "hipblaslt" (torch / hipBLASLt GEMMs) or "atta" (the
        # hand-written CDNA4 GEMM, ops/csrc/prefill_gemm.hip) for >= prefill_gemm_min_rows rows
        self.prefill_gemm = "auto"
        self.prefill_gemm_min_rows = 128
        # prefill steps of <= 32 rows on the fused decode kernels (EngineConfig.small_prefill_fused)
        self.small_prefill_fused = True
        # the runner's fused-decode switch (EngineConfig.fused_decode): off also turns the
        # fused kernels off for small prefill steps
        self.fused_decode = True
        self.cfg = cfg
        self.dtype = dtype
        self.device = torch.device(device)
        self.tp_rank, self.tp_size, self.tp_group = tp_rank, tp_size, tp_group
        if cfg.num_heads % tp_size:
            raise ValueError(f"num_heads {cfg.num_heads} not divisible by tp {tp_size}")
        self.n_heads = cfg.num_heads // tp_size
        # KV heads are split when possible, replicated when tp > num_kv_heads
        self.kv_rep = max(1, tp_size // cfg.num_kv_heads)
        self.n_kv_heads = max(1, cfg.num_kv_heads // tp_size)
        self.head_dim = cfg.head_dim
        self.inter = cfg.intermediate_size // tp_size
        if cfg.intermediate_size % tp_size or cfg.vocab_size % tp_size:
            raise ValueError("intermediate/vocab not divisible by tp")
        self.vocab_shard = cfg.vocab_size // tp_size
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        self.layers: list[LayerWeights] = []
        self.lm_head_ps = None
        self.embed = None
        self.norm = None
        self.lm_head = None
        self.cos_sin = ref.rope_cos_sin(cfg.head_dim, min(cfg.max_position_embeddings, 1 << 17),
                                        cfg.rope_theta, cfg.rope_scaling, device=self.device)
        self.g = self.n_heads // self.n_kv_heads
        self._proj_dims_ok = sp.proj_dims_ok(self.device.type == "cuda", self.quant,
                                             cfg.hidden_size, self.n_heads * self.head_dim,
                                             self.inter)  # proj_fusable
        if self.head_dim != 128 and self.device.type == "cuda":
            raise ValueError("HIP attention kernels require head_dim 128")

    # ---------------------------------------------------------------------------------
    @property
    def qkv_width(self) -> int:
        return (self.n_heads + 2 * self.n_kv_heads) * self.head_dim

    def init_random(self, seed: int = 0, std: float = 0.02):
        """Seeded random-init weights of the full architecture (each rank draws its shard
        from the full-model generator stream so TP=N reproduces TP=1 exactly)."""
        cfg, dev, dt = self.cfg, self.device, self.dtype
        gen_dev = dev if dev.type == "cuda" else torch.device("cpu")
        g = torch.Generator(device=gen_dev)

        def rnd(shape, tag: int, scale=std):
            g.manual_seed(seed * 1000003 + tag)
            return (torch.randn(shape, generator=g, device=gen_dev, dtype=torch.float32)
                    * scale).to(dt).to(dev)

        H, D = cfg.hidden_size, cfg.head_dim
        self.embed = rnd((cfg.vocab_size, H), 1, 1.0)

        def norm_w(tag):  # non-trivial norm weights so the folding is exercised
            return (1.0 + rnd((H,), tag, 0.1).float()).to(dt)

        self.norm = norm_w(3)
        lm = self.embed if cfg.tie_word_embeddings else rnd((cfg.vocab_size, H), 2)
        self.lm_head = self._shard_rows(lm, self.vocab_shard).contiguous()
        self.layers = []
        for i in range(cfg.num_layers):
            base = 100 + i * 10
            wq = rnd((cfg.q_size, H), base + 0)
            wk = rnd((cfg.kv_size, H), base + 1)
            wv = rnd((cfg.kv_size, H), base + 2)
            wo = rnd((H, cfg.q_size), base + 3)
            wg = rnd((cfg.intermediate_size, H), base + 4)
            wu = rnd((cfg.intermediate_size, H), base + 5)
            wd = rnd((H, cfg.intermediate_size), base + 6) / math.sqrt(2 * cfg.num_layers) * 4
            self.layers.append(self._make_layer(wq, wk, wv, wo, wg, wu, wd, norm_w(base + 7),
                                                norm_w(base + 8)))
            del wq, wk, wv, wo, wg, wu, wd
        self._fold_final_norm()
        self._alloc_w4_scratch()
        return self

    def _shard_rows(self, w: torch.Tensor, rows: int) -> torch.Tensor:
        if self.tp_size == 1:
            return w
        return w[self.tp_rank * rows:(self.tp_rank + 1) * rows]

    def _shard_cols(self, w: torch.Tensor, cols: int) -> torch.Tensor:
        if self.tp_size == 1:
            return w
        return w[:, self.tp_rank * cols:(self.tp_rank + 1) * cols]

    def _make_layer(self, wq, wk, wv, wo, wg, wu, wd, n_in, n_post) -> LayerWeights:
        D = self.head_dim
        q = self._shard_rows(wq, self.n_heads * D)
        kv_rank = self.tp_rank // self.kv_rep
        if self.tp_size == 1:
            k, v = wk, wv
        else:
            k = wk[kv_rank * self.n_kv_heads * D:(kv_rank + 1) * self.n_kv_heads * D]
            v = wv[kv_rank * self.n_kv_heads * D:(kv_rank + 1) * self.n_kv_heads * D]
        qkv = torch.cat([q, k, v], 0).contiguous()
        o = self._shard_cols(wo, self.n_heads * D).contiguous()
        gu = torch.cat([self._shard_rows(wg, self.inter), self._shard_rows(wu, self.inter)],
                       0).contiguous()
        down = self._shard_cols(wd, self.inter).contiguous()
        # Fold the RMSNorm weights into the following projections (x*w) W^T = x (W diag(w))^T:
        # the decode kernels then only need the per-row rms, and the prefill path normalises
        # with a unit weight.  Both paths see identical folded weights.
        qkv = (qkv.float() * n_in.float()[None, :]).to(qkv.dtype).contiguous()
        gu = (gu.float() * n_post.float()[None, :]).to(gu.dtype).contiguous()
        ones = self._ones(n_in)
        if self.quant == "fp8":
            # row-parallel shards (o, down: a K slice of every row) quantise with the FULL
            # row's scale, so TP=N fp8 weights equal TP=1's bit for bit
            full = self.tp_size > 1
            amax = (wo.float().abs().amax(1) if full else None,
                    wd.float().abs().amax(1) if full else None)
            return self._quantize_layer(ones, qkv, o, gu, down, amax)
        if self.w4_only:
            # 4 bits only: quantise, lay out for the kernels, drop the 16-bit tensor - one at a
            # time, so the peak is this layer's 16-bit weights, not the model's
            L = LayerWeights(ones, None, None, ones, None, None)
            for proj, w in (("qkv", qkv), ("o", o), ("gate_up", gu), ("down", down)):
                wq, sq = ops.preshuffle_mxfp4(*ops.quantize_mxfp4(w), W4_ROWMAPS[proj])
                setattr(L, proj + "_w4", wq)
                setattr(L, proj + "_b4", sq)
            return L
        if self.quant == "mxfp4":  # the values MXFP4 can represent, in 16 bits
            qkv, o, gu, down = (ops.dequantize_mxfp4(*ops.quantize_mxfp4(w), self.dtype)
                                for w in (qkv, o, gu, down))
        return LayerWeights(ones, qkv, o, ones, gu, down)

    # -- mxfp4_weights_only ----------------------------------------------------------------
    def proj_shape(self, L: LayerWeights, proj: str) -> tuple[int, int]:
        """(N, K) of a layer projection, whichever copies exist."""
        w = getattr(L, proj)
        if w is not None:
            return tuple(w.shape)
        wq = getattr(L, proj + "_w4")
        return wq.shape[0], wq.shape[1] * 2

    def _alloc_w4_scratch(self):
        """The one 16-bit scratch of the weights-only mode: the largest projection's N * K
        values, shared by every layer and projection (a step expands into it in stream order,
        just before the GEMM that reads it).  Allocated once at load.  None with
        mxfp4_fp8_activations: every step without a 4-bit fused kernel runs ops.gemm_w4a8 on
        the 4-bit copies themselves."""
        if self.w4_only and self.layers and not self.w4a8:
            n = max(math.prod(self.proj_shape(self.layers[0], p)) for p in sp.PROJS)
            self.w4_scratch = torch.empty(n, dtype=self.dtype, device=self.device)

    def _w16(self, L: LayerWeights, proj: str) -> torch.Tensor:
        """The row-major 16-bit weight of a projection for a library / prefill GEMM: the stored
        tensor, or (weights-only mode) the 4-bit copy expanded into the shared scratch - valid
        until the next call."""
        w = getattr(L, proj)
        if w is not None:
            return w
        if self.w4_scratch is None:
            raise RuntimeError("mxfp4_weights_only: no 16-bit scratch (weights not loaded?)")
        n, k = self.proj_shape(L, proj)
        return ops.expand_mxfp4(getattr(L, proj + "_w4"), getattr(L, proj + "_b4"),
                                W4_ROWMAPS[proj], self.w4_scratch[:n * k].view(n, k))

    def dense_weight(self, layer_index: int, proj: str) -> torch.Tensor:
        """The exact 16-bit values of a layer projection ("qkv" | "o" | "gate_up" | "down",
        norm weights folded in) as a new row-major tensor - for tests and tools that need a
        dense copy (tests/helpers.dense_logits) of a model that keeps none."""
        L = self.layers[layer_index]
        w = getattr(L, proj)
        if w is not None and L.qkv_s is None:
            return w.clone()
        if getattr(L, proj + "_w4") is None:
            raise ValueError("dense_weight: 16-bit or MXFP4 weights only")
        codes, scales = ops.unshuffle_mxfp4(getattr(L, proj + "_w4"), getattr(L, proj + "_b4"),
                                            W4_ROWMAPS[proj])
        return ops.dequantize_mxfp4(codes, scales, self.dtype)

    def resident_weight_bytes(self) -> dict:
        """Bytes of weights held on the device, by kind: "codes4" (MXFP4 codes), "scales4"
        (their block scales), "fp8" (bytes + row scales), "w16" (every 16-bit tensor:
        embedding, norms, LM head, projections and pre-shuffled copies), "scratch"."""
        def nb(ts):
            seen, n = set(), 0
            for t in ts:
                if t is not None and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    n += t.numel() * t.element_size()
            return n

        Ls = self.layers
        main = [w for l in Ls for w in (l.qkv, l.o, l.gate_up, l.down, l.qkv_ps, l.o_ps,
                                        l.gate_up_ps, l.down_ps)]
        fp8 = [w for w in main if w is not None and w.dtype == torch.uint8]
        fp8 += [w for l in Ls for w in (l.qkv_s, l.o_s, l.gate_up_s, l.down_s)]
        w16 = [w for w in main if w is not None and w.dtype != torch.uint8]
        w16 += [self.embed, self.norm, self.lm_head, self.lm_head_ps]
        w16 += [w for l in Ls for w in (l.input_norm, l.post_norm)]
        return {"codes4": nb(w for l in Ls for w in (l.qkv_w4, l.o_w4, l.gate_up_w4, l.down_w4)),
                "scales4": nb(w for l in Ls for w in (l.qkv_b4, l.o_b4, l.gate_up_b4, l.down_b4)),
                "fp8": nb(fp8), "w16": nb(w16), "scratch": nb([self.w4_scratch])}

    def _quantize_layer(self, ones, qkv, o, gu, down, amax=(None, None)) -> LayerWeights:
        """fp8 weight-only quantisation of the four projections (after norm folding)."""
        qs = [ops.quantize_fp8(qkv), ops.quantize_fp8(o, amax[0]), ops.quantize_fp8(gu),
              ops.quantize_fp8(down, amax[1])]
        if self.device.type != "cuda":  # CPU reference: the values fp8 can represent
            deq = [ops.dequantize_fp8(q, sc, self.dtype) for q, sc in qs]
            return LayerWeights(ones, deq[0], deq[1], ones, deq[2], deq[3])
        return LayerWeights(ones, qs[0][0], qs[1][0], ones, qs[2][0], qs[3][0],
                            qkv_s=qs[0][1], o_s=qs[1][1], gate_up_s=qs[2][1], down_s=qs[3][1])

    def _ones(self, like):
        if getattr(self, "_ones_t", None) is None or self._ones_t.shape != like.shape:
            self._ones_t = torch.ones_like(like)
        return self._ones_t

    def _fold_final_norm(self):
        self.lm_head = (self.lm_head.float() * self.norm.float()[None, :]).to(
            self.lm_head.dtype).contiguous()
        self.norm = self._ones(self.norm)

    def load_safetensors(self, path: str):
        """Load HF Llama weights (model*.safetensors) and shard for this TP rank."""
        from safetensors import safe_open

        p = Path(path)
        files = sorted(p.glob("*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no safetensors in {path}")
        index = {}
        for f in files:
            with safe_open(str(f), framework="pt") as sf:
                for k in sf.keys():
                    index[k] = f

        def get(name):
            with safe_open(str(index[name]), framework="pt") as sf:
                return sf.get_tensor(name).to(self.dtype).to(self.device)

        cfg = self.cfg
        self.embed = get("model.embed_tokens.weight")
        self.norm = get("model.norm.weight")
        lm = self.embed if cfg.tie_word_embeddings or "lm_head.weight" not in index else get(
            "lm_head.weight")
        self.lm_head = self._shard_rows(lm, self.vocab_shard).contiguous()
        self.layers = []
        for i in range(cfg.num_layers):
            pre = f"model.layers.{i}."
            self.layers.append(self._make_layer(
                get(pre + "self_attn.q_proj.weight"), get(pre + "self_attn.k_proj.weight"),
                get(pre + "self_attn.v_proj.weight"), get(pre + "self_attn.o_proj.weight"),
                get(pre + "mlp.gate_proj.weight"), get(pre + "mlp.up_proj.weight"),
                get(pre + "mlp.down_proj.weight"), get(pre + "input_layernorm.weight"),
                get(pre + "post_attention_layernorm.weight")))
        self._fold_final_norm()
        self._alloc_w4_scratch()
        return self

    def prepare_decode_weights(self, copies16: bool = True):
        """Build pre-shuffled copies of every decode-GEMV weight (row-major originals stay
        for the hipBLASLt prefill GEMMs): each wave load of the decode kernels then reads one
        contiguous 1 KiB instead of 16 rows x 64 B.  Costs one extra copy of the weights,
        which 288 GB of HBM affords (16 GB for Llama-3-8B).

        mxfp4_weights_only: the layers hold their 4-bit copies already and get no 16-bit ones;
        only the LM head is pre-shuffled.

        quantization="mxfp4" always builds the 4-bit copies as well (4.25 bits per weight on
        top: re-quantising the stored values returns the codes they came from);
        ``copies16=False`` then leaves the 16-bit pre-shuffled copies out (no room: steps
        past 32 rows run from the row-major weights)."""
        if self.device.type != "cuda":
            return self
        if self.quant == "mxfp4":
            for L in self.layers:
                if L.qkv_w4 is not None:
                    continue
                for proj, rowmap in W4_ROWMAPS.items():
                    wq, sq = ops.preshuffle_mxfp4(*ops.quantize_mxfp4(getattr(L, proj)), rowmap)
                    setattr(L, proj + "_w4", wq)
                    setattr(L, proj + "_b4", sq)
            if not copies16:
                torch.cuda.synchronize(self.device)
                return self
        for L in self.layers:
            if L.qkv is None:  # mxfp4_weights_only: the LM head's copy alone
                break
            if L.qkv_s is not None:  # fp8: 16-row x 64-col blocks of bytes
                L.qkv_ps = ops.preshuffle_fp8(L.qkv, "qkv")
                L.o_ps = ops.preshuffle_fp8(L.o)
                L.gate_up_ps = ops.preshuffle_fp8(L.gate_up, "silu")
                L.down_ps = ops.preshuffle_fp8(L.down)
                continue
            L.qkv_ps = ops.preshuffle(L.qkv, "qkv")
            L.o_ps = ops.preshuffle(L.o)
            L.gate_up_ps = ops.preshuffle(L.gate_up, "silu")
            L.down_ps = ops.preshuffle(L.down)
        self.lm_head_ps = ops.preshuffle(self.lm_head)
        torch.cuda.synchronize(self.device)
        return self

    def decode_copy_bytes(self) -> int:
        """Bytes ``prepare_decode_weights`` adds (one copy of every decode GEMV weight)."""
        ts = [self.lm_head] + [w for l in self.layers for w in (l.qkv, l.o, l.gate_up, l.down)]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    # ---------------------------------------------------------------------------------
    def weight_bytes(self) -> int:
        """Bytes of the weights one forward streams (row-major copies, scales included)."""
        ts = [self.embed, self.norm, self.lm_head]
        for l in self.layers:
            ts += [l.input_norm, l.qkv, l.o, l.post_norm, l.gate_up, l.down, l.qkv_s, l.o_s,
                   l.gate_up_s, l.down_s]
            if l.qkv is None:  # mxfp4_weights_only: the 4-bit copies are what is streamed
                ts += [l.qkv_w4, l.o_w4, l.gate_up_w4, l.down_w4, l.qkv_b4, l.o_b4,
                       l.gate_up_b4, l.down_b4]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def _all_reduce(self, x: torch.Tensor) -> torch.Tensor:
        if self.tp_size > 1:
            self.tp_group.all_reduce(x)
        return x

    def forward(self, input_ids: torch.Tensor, md: AttnMeta, k_caches, v_caches,
                part_out=None, part_lse=None, num_parts: int = 1, part_tokens: int = 256,
                prev_tokens=None, feed_prev=None, rows: torch.Tensor | None = None):
        """Returns the final normed hidden state rows [T, H] - or only ``rows`` (int64 row
        indices, e.g. each sequence's last token) when given: the final norm then runs on
        those rows alone."""
        cfg = self.cfg
        eps = cfg.rms_norm_eps
        # the residual stream IS the embedding output: every row-parallel projection adds its
        # product into it inside the GEMM epilogue (hipBLASLt beta=1 C-matrix epilogue, or the
        # skinny GEMV's RESADD) - no separate add / copy passes over [T, hidden]
        residual = ops.embed(self.embed, input_ids, prev_tokens, feed_prev)
        T = residual.shape[0]
        nq, nkv, D = self.n_heads, self.n_kv_heads, self.head_dim
        dt = residual.dtype
        pending = None  # fp8 chain: the previous down_proj output, added by the next norm kernel
        # one backend per projection, the same for every layer (step_plan.py has the table):
        # small steps run the fused decode kernels around the prefill attention - 5 launches per
        # layer at weight-stream speed instead of ~9 with the row-major skinny / library GEMMs
        # (17 rows: 168 -> ~80 us of GEMMs per layer, profiles/r4_small_prefill_fused.txt);
        # 129..640-row steps (uncached burst / planning prefills) run the mid-M kernel per
        # projection where it beats the tuned library GEMM + separate kernels; fp8 steps past
        # the fused rows run the activation-quantised chain: every projection is ONE fp8 GEMM
        # with row-wise scales whose activation operand comes quantised out of the norm /
        # SiLU-mul kernel that produced it
        plan = self.step_plan(T)
        for li, L in enumerate(self.layers):
            if plan.qkv == FUSED:
                q = ops.decode_qkv_rope(residual, eps=eps, positions=md.positions,
                                        slots=md.slot_mapping, cos_sin=self.cos_sin,
                                        k_cache=k_caches[li], v_cache=v_caches[li], n_q_heads=nq,
                                        n_kv_heads=nkv, **self._decode_w(L, "qkv", T))
            else:
                if plan.fp8_chain:
                    if pending is None:
                        xq, xs = ops.quant_rows_fp8(residual, ops.QUANT_NORM, L.input_norm, eps)
                    else:
                        xq, xs = ops.quant_rows_fp8(pending, ops.QUANT_ADDNORM, L.input_norm,
                                                    eps, residual)
                    qkv = self._chain_gemm(plan.qkv, L, "qkv", xq, xs, dt)
                else:
                    x = ops.rms_norm(residual, L.input_norm, eps)
                    wqkv = self._w16(L, "qkv")
                    qkv = ops.prefill_gemm(x, wqkv) if plan.qkv == GEMM else ops.linear(x, wqkv)
                q = ops.rope_cache(qkv, md.positions, md.slot_mapping, self.cos_sin,
                                   k_caches[li], v_caches[li], nq, nkv, D)
            attn = torch.empty_like(q)
            if md.num_decode > 0:
                ops.attention_decode(q, k_caches[li], v_caches[li], md.block_tables,
                                     md.seq_kvlen, md.seq_qstart, self.scale, part_out, part_lse,
                                     num_parts, part_tokens, out=attn, num_seqs=md.num_decode)
            if md.num_tiles > 0:
                ops.attention_prefill(q, k_caches[li], v_caches[li], md.block_tables,
                                      md.seq_kvlen, md.seq_qstart, md.tile_seq, md.tile_qoff,
                                      self.scale, out=attn)
            if plan.fp8_chain:
                aq, as_ = ops.quant_rows_fp8(attn.view(T, nq * D))
                y = self._all_reduce(self._chain_gemm(plan.o, L, "o", aq, as_, dt))
                xq, xs = ops.quant_rows_fp8(y, ops.QUANT_ADDNORM, L.post_norm, eps, residual)
                if plan.gate_up == GEMM:
                    # SiLU-mul fused into the gate_up GEMM epilogue: [T, I] out, plain quant
                    act = ops.prefill_gemm(xq, L.gate_up, ops.GEMM_SILU, xs=xs, ws=L.gate_up_s)
                    aq, as_ = ops.quant_rows_fp8(act)
                elif plan.gate_up == GEMM_W4A8:
                    act = self._chain_gemm(plan.gate_up, L, "gate_up", xq, xs, dt, ops.GEMM_SILU)
                    aq, as_ = ops.quant_rows_fp8(act)
                else:
                    gu = ops.gemm_fp8(xq, xs, L.gate_up, L.gate_up_s, dt)
                    aq, as_ = ops.quant_rows_fp8(gu, ops.QUANT_SILU)
                pending = self._all_reduce(self._chain_gemm(plan.down, L, "down", aq, as_, dt))
                continue
            self._proj_residual(plan.o, attn.view(T, nq * D), L, "o", residual)
            if plan.gate_up == FUSED:
                a = ops.decode_gate_up_silu(residual, eps=eps, **self._decode_w(L, "gate_up", T))
            elif L.gate_up_s is not None:
                # fp8 gate_up of a fused step past its crossover: an fp8 GEMM on row-quantised
                # activations (norm fused into the quantiser), bf16 SiLU-mul for the fused down
                xq, xs = ops.quant_rows_fp8(residual, ops.QUANT_NORM, L.post_norm, eps)
                a = ops.silu_and_mul(self._gemm8(plan.gate_up, xq, xs, L.gate_up, L.gate_up_s, dt))
            else:
                x = ops.rms_norm(residual, L.post_norm, eps)
                wgu = self._w16(L, "gate_up")
                if plan.gate_up == GEMM:
                    a = ops.prefill_gemm(x, wgu, ops.GEMM_SILU)
                else:
                    a = ops.silu_and_mul(ops.linear(x, wgu))
            self._proj_residual(plan.down, a, L, "down", residual)
        if rows is not None:
            residual = residual.index_select(0, rows)
            pending = None if pending is None else pending.index_select(0, rows)
        if pending is not None:
            return ops.fused_add_rms_norm(pending, residual, self.norm, eps)
        return ops.rms_norm(residual, self.norm, eps)

    # the measured routing tables (step_plan.py); read at call time, so an instance may
    # assign its own
    MIDM_ROUTES = sp.MIDM_ROUTES
    MIDM_FP8_ROWS = sp.MIDM_FP8_ROWS
    FP8_GATE_UP_WIDE_MAX = sp.FP8_GATE_UP_WIDE_MAX
    FP8_FUSED_MAX_ROWS = sp.FP8_FUSED_MAX_ROWS
    _PG_AUTO = sp.PG_AUTO
    _PG_AUTO_UNTUNED = sp.PG_AUTO_UNTUNED
    _PG_SPLITK = sp.PG_SPLITK
    gemm_tuned = False  # set by the model runner when a tuned library table is loaded

    def _w4_rows(self, T: int) -> bool:
        """Does a T-row step stream the MXFP4 copies (the 4-bit build of the 16-row-tile GEMV;
        mxfp4_weights_only: or the wide kernel's 4-bit builds)?"""
        return (self.quant == "mxfp4" and bool(self.layers) and self.layers[0].qkv_w4 is not None
                and ops.fused_kernel(T, True, mxfp4=True, wide_w4=self.w4_only) is not None)

    def _decode_w(self, L: LayerWeights, proj: str, T: int) -> dict:
        """The weight arguments of a fused op for a T-row step: the 4-bit copy with its block
        scales, else the pre-shuffled copy (fp8: with its row scales), else the row-major
        weight."""
        if self._w4_rows(T):
            return {"w": getattr(L, proj + "_w4"), "w_block_scale": getattr(L, proj + "_b4"),
                    "wide_w4": self.w4_only}
        if self.w4_only:
            raise RuntimeError(f"mxfp4_weights_only: no 4-bit kernel runs a {T}-row fused "
                               f"{proj} (the step plan sends such steps through the scratch)")
        ps = L.qkv_ps is not None
        return {"w": getattr(L, proj + "_ps") if ps else getattr(L, proj), "preshuffled": ps,
                "w_scale": getattr(L, proj + "_s")}

    def step_plan(self, T: int) -> sp.StepPlan:
        """The backend of each projection of a T-row prefill / mixed step, whether it runs the
        activation-quantised fp8 chain and whether the runner pads its rows (step_plan.py).
        Every fact is read now: tests and tuning tools assign them after construction."""
        gpu = self.device.type == "cuda"
        return sp.step_plan(T, sp.StepFacts(
            gpu=gpu, quant=self.quant,
            wdtype=torch.uint8 if gpu and self.quant == "fp8" else self.dtype,
            tp_size=self.tp_size,
            preshuffled=bool(self.layers) and self.layers[0].qkv_ps is not None,
            hidden=self.cfg.hidden_size, q_width=self.n_heads * self.head_dim,
            kv_width=self.n_kv_heads * self.head_dim, inter=self.inter,
            gemm_tuned=self.gemm_tuned, prefill_gemm=self.prefill_gemm,
            prefill_gemm_min_rows=self.prefill_gemm_min_rows,
            small_prefill_fused=self.small_prefill_fused, fused_decode=self.fused_decode,
            w4_only=self.w4_only, w4a8=self.w4a8, midm_routes=self.MIDM_ROUTES, pg_auto=self._PG_AUTO,
            pg_auto_untuned=self._PG_AUTO_UNTUNED, pg_splitk=self._PG_SPLITK,
            midm_fp8_rows=self.MIDM_FP8_ROWS, fp8_gate_up_wide_max=self.FP8_GATE_UP_WIDE_MAX,
            fp8_fused_max_rows=self.FP8_FUSED_MAX_ROWS))

    @staticmethod
    def _gemm8(backend, xq, xs, w, ws, dt):
        """fp8 prefill projection on row-quantised activations: the hand-written fp8 GEMM or
        the hipBLASLt row-scaled GEMM."""
        if backend == GEMM:
            return ops.prefill_gemm(xq, w, xs=xs, ws=ws)
        return ops.gemm_fp8(xq, xs, w, ws, dt)

    def _chain_gemm(self, backend, L, proj, xq, xs, dt, mode=ops.GEMM_PLAIN):
        """One projection of the activation-quantised chain on the plan's backend: an fp8
        weight GEMM (``_gemm8``), or the W4A8 GEMM on the layer's resident 4-bit copy.  The CPU
        reference has no 4-bit copies: it runs the W4A8 arithmetic (e4m3 activations, fp32
        accumulation, bf16 out) on the dequantised 16-bit weight."""
        if backend != GEMM_W4A8:
            return self._gemm8(backend, xq, xs, getattr(L, proj), getattr(L, proj + "_s"), dt)
        wq = getattr(L, proj + "_w4")
        if wq is not None:
            return ops.gemm_w4a8(xq, xs, wq, getattr(L, proj + "_b4"), W4_ROWMAPS[proj], mode)
        if xq.is_cuda:
            raise RuntimeError("mxfp4_fp8_activations: no 4-bit copies (prepare_decode_weights "
                               "not run?)")
        y = (xq.view(torch.float8_e4m3fn).float() @ getattr(L, proj).float().t()) * xs
        if mode == ops.GEMM_SILU:
            y = F.silu(y[:, :self.inter]) * y[:, self.inter:]
        return y.to(torch.bfloat16).to(dt)

    def _proj_residual(self, backend, x, L, proj, residual):
        """residual += x @ w.T (row-parallel o / down projection; TP: all-reduced partial
        sums) on the plan's backend."""
        if backend == FUSED:
            return self._row_parallel(x, L, proj, residual)
        w = self._w16(L, proj)
        if backend == GEMM_SPLITK:
            return ops.prefill_gemm(x, w, ops.GEMM_RESADD, residual=residual, schedule="splitk")
        if self.tp_size > 1:
            # residual += sum over ranks, the add fused into the IPC reduction's epilogue
            y = ops.prefill_gemm(x, w) if backend == GEMM else ops.linear(x, w)
            return self.tp_group.all_reduce_residual(y, residual)
        if backend == GEMM:
            return ops.prefill_gemm(x, w, ops.GEMM_RESADD, residual=residual)
        return ops.linear(x, w, residual=residual)

    def midm_route(self, T: int) -> dict:
        """{projection: True} for the projections of a T-row 16-bit step that run the mid-M
        kernel (empty when the step cannot: TP, fp8, no pre-shuffled weights, rows past
        ops.MIDM_MAX_M)."""
        if T <= ops.WIDE_ROWS or self.quant == "fp8":
            return {}
        plan = self.step_plan(T)
        return {p: True for p in sp.PROJS if getattr(plan, p) == FUSED}

    def midm_fp8_ok(self, T: int) -> bool:
        """Does an fp8 step past the wide kernel's rows run qkv / o / down on the mid-M W8
        builds (MIDM_FP8_ROWS)?  Its gate_up is past the fp8 crossover: the library fp8 GEMM."""
        return self.quant == "fp8" and T > ops.WIDE_ROWS and self.step_plan(T).qkv == FUSED

    def small_prefill_ok(self, T: int) -> bool:
        """Does a (prefill or mixed) step of T rows run on the fused decode kernels - RMSNorm
        folded into the pre-shuffled skinny GEMVs, RoPE + KV write in the QKV epilogue, SiLU-mul
        in gate_up?  Such steps stay unpadded; steps that take the library path are padded to
        its tuned buckets (fused_decode=False turns the fused kernels off here too).
        Up to 128 rows, 16-bit or fp8 weights, any TP degree (the row-parallel sums go through
        _row_parallel); past 128 rows every projection is routed on its own (midm_route)."""
        return not self.step_plan(T).pad_rows

    def proj_fusable(self, T: int) -> bool:
        """Can the layer projections of a T-row step run the hand-written weight-streaming
        kernels (ops.fused_kernel: the 16-row-tile GEMVs on any layout, the wide small-M and
        mid-M kernels over the pre-shuffled 16-bit or fp8 weights)?  Any TP degree up to the
        wide kernel's rows (past the fused push's rows the row-parallel sums take the IPC /
        RCCL all-reduce); the mid-M routes are measured at TP = 1 shapes only."""
        ps = bool(self.layers) and self.layers[0].qkv_ps is not None
        return sp.proj_fusable(T, self._proj_dims_ok, self.tp_size, ps, self.quant, self.w4_only)

    def decode_step_fusable(self, B: int) -> bool:
        """Can ``forward_decode`` run B sequences?  It runs every projection fused (gate_up
        included, which loses to the library past the wide kernel's rows: MIDM_ROUTES) and
        ends in the fused LM head + sampler."""
        return (self.proj_fusable(B) and B <= min(ops.fused_max_rows(), ops.WIDE_ROWS)
                and (not self.w4_only or self._w4_rows(B))
                and self.sampler_fusable(B))

    def sampler_fusable(self, rows: int) -> bool:
        """Can ``sample_rows`` take these rows?  The LM-head kernels with the sampler epilogue,
        streaming K = hidden in 128-wide (16-bit) wave steps."""
        lm_ps = self.lm_head_ps is not None
        return (self.device.type == "cuda" and self.cfg.hidden_size % 128 == 0
                and ops.fused_kernel(rows, lm_ps, False, "sample") is not None)

    def forward_decode(self, input_ids: torch.Tensor, md: AttnMeta, k_caches, v_caches, ws: dict,
                       args: SampleArgs, prev_tokens=None, feed_prev=None, max_qlen: int = 1,
                       min_qlen: int = 1) -> torch.Tensor:
        """Fused decode step; returns sampled ids, one per row.  Every sequence has one query
        row - or, in a verify step of speculative decoding (``max_qlen`` > 1: the longest of
        the batch), sequence s of ``md.num_decode`` has the rows ``md.seq_qstart[s]`` ..
        ``md.seq_qstart[s + 1] - 1`` (its pending token and its drafts, at most 16 // G), the
        attention is ``ops.attention_decode_mq`` (the multi-query kernel for the sequences with
        drafts, the one-token kernel for those without; ``min_qlen``: the shortest qlen) and
        ``args``' temperature / seeds / steps are per row.

        Per layer: [RMSNorm+QKV+RoPE+KV-write] -> [paged attention, in-kernel split-K
        combine] -> [o_proj + residual add] -> [RMSNorm+gate_up+SiLU*up] ->
        [down_proj + residual add]; then ``sample_tail``: [final RMSNorm + LM head + sampler].
        5 kernels per layer instead of ~10, no normalised activations or logits ever hit HBM -
        unless ``args.plan`` materialises the logits."""
        eps = self.cfg.rms_norm_eps
        nq, nkv = self.n_heads, self.n_kv_heads
        B = input_ids.shape[0]
        residual = ops.embed(self.embed, input_ids, prev_tokens, feed_prev)
        q = ws["q"][:B]
        attn = ws["attn"][:B]
        act = ws["act"][:B]
        # verify step: which sequences the one-token and the multi-query kernel take (once
        # per step, every layer's attention reuses it)
        split = (ops.mq_split_kvlen(md.seq_kvlen, md.seq_qstart, md.num_decode)
                 if max_qlen > 1 and min_qlen <= 1 and q.is_cuda else None)
        for li, L in enumerate(self.layers):
            if L.qkv_s is not None and L.qkv_ps is None:
                raise RuntimeError("fp8 decode needs prepare_decode_weights()")
            ops.decode_qkv_rope(residual, eps=eps, positions=md.positions,
                                slots=md.slot_mapping, cos_sin=self.cos_sin,
                                k_cache=k_caches[li], v_cache=v_caches[li], n_q_heads=nq,
                                n_kv_heads=nkv, q_out=q, **self._decode_w(L, "qkv", B))
            if max_qlen > 1:
                ops.attention_decode_mq(q, k_caches[li], v_caches[li], md.block_tables,
                                        md.seq_kvlen, md.seq_qstart, self.scale, ws["part_out"],
                                        ws["part_lse"], ws["counters"], ws["max_parts"],
                                        ws["part_tokens"], out=attn, num_seqs=md.num_decode,
                                        max_qlen=max_qlen, min_qlen=min_qlen, split=split)
            else:
                ops.attention_decode_v2(q, k_caches[li], v_caches[li], md.block_tables,
                                        md.seq_kvlen, md.seq_qstart, self.scale, ws["part_out"],
                                        ws["part_lse"], ws["counters"], ws["max_parts"],
                                        ws["part_tokens"], out=attn, num_seqs=B)
            self._row_parallel(attn.view(B, nq * self.head_dim), L, "o", residual)
            ops.decode_gate_up_silu(residual, eps=eps, out=act,
                                    **self._decode_w(L, "gate_up", B))
            self._row_parallel(act, L, "down", residual)
        return self.sample_tail(residual, eps, args, ws, out=ws["tokens"][:B], fused_ok=True)

    def sample_tail(self, x: torch.Tensor, eps: float, args: SampleArgs, ws: dict, out=None,
                    fused_ok: bool = True) -> torch.Tensor:
        """The end of every step: one token per row of ``x`` (``eps`` > 0: rows still to be
        normalised; 0: already normalised, as ``forward`` returns them).

        Fused (the plan materialises nothing and ``fused_ok``: ``sampler_fusable`` rows):
        ``sample_rows``, the LM head and the sampler in one kernel, tokens in ws["tokens"];
        with ``plan.lp_fused`` its logprob epilogue leaves each sampled token's logprob in
        ws["lp"] (same launch count, tokens bit-identical to the plain step's).

        Materialised (top-k / top-p, penalties, guides, every other logprob mode, or rows the
        fused kernels do not take): [RMSNorm] -> ``compute_logits`` -> ``sample_logits`` into
        ``out`` (None: a fresh tensor) -> with ``plan.lp_top`` ``ops.token_logprobs`` of the
        samples and their ``lp_top`` alternatives into ws["lp"] / ws["top_ids"] / ws["top_lp"]
        (logprobs read the raw logits, not the penalised or masked ones)."""
        plan = args.plan
        if not plan.materialise and fused_ok:
            return self.sample_rows(x, eps, args.temperature, args.seeds, args.steps, ws,
                                    logprobs=plan.lp_fused)
        logits = self.compute_logits(ops.rms_norm(x, self.norm, eps) if eps > 0 else x)
        toks = self.sample_logits(logits, args.temperature, args.seeds, args.steps,
                                  top_p=args.top_p, top_k=args.top_k, out=out,
                                  penalty=args.penalty, guide=args.guide)
        if plan.lp_top is not None:
            self.logits_logprobs(logits, toks, plan.lp_top, ws)
        return toks

    @staticmethod
    def sample_logits(logits: torch.Tensor, temperature, seeds, steps, top_p=None, top_k=None,
                      out=None, penalty: dict | None = None,
                      guide: dict | None = None) -> torch.Tensor:
        """Sample one token per materialised ``logits`` row: the top-k / top-p kernel with
        ``top_p`` (per-row device tensors), else the plain sampler.  ``penalty`` (the runner's
        penalty state plus this step's per-row "slot" / "rep" / "freq" / "pres"): the sampler
        reads ``ops.penalty_apply``'s fp32 rows instead of the raw ones and
        ``ops.penalty_update`` then counts the sampled tokens - apply, sample, update, all on
        device-side parameters, so the tail is captured with the step.  ``guide`` (the runner's
        guide state plus this step's per-row "slot"): ``ops.guide_apply`` masks the rows - the
        penalised ones in place, else the raw ones into the fp32 buffer - by each row's
        automaton state and ``ops.guide_advance`` moves the states by the sampled tokens.  The
        order: penalty_apply, guide_apply, sampler, penalty_update, guide_advance."""
        src = logits
        if penalty is not None:
            src = ops.penalty_apply(penalty["logits"][:logits.shape[0]], logits,
                                    penalty["state"], penalty["slot"], penalty["rep"],
                                    penalty["freq"], penalty["pres"], penalty["bias_ids"],
                                    penalty["bias_vals"])
        if guide is not None:
            src = ops.guide_apply(guide["logits"][:logits.shape[0]], src, guide["next"],
                                  guide["state"], guide["slot"])
        if top_p is not None:
            toks = ops.sample_topkp(src, temperature, top_p, top_k, seeds, steps, out=out)
        else:
            toks = ops.sample(src, temperature, seeds, steps, out=out)
        if penalty is not None:
            ops.penalty_update(penalty["state"], penalty["slot"], toks)
        if guide is not None:
            ops.guide_advance(guide["state"], guide["next"], guide["slot"], toks)
        return toks

    @staticmethod
    def logits_logprobs(logits: torch.Tensor, toks: torch.Tensor, n_top: int, ws: dict) -> None:
        """Logprobs of the samples ``toks`` under the materialised ``logits`` rows, and the
        ``n_top`` most likely tokens per row, into ws["lp"] / ws["top_ids"] / ws["top_lp"]
        (every rank under TP: the logits are all-gathered)."""
        n = logits.shape[0]
        ops.token_logprobs(logits, toks, n_top,
                           out=(ws["lp"][:n], ws["top_ids"][:n], ws["top_lp"][:n]))

    def _row_parallel(self, x: torch.Tensor, L, proj: str, residual: torch.Tensor) -> None:
        """residual += x @ W.T for the row-parallel o / down projection on the fused kernels
        (16-row-tile GEMV, wide or mid-M kernel; fp8 weights with their row scales).  TP: the
        GEMV epilogue pushes the partial product into the peers' IPC slots and one receive
        kernel adds the rank-order sum into the residual (X1 / X2, <= 32 rows), else the
        product goes through the all-reduce whose epilogue adds it (IPC one- / two-shot, or
        RCCL)."""
        if self._w4_rows(x.shape[0]):  # MXFP4: one GPU only
            ops.linear(x, getattr(L, proj + "_w4"), residual=residual,
                       waves=ops.decode_waves(proj, mxfp4=True), ksplit=None, proj=proj,
                       w_block_scale=getattr(L, proj + "_b4"), wide_w4=self.w4_only)
            return
        if self.w4_only:
            raise RuntimeError(f"mxfp4_weights_only: no 4-bit kernel runs a {x.shape[0]}-row "
                               f"fused {proj}")
        ps = L.qkv_ps is not None
        w = getattr(L, proj + "_ps") if ps else getattr(L, proj)
        scale = getattr(L, proj + "_s")
        waves = ops.decode_waves(proj, ps, scale is not None)
        if self.tp_size == 1:
            ops.linear(x, w, residual=residual, waves=waves, preshuffled=ps, w_scale=scale,
                       ksplit=None, proj=proj)
        elif self.tp_group.push_ok(x.shape[0], w.shape[0]):
            ops.linear_push_reduce(x, w, residual, self.tp_group.ipc, waves=waves,
                                   preshuffled=ps, w_scale=scale, proj=proj)
        else:
            self.tp_group.all_reduce_residual(
                ops.linear(x, w, waves=waves, preshuffled=ps, w_scale=scale, ksplit=None,
                           proj=proj), residual)

    def sample_rows(self, x, eps, temperature, seeds, steps, ws,
                    logprobs: bool = False) -> torch.Tensor:
        """[final RMSNorm (eps > 0) +] LM head + sampler for ``sampler_fusable`` rows (<= 32 on
        row-major weights, <= 128 pre-shuffled) without materialising logits; tokens land in
        ws["tokens"][:B] on every rank (an async look-ahead step embeds them from there).  Used
        by the fused decode step and for the last-token rows of prefill steps (their rows are
        already normalised: eps = 0).  ``logprobs`` (one GPU only): the launch records each
        token's logprob into ws["lp"][:B] as well (the SAMPLE_LP epilogue)."""
        B = x.shape[0]
        lm_ps = self.lm_head_ps is not None
        lm = self.lm_head_ps if lm_ps else self.lm_head
        if self.tp_size == 1:
            lp = {"logprobs": ws["lp"][:B], "lp_ws": ws["lp_ws"]} if logprobs else {}
            return ops.decode_lm_head_sample(x, lm, eps, temperature, seeds, steps, ws["keys"],
                                             tokens=ws["tokens"][:B], preshuffled=lm_ps, **lp)
        if logprobs:
            raise RuntimeError("sample_rows: vocab-parallel shards have no logprob epilogue")
        # TP: each rank samples its vocab shard down to one packed key per row (global ids,
        # so the Gumbel noise equals TP=1's); one int64 MAX all-reduce picks the winner
        keys = ops.decode_lm_head_sample(x, lm, eps, temperature, seeds, steps, ws["keys"],
                                         tokens=ws["tp_keys"][:B], finalize="key",
                                         vocab_offset=self.tp_rank * self.vocab_shard,
                                         preshuffled=lm_ps)
        toks = ws["tokens"][:B]
        self.tp_group.all_reduce_max(keys, tokens=toks)  # IPC: one kernel, tokens included
        return toks

    def score_chunk_rows(self) -> int:
        """Rows per launch of ``score_rows``: what the wide kernel takes over a pre-shuffled
        LM head, else what the 16-row-tile GEMV takes."""
        return ops.WIDE_ROWS if self.lm_head_ps is not None else ops.SKINNY_ROWS

    def score_fusable(self, rows: int) -> bool:
        """Can the fused LM head score these rows (``ops.lm_head_score``)?  One GPU, and the
        LM-head kernels with the scoring epilogue, as ``sampler_fusable``."""
        lm_ps = self.lm_head_ps is not None
        return (self.tp_size == 1 and self.device.type == "cuda"
                and self.cfg.hidden_size % 128 == 0
                and ops.fused_kernel(rows, lm_ps, False, "score") is not None)

    def score_rows(self, hidden: torch.Tensor, targets: torch.Tensor, n_top: int,
                   ws: dict | None, fused: bool = True):
        """Teacher-forced scoring: the logprob of token ``targets[r]`` (int32) under row r of
        ``hidden`` (already normalised: eps = 0, as the rows ``forward(rows=...)`` returns),
        and with ``n_top`` >= 1 each row's ``n_top`` most likely tokens with theirs.  Returns
        (lp [R] fp32, top_ids [R, n_top] int32 | None, top_lp [R, n_top] fp32 | None).

        Chunks of at most ``score_chunk_rows`` rows.  ``n_top`` == 0 where the fused route
        exists (``score_fusable``; ``fused=False`` turns it off): ``ops.lm_head_score`` per
        chunk with ``ws["rec"]`` as its record workspace - each chunk streams the LM head once
        and no logits reach memory.  Otherwise per chunk ``compute_logits`` and
        ``ops.token_logprobs``: the logits buffer never exceeds one chunk."""
        R = hidden.shape[0]
        dev = hidden.device
        lp = torch.empty(R, dtype=torch.float32, device=dev)
        top_ids = top_lp = None
        if n_top > 0:
            top_ids = torch.empty(R, n_top, dtype=torch.int32, device=dev)
            top_lp = torch.empty(R, n_top, dtype=torch.float32, device=dev)
        lm_ps = self.lm_head_ps is not None
        step = self.score_chunk_rows()
        tok64 = targets.long() if R else targets
        for r0 in range(0, R, step):
            r1 = min(R, r0 + step)
            chunk = hidden[r0:r1]
            if n_top == 0 and fused and ws is not None and self.score_fusable(r1 - r0):
                ops.lm_head_score(chunk, self.lm_head_ps if lm_ps else self.lm_head, 0.0,
                                  targets[r0:r1], ws["rec"], out=lp[r0:r1], preshuffled=lm_ps)
                continue
            logits = self.compute_logits(chunk)
            got = ops.token_logprobs(logits, tok64[r0:r1], n_top)
            lp[r0:r1].copy_(got[0])
            if n_top > 0:
                top_ids[r0:r1].copy_(got[1])
                top_lp[r0:r1].copy_(got[2])
        return lp, top_ids, top_lp

    def compute_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        logits = ops.linear(hidden, self.lm_head)
        if self.tp_size > 1:
            logits = self.tp_group.all_gather_last(logits)
        return logits


def save_config_json(cfg: ModelConfig, path: str):
    Path(path).write_text(json.dumps(cfg.__dict__, indent=2, default=list))
