"""Dense fp32 oracle of an MXFP4 model with fp8 activations (mxfp4_fp8_activations), shared by
tests/test_w4a8.py (CPU engine) and tests/test_w4a8_gpu.py.

The engine runs a prompt of more than 128 rows through the activation-quantised chain: the
input of each of the four projections is rounded per token to e4m3 (ops.quant_rows_fp8) and
multiplied by the MXFP4 weight values in fp32; later (decode) rows keep 16-bit activations.
The oracle does the same on ``model.dense_weight`` copies: rows [0, n_prompt) pass through
``helpers._qdq_rows`` at the four quantisation points, as ``helpers.dense_logits_fp8`` does for
fp8 weights."""
import numpy as np
import torch
import torch.nn.functional as F

from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.ops import reference as ref

from helpers import _qdq_rows

PROJS = ("qkv", "o", "gate_up", "down")
TOL_LOGIT = 0.3       # a token that is not the oracle's argmax must be within this many logits
PROMPT_ROWS = (160, 300)
# Seeds for which the CPU engine - the reference arithmetic of the mode - agrees with the
# oracle's argmax at every generated position (test_w4a8.test_cpu_engine_tokens asserts it), so
# the one-in-five cap of check() hides nothing there.
PROMPT_SEED = 0
MAX_TOKENS = 6


def prompts(rows=PROMPT_ROWS, seed=PROMPT_SEED, vocab=30000):
    rng = np.random.default_rng(seed)
    return [rng.integers(300, vocab, size=n).tolist() for n in rows]


def dense_weights(model):
    """{(layer, proj): fp32 dense weight} from model.dense_weight (whatever copies it holds)."""
    return {(i, p): model.dense_weight(i, p).float()
            for i in range(len(model.layers)) for p in PROJS}


@torch.no_grad()
def dense_logits_w4a8(model, W, ids, n_quant):
    """Last-row logits of the full-sequence causal forward in fp32; rows [0, n_quant) see e4m3
    activations at the inputs of qkv, o, gate_up and down, the SiLU-mul of those rows on the
    unrounded fp32 gate / up values (the GEMM's epilogue), and each o / down product rounded to
    the model dtype before it joins the residual (the chain adds it in the next norm kernel)."""
    c = model.cfg
    dev = model.embed.device
    dt = model.dtype
    x = F.embedding(torch.tensor(ids, device=dev), model.embed).float()
    T = len(ids)
    D = model.head_dim
    nq, nkv = model.n_heads, model.n_kv_heads
    pos = torch.arange(T, device=dev)
    mask = torch.triu(torch.ones(T, T, dtype=torch.bool, device=dev), 1)[None]
    P = min(n_quant, T)
    rnd = lambda t: t.to(dt).float()  # noqa: E731
    for i, L in enumerate(model.layers):
        h = _qdq_rows(ref.rms_norm(x, L.input_norm.float(), c.rms_norm_eps), P)
        qkv = rnd(h @ W[i, "qkv"].t())
        q = qkv[:, :nq * D].view(T, nq, D)
        k = qkv[:, nq * D:(nq + nkv) * D].view(T, nkv, D)
        v = qkv[:, (nq + nkv) * D:(nq + 2 * nkv) * D].view(T, nkv, D)
        q = ref.rope_rotate(q, pos, model.cos_sin)
        k = ref.rope_rotate(k, pos, model.cos_sin)
        kk = k.float().repeat_interleave(model.g, 1)
        vv = v.float().repeat_interleave(model.g, 1)
        s = torch.einsum("qhd,khd->hqk", q.float(), kk) * model.scale
        s = s.masked_fill(mask, float("-inf"))
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), vv)
        a = _qdq_rows(rnd(a.reshape(T, -1)), P)
        y = a @ W[i, "o"].t()
        x = rnd(x + torch.cat([rnd(y[:P]), y[P:]]))
        h = _qdq_rows(ref.rms_norm(x, L.post_norm.float(), c.rms_norm_eps), P)
        gu = h @ W[i, "gate_up"].t()
        gu = torch.cat([gu[:P], rnd(gu[P:])])
        g = _qdq_rows(rnd(ref.silu_and_mul(gu)), P)
        y = g @ W[i, "down"].t()
        x = rnd(x + torch.cat([rnd(y[:P]), y[P:]]))
    x = ref.rms_norm(x, model.norm.float(), c.rms_norm_eps)
    return (x[-1:] @ model.lm_head.float().t())[0]


def check(eng, prompt_list, max_tokens=MAX_TOKENS, chain_min_rows=129):
    """Greedy tokens of ``eng``, every position teacher-forced against the oracle: a token that
    is not its argmax must be within TOL_LOGIT, and at most one position in five may diverge.
    Returns (token lists, divergent positions)."""
    sp = SamplingParams(temperature=0.0, max_tokens=max_tokens, ignore_eos=True)
    outs = [eng.generate([p], sp)[0] for p in prompt_list]  # each prompt alone in its step
    model = eng.runner.model
    W = dense_weights(model)
    bad = checked = 0
    for p, o in zip(prompt_list, outs):
        assert len(o.token_ids) == max_tokens
        ids = list(p)
        nq = len(p) if len(p) >= chain_min_rows else 0
        for got in o.token_ids:
            lg = dense_logits_w4a8(model, W, ids, nq)
            checked += 1
            if int(torch.argmax(lg)) != got:
                gap = float(lg.max() - lg[got])
                assert gap < TOL_LOGIT, (o.token_ids, len(ids) - len(p), gap)
                bad += 1
            ids.append(got)
    assert bad <= checked // 5, (bad, checked)
    return [o.token_ids for o in outs], bad
