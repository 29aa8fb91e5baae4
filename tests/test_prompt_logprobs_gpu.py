"""Prompt logprobs on the GPU: the fused LM head's scoring epilogue (EPI_SCORE + its finalize)
in the 16-row-tile GEMV and the wide kernel, against the materialised chunk route and through
the engine.

Bounds are those of tests/test_logprobs_gpu.py, for its reasons.  Exact-logit cases: every logit
is a multiple of 1/4 with |l| <= 64, exact in bf16 and in the fp32 accumulator, so the expected
values are fp64 ``log_softmax`` of the exact logits and only the kernels' fp32 exp / log / sums
are under test (< 1e-5): 1e-3 absolute.  Random cases: the kernel's and the reference's fp32
products can round to neighbouring bf16 values, one ulp <= 2^-7 |l| on the token's logit and,
as a weighted mean, on logZ: 2^-6 max|l| + 1e-3."""
import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.ops import reference as ref
from test_logprobs_gpu import exact_rows, exact_weights, random_bound
from test_prompt_logprobs import dense_all_logits

pytestmark = pytest.mark.gpu
EXACT_ATOL = 1e-3


def cycle_targets(l64: torch.Tensor) -> torch.Tensor:
    """One target per row, cycling through: id 0, ids 15 and 16 (a tile edge), vocab - 1, the
    row's argmax, the row's argmin, and the previous row's target (shared by two rows)."""
    m, vocab = l64.shape
    t = []
    for r in range(m):
        k = r % 7
        t.append((0, 15, 16, vocab - 1, int(l64[r].argmax()), int(l64[r].argmin()),
                  t[-1] if t else 0)[k])
    return torch.tensor(t, dtype=torch.int32)


def score(x, w, eps, targets, preshuffled, extra=3):
    """ops.lm_head_score into a buffer with ``extra`` NaN rows behind the M results."""
    m, tiles = x.shape[0], w.shape[0] // 16
    wk = ops.preshuffle(w) if preshuffled else w
    ws = torch.zeros(4 * m * tiles, dtype=torch.float32, device="cuda")
    buf = torch.full((m + extra,), float("nan"), device="cuda")
    lp = ops.lm_head_score(x, wk, eps, targets, ws, out=buf, preshuffled=preshuffled)
    torch.cuda.synchronize()
    assert lp.shape == (m,) and lp.data_ptr() == buf.data_ptr()
    return lp.cpu(), buf[m:].cpu()


EXACT_CASES = ([(m, False, 4112) for m in (1, 5, 16, 32)]
               + [(m, True, 4112) for m in (1, 5, 16, 32)]      # 32 pre-shuffled rows: wide
               + [(m, True, 4112) for m in (17, 33, 100, 128)]  # the wide kernel
               + [(5, True, 131200)])                           # finalize loop's second trip


@pytest.mark.parametrize("m,preshuffled,vocab", EXACT_CASES)
def test_fused_exact_logits(m, preshuffled, vocab):
    w, _ = exact_weights(vocab)
    x = exact_rows(m, seed=m)
    # the exactness claim, checked here: fp64 logits are multiples of 1/4 within +-64, bf16
    # holds them, and an fp32 product equals them
    l64 = x.double() @ w.double().t()
    assert bool((l64 * 4 == (l64 * 4).round()).all()) and float(l64.abs().max()) <= 64
    assert torch.equal(l64.to(torch.bfloat16).double(), l64)
    assert torch.equal((x.float() @ w.float().t()).double(), l64)
    expect = torch.log_softmax(l64, dim=-1)
    tgt = cycle_targets(l64)
    want_route = ("wide" if preshuffled and m >= 17 else "skinny")
    assert ops.fused_kernel(m, preshuffled, False, "score") == want_route

    lp, tail = score(x.cuda(), w.cuda(), 0.0, tgt.cuda(), preshuffled)
    assert bool(torch.isnan(tail).all()), "rows past M were written"
    want = expect.gather(1, tgt.long().view(-1, 1)).view(-1)
    err = (lp.double() - want).abs()
    print(f"m={m} ps={preshuffled} vocab={vocab}: max |dlp| = {float(err.max()):.3e}")
    assert float(err.max()) <= EXACT_ATOL


@pytest.mark.parametrize("m,preshuffled", [(5, False), (32, False), (12, True), (33, True),
                                           (128, True)])
def test_fused_random_norm_folded(m, preshuffled):
    torch.manual_seed(200 + m)
    hidden, vocab = 1024, 4096
    x = torch.randn(m, hidden).to(torch.bfloat16)
    w = (torch.randn(vocab, hidden) * 0.05).to(torch.bfloat16)
    tgt = torch.randint(0, vocab, (m,), dtype=torch.int32)
    tgt[0], tgt[-1] = 0, vocab - 1
    lp, tail = score(x.cuda(), w.cuda(), 1e-5, tgt.cuda(), preshuffled)
    assert bool(torch.isnan(tail).all())
    want = ref.lm_head_score(x, w, 1e-5, tgt)
    xn = ref.rms_norm(x, torch.ones(hidden, dtype=x.dtype), 1e-5)
    logits = torch.nn.functional.linear(xn, w)
    bound = torch.tensor([random_bound(float(logits[r].float().abs().max())) for r in range(m)])
    err = (lp - want).abs()
    print(f"m={m} ps={preshuffled}: fused vs reference max |dlp| = {float(err.max()):.3e}, "
          f"bound >= {float(bound.min()):.3e}")
    assert bool((err <= bound).all())
    # the materialised chunk route on the same inputs: norm, LM-head GEMM, the row kernel
    xg, wg = x.cuda(), w.cuda()
    lg = torch.nn.functional.linear(
        ops.rms_norm(xg, torch.ones(hidden, dtype=xg.dtype, device="cuda"), 1e-5), wg)
    mat = ops.token_logprobs(lg, tgt.cuda().long(), 0)[0].cpu()
    err = (lp - mat).abs()
    print(f"m={m} ps={preshuffled}: fused vs materialised max |dlp| = {float(err.max()):.3e}")
    assert bool((err <= bound).all())


def test_op_refuses_what_the_host_can_check():
    x = torch.zeros(40, 256, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(4096, 256, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(4 * 40 * 256, dtype=torch.float32, device="cuda")
    t32 = torch.zeros(40, dtype=torch.int32, device="cuda")
    assert ops.fused_kernel(40, False, False, "score") is None
    assert ops.fused_kernel(129, True, False, "score") is None
    assert ops.fused_kernel(8, True, True, "score") is None       # no fp8 build
    with pytest.raises(ValueError):
        ops.lm_head_score(x, w, 0.0, t32, ws)                     # 40 rows, row-major
    with pytest.raises(ValueError):
        ops.lm_head_score(x[:8], w, 0.0, t32.long(), ws)          # int64 targets
    with pytest.raises(RuntimeError):
        ops.lm_head_score(x[:8], w, 0.0, t32, ws[:64])            # workspace too small


# ---- the engine ----------------------------------------------------------------------------
def _prompt(vocab, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(10, vocab // 2, (n,), generator=g).tolist()


def _engine(model, **kw):
    base = dict(model=model, device="cuda", max_model_len=512, num_kv_blocks=512,
                max_num_seqs=8, startup_warmup=False, enable_prefix_caching=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _check_dense(eng, prompt, out, tag):
    """Every prompt entry against the dense all-rows forward, each under its row's bound."""
    assert len(out.prompt_logprobs) == len(prompt) and out.prompt_logprobs[0] is None
    logits = dense_all_logits(eng.runner.model, list(prompt))
    ls = torch.log_softmax(logits, -1)
    worst, slack = 0.0, float("inf")
    for i in range(1, len(prompt)):
        d = abs(float(ls[i - 1, prompt[i]]) - out.prompt_logprobs[i])
        b = random_bound(float(logits[i - 1].abs().max()))
        worst, slack = max(worst, d), min(slack, b - d)
    print(f"{tag}: max |dlp| = {worst:.3e}, least margin {slack:.3e}")
    assert slack >= 0.0


@pytest.mark.parametrize("model", ["tiny", "llama-8b-slice"])
def test_engine_one_step_three_launches(model):
    eng = _engine(model, max_num_batched_tokens=512)
    assert eng.runner.score_ws is None            # nothing allocated before the first request
    p = _prompt(eng.model_cfg.vocab_size, 300, seed=1)
    eng.add_request("r", p, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                           prompt_logprobs=0))
    assert eng.runner.score_ws is not None and "rec" in eng.runner.score_ws
    outs = eng.step()                             # the whole prompt in one prefill step
    assert len(eng.runner.last_scored) == 299     # 128 + 128 + 43 rows
    assert eng.runner.model.score_chunk_rows() == 128
    assert eng.runner.model.score_fusable(128) and eng.runner.model.score_fusable(43)
    while eng.has_unfinished():
        outs = eng.step()
    _check_dense(eng, p, outs[0], f"{model} 300 tokens")


@pytest.mark.parametrize("model", ["tiny", "llama-8b-slice"])
def test_engine_chunked_prefill(model):
    eng = _engine(model, max_num_batched_tokens=16)
    p = _prompt(eng.model_cfg.vocab_size, 40, seed=2)
    out = eng.generate([p], SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                           prompt_logprobs=0))[0]
    _check_dense(eng, p, out, f"{model} 40 tokens in chunks of 16")


@pytest.mark.parametrize("model", ["tiny", "llama-8b-slice"])
def test_engine_self_consistency_and_top2(model):
    eng = _engine(model, max_num_batched_tokens=512)
    p = _prompt(eng.model_cfg.vocab_size, 21, seed=3)
    gen = eng.generate([p], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True,
                                           logprobs=0))[0]
    full = p + gen.token_ids
    sc = eng.generate([full], SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True,
                                             prompt_logprobs=0))[0]
    logits = dense_all_logits(eng.runner.model, full)
    assert len(sc.prompt_logprobs) == len(full) and len(gen.logprobs) == 8
    for j, lp in enumerate(gen.logprobs):        # nothing skipped: the prompt fixes the tokens
        i = len(p) + j
        bound = random_bound(float(logits[i - 1].abs().max()))
        assert abs(sc.prompt_logprobs[i] - lp) <= bound, (j, sc.prompt_logprobs[i], lp)
    top = eng.generate([full], SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True,
                                              prompt_logprobs=2))[0]
    assert top.prompt_top_logprobs[0] is None and len(top.prompt_top_logprobs) == len(full)
    for i in range(1, len(full)):
        alts = top.prompt_top_logprobs[i]
        assert len(alts) == 2 and alts[0][1] >= alts[1][1]
        assert alts[0][1] >= top.prompt_logprobs[i]
        # the materialised (top-N) route against the fused one
        bound = random_bound(float(logits[i - 1].abs().max()))
        assert abs(top.prompt_logprobs[i] - sc.prompt_logprobs[i]) <= bound


@pytest.mark.parametrize("model", ["tiny", "llama-8b-slice"])
def test_engine_tokens_unchanged_and_no_workspace_unasked(model):
    eng = _engine(model, max_num_batched_tokens=512)
    vocab = eng.model_cfg.vocab_size
    ps = [_prompt(vocab, n, seed=10 + n) for n in (9, 40, 150)]
    kw = dict(temperature=0.0, max_tokens=6, ignore_eos=True)
    off = eng.generate(ps, SamplingParams(**kw))
    assert eng.runner.score_ws is None            # no scoring request seen: no workspace
    assert all(o.prompt_logprobs is None for o in off)
    on = eng.generate(ps, SamplingParams(prompt_logprobs=0, **kw))
    assert [o.token_ids for o in on] == [o.token_ids for o in off]
    assert [len(o.prompt_logprobs) for o in on] == [9, 40, 150]
