"""Per-token logprobs on the GPU: the fused LM head + sampler's logprob epilogue
(EPI_SAMPLE_LP + its finalize), the row kernel over materialised logits
(``ops.token_logprobs``) and both through the engine.

Bounds.  Exact-logit cases: every logit is a multiple of 1/4 with |l| <= 64, exact in bf16
and in the fp32 accumulator, so the expected values are fp64 ``log_softmax`` of the exact
logits and only the kernels' fp32 exp / log / sums are under test: per-thread serial sums of
<= 8 terms plus log-depth trees give ~30 * 2^-24 relative error on the sum and the fast exp's
argument error is <= 64 * 2^-24, both < 1e-5 - the bound is 1e-3 absolute.  Random cases: the
kernel's and the reference's fp32 products can round to neighbouring bf16 values, one ulp
<= 2^-7 |l| on the token's logit and, as a weighted mean, on logZ: 2^-6 max|l| + 1e-3."""
import functools

import pytest
import torch

from agentic_traffic_testing_amd import ops
from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.ops import reference as ref
from helpers import dense_logits

pytestmark = pytest.mark.gpu
EXACT_ATOL = 1e-3
K_EXACT = 256
BLOCKS = ((0, 80), (80, 160), (160, 256))  # x columns of the rows whose winner is plant j


def random_bound(max_abs_logit: float) -> float:
    return 2.0 ** -6 * max_abs_logit + 1e-3


@functools.lru_cache(maxsize=None)
def exact_weights(vocab: int):
    """W [vocab, 256] from {0, +-1/2, +-1, +-2} and the three planted rows (first, a middle
    and the last 16-column tile): all 2 on their own column block, 0 elsewhere."""
    g = torch.Generator().manual_seed(vocab)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    w = vals[torch.randint(0, 7, (vocab, K_EXACT), generator=g)]
    plants = (3, (vocab // 32) * 16 + 5, vocab - 2)
    for (lo, hi), v in zip(BLOCKS, plants):
        w[v] = 0.0
        w[v, lo:hi] = 2.0
    return w.to(torch.bfloat16), plants


def exact_rows(m: int, seed: int):
    """x [m, 256]: 8 values from {1/2, 1, 2} per row inside block (row % 3), so row r's
    largest logit, 2 * sum(x), is its plant's (any other weight row needs all eight 2s)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(m, K_EXACT)
    vals = torch.tensor([0.5, 1.0, 2.0])
    for r in range(m):
        lo, hi = BLOCKS[r % 3]
        pos = lo + torch.randperm(hi - lo, generator=g)[:8]
        x[r, pos] = vals[torch.randint(0, 3, (8,), generator=g)]
    return x.to(torch.bfloat16)


def sampler_inputs(m: int):
    temp = torch.tensor([0.0 if r % 2 == 0 else 0.7 for r in range(m)], device="cuda")
    seeds = torch.arange(11, 11 + m, dtype=torch.long, device="cuda")
    steps = torch.arange(m, dtype=torch.long, device="cuda") % 5
    return temp, seeds, steps


def run_both(x, w, eps, preshuffled):
    """The plain sampler launch and the logprob one on the same inputs: (tokens, keys) of
    each and the logprobs."""
    m, tiles = x.shape[0], w.shape[0] // 16
    wk = ops.preshuffle(w) if preshuffled else w
    temp, seeds, steps = sampler_inputs(m)
    keys_a = torch.zeros(m * tiles, dtype=torch.long, device="cuda")
    keys_b = torch.zeros_like(keys_a)
    lp_ws = torch.zeros(4 * m * tiles, dtype=torch.float32, device="cuda")
    lp = torch.full((m,), float("nan"), device="cuda")
    ta = ops.decode_lm_head_sample(x, wk, eps, temp, seeds, steps, keys_a,
                                   preshuffled=preshuffled).clone()
    tb = ops.decode_lm_head_sample(x, wk, eps, temp, seeds, steps, keys_b,
                                   preshuffled=preshuffled, logprobs=lp, lp_ws=lp_ws).clone()
    torch.cuda.synchronize()
    return ta, keys_a, tb, keys_b, lp, temp


EXACT_CASES = ([(m, False, 4112) for m in (1, 5, 16, 32)]
               + [(m, True, 4112) for m in (1, 5, 16, 32)]      # 32 pre-shuffled rows: wide
               + [(m, True, 4112) for m in (17, 33, 100, 128)]  # the wide kernel
               + [(5, True, 131200)])                           # finalize loop's second trip


@pytest.mark.parametrize("m,preshuffled,vocab", EXACT_CASES)
def test_fused_exact_logits(m, preshuffled, vocab):
    w, plants = exact_weights(vocab)
    x = exact_rows(m, seed=m)
    # the exactness claim, checked here: fp64 logits are multiples of 1/4 within +-64, bf16
    # holds them, and an fp32 product equals them
    l64 = x.double() @ w.double().t()
    assert bool((l64 * 4 == (l64 * 4).round()).all()) and float(l64.abs().max()) <= 64
    assert torch.equal(l64.to(torch.bfloat16).double(), l64)
    assert torch.equal((x.float() @ w.float().t()).double(), l64)
    expect = torch.log_softmax(l64, dim=-1)

    ta, keys_a, tb, keys_b, lp, temp = run_both(x.cuda(), w.cuda(), 0.0, preshuffled)
    assert torch.equal(keys_a, keys_b), "keys differ from the EPI_SAMPLE launch"
    assert torch.equal(ta, tb)
    toks = tb.cpu()
    for r in range(m):
        if float(temp[r]) == 0.0:
            assert int(toks[r]) == plants[r % 3]
    want = expect.gather(1, toks.view(-1, 1)).view(-1)
    err = (lp.cpu().double() - want).abs()
    print(f"m={m} ps={preshuffled} vocab={vocab}: max |dlp| = {float(err.max()):.3e}")
    assert float(err.max()) <= EXACT_ATOL


@pytest.mark.parametrize("m,preshuffled", [(5, False), (32, False), (12, True), (33, True),
                                           (128, True)])
def test_fused_random_norm_folded(m, preshuffled):
    torch.manual_seed(100 + m)
    hidden, vocab = 1024, 4096
    x = torch.randn(m, hidden).to(torch.bfloat16)
    w = (torch.randn(vocab, hidden) * 0.05).to(torch.bfloat16)
    ta, keys_a, tb, keys_b, lp, _ = run_both(x.cuda(), w.cuda(), 1e-5, preshuffled)
    assert torch.equal(keys_a, keys_b) and torch.equal(ta, tb)
    # ops.reference on the kernel's own tokens (a near tie may pick its neighbour)
    xn = ref.rms_norm(x, torch.ones(hidden, dtype=x.dtype), 1e-5)
    logits = torch.nn.functional.linear(xn, w)
    want = ref.token_logprobs(logits, tb.cpu(), 0)[0]
    err = (lp.cpu() - want).abs()
    bound = torch.tensor([random_bound(float(logits[r].float().abs().max())) for r in range(m)])
    print(f"m={m} ps={preshuffled}: max |dlp| = {float(err.max()):.3e}, "
          f"bound >= {float(bound.min()):.3e}")
    assert bool((err <= bound).all())


# ---- the row kernel ---------------------------------------------------------------------
TIE_AT = (7, 8, 511, 512, 4095, 8191, 8192, 65535, 65536)  # thread / wave / pass boundaries


@functools.lru_cache(maxsize=None)
def row_case(vocab: int, rows: int):
    """Exact bf16 logits (multiples of 1/4 in [-16, 16]) with the row maximum 20 tied across
    thread, wave and workgroup-pass boundaries and at the row's end, and a second tier of
    ties below it; the reference over them, for every N at once."""
    g = torch.Generator().manual_seed(vocab * 64 + rows)
    l = torch.randint(-64, 65, (rows, vocab), generator=g).float() / 4
    top = [i for i in TIE_AT if i < vocab] + [vocab - 1]
    for r in range(rows):
        l[r, top[r % 3:]] = 20.0              # rows differ in how many ties lead
        l[r, [i + 2 for i in top[:4]]] = 19.75
    tokens = torch.tensor([top[-1] if r % 2 == 0 else 50 + r for r in range(rows)])
    for r in range(1, rows, 2):
        l[r, 50 + r] = -10.0                  # an odd row's token is far from its top-N
    lb = l.to(torch.bfloat16)
    assert torch.equal(lb.float(), l)
    return lb, tokens, ref.token_logprobs(lb, tokens, ops.MAX_TOP_LOGPROBS)


@pytest.mark.parametrize("vocab", [4096, 4112, 128256])
@pytest.mark.parametrize("rows", [1, 12, 40])
def test_row_kernel(vocab, rows):
    lb, tokens, (lp_ref, ids_ref, top_ref) = row_case(vocab, rows)
    lg, tg = lb.cuda(), tokens.cuda()
    for n in (1, 5, 20):
        lp, ids, top = ops.token_logprobs(lg, tg, n)
        assert ids.shape == (rows, n) and ids.dtype == torch.int32
        assert torch.equal(ids.cpu(), ids_ref[:, :n]), f"N={n}: ids / tie order"
        assert float((top.cpu() - top_ref[:, :n]).abs().max()) <= EXACT_ATOL
        assert float((lp.cpu() - lp_ref).abs().max()) <= EXACT_ATOL
    # the sampled token is reported whether or not it is among the alternatives
    inside = [bool((ids_ref[r] == tokens[r]).any()) for r in range(rows)]
    assert inside[0] and (rows == 1 or not inside[1])


def test_row_kernel_unaligned_and_fp32():
    """A row base off the 16-B grid takes the element-wise loads; fp32 logits the float4 ones."""
    lb, tokens, _ = row_case(4112, 12)
    sl = lb.cuda()[:, 1:]                     # stride 4112, base + 2 bytes
    tok = (tokens - 1).cuda()
    want = ref.token_logprobs(lb[:, 1:], tokens - 1, 5)
    for logits in (sl, sl.float().contiguous()):
        lp, ids, top = ops.token_logprobs(logits, tok, 5)
        assert torch.equal(ids.cpu(), want[1])
        assert float((lp.cpu() - want[0]).abs().max()) <= EXACT_ATOL
        assert float((top.cpu() - want[2]).abs().max()) <= EXACT_ATOL


def test_row_kernel_signed_zero():
    """-0 and +0 are one logit: among equal logits the lower id leads, whatever the sign bit."""
    l = torch.full((2, 4096), -5.0)
    l[0, 50], l[0, 100] = -0.0, 0.0
    l[1, 50], l[1, 100] = 0.0, -0.0
    _, ids, top = ops.token_logprobs(l.to(torch.bfloat16).cuda(),
                                     torch.zeros(2, dtype=torch.long, device="cuda"), 2)
    assert ids.cpu().tolist() == [[50, 100], [50, 100]]
    assert float((top[:, 0] - top[:, 1]).abs().max()) == 0.0


# ---- the engine ----------------------------------------------------------------------------
def _prompts(vocab, sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(10, vocab // 2, (n,), generator=g).tolist() for n in sizes]


def _engine(model, **kw):
    base = dict(model=model, device="cuda", max_model_len=512, num_kv_blocks=512,
                max_num_seqs=8, startup_warmup=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def _teacher_forced(eng, prompt, out):
    """(max |dlp|, bound) of one request against the dense forward, position by position."""
    ids, worst, bound = list(prompt), 0.0, float("inf")
    for t, lp in zip(out.token_ids, out.logprobs):
        logits = dense_logits(eng.runner.model, ids)
        want = float(torch.log_softmax(logits, -1)[t])
        worst = max(worst, abs(want - lp))
        bound = min(bound, random_bound(float(logits.abs().max())))
        ids.append(t)
    return worst, bound


@pytest.mark.parametrize("model", ["tiny", "llama-8b-slice"])
def test_engine_graph_equals_eager_and_variants(model):
    outs = {}
    for graphs in (True, False):
        eng = _engine(model, use_graphs=graphs)
        vocab = eng.model_cfg.vocab_size
        prompts = _prompts(vocab, (9, 17, 5))
        for n in (0, 1):
            sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True, logprobs=n)
            outs[graphs, n] = eng.generate(prompts, sp)
        if graphs:
            assert eng.runner.graph_steps > 0
            variants = {k[2] for k in eng.runner.graphs}
            assert {2, 4} <= variants  # sampled-only and top-N graphs, captured on first use
    for n in (0, 1):
        for a, b in zip(outs[True, n], outs[False, n]):
            assert a.token_ids == b.token_ids
            assert a.logprobs == b.logprobs, "graph replay != eager"
            assert a.top_logprobs == b.top_logprobs
    # fused variant (logprobs=0) against the materialised one (logprobs=1), while both
    # sampled the same tokens (a near tie may part them)
    compared = 0
    for p, a, b in zip(prompts, outs[True, 0], outs[True, 1]):
        assert len(a.logprobs) == len(a.token_ids) == 6 and len(b.top_logprobs) == 6
        assert all(len(alts) == 1 and alts[0][0] == t      # greedy: the top-1 is the token
                   for alts, t in zip(b.top_logprobs, b.token_ids))
        ids = list(p)
        for i, (ta, tb) in enumerate(zip(a.token_ids, b.token_ids)):
            if ta != tb:
                break
            bound = random_bound(float(dense_logits(eng.runner.model, ids).abs().max()))
            assert abs(a.logprobs[i] - b.logprobs[i]) <= bound
            assert abs(b.top_logprobs[i][0][1] - b.logprobs[i]) == 0.0
            ids.append(ta)
            compared += 1
    assert compared >= 6


@pytest.mark.parametrize("model", ["tiny", "llama-8b-slice"])
def test_engine_teacher_forced_async_mixed(model):
    """async look-ahead on, three requests of which one did not ask: entry i is token i's."""
    eng = _engine(model, async_decode=True)
    prompts = _prompts(eng.model_cfg.vocab_size, (11, 6, 20), seed=1)
    sps = [SamplingParams(temperature=0.8, max_tokens=8, ignore_eos=True, seed=5, logprobs=0),
           SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True),
           SamplingParams(temperature=0.0, max_tokens=5, ignore_eos=True, logprobs=4)]
    outs = eng.generate(prompts, sps)
    assert eng.timing["lookahead_steps"] > 0
    assert outs[1].logprobs is None and outs[1].top_logprobs is None
    for p, o in ((prompts[0], outs[0]), (prompts[2], outs[2])):
        assert len(o.logprobs) == len(o.token_ids)
        worst, bound = _teacher_forced(eng, p, o)
        print(f"{model}: max |dlp| = {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound
    assert all(len(alts) == 4 for alts in outs[2].top_logprobs)
    assert all(a[0][1] >= a[1][1] >= a[2][1] >= a[3][1] for a in outs[2].top_logprobs)


def test_engine_teacher_forced_wide_batch():
    """48 sequences decode through the wide kernel's logprob epilogue."""
    eng = _engine("llama-8b-slice", max_num_seqs=48, num_kv_blocks=1024,
                  max_num_batched_tokens=1024)
    prompts = _prompts(eng.model_cfg.vocab_size, [5 + (i % 7) for i in range(48)], seed=2)
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True,
                                                logprobs=0))
    assert max(eng.batch_size_history) == 48
    worst = 0.0
    for p, o in zip(prompts, outs):
        w, bound = _teacher_forced(eng, p, o)
        assert w <= bound
        worst = max(worst, w)
    print(f"B=48: max |dlp| = {worst:.3e}")
