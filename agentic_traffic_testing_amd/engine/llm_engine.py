"""Synchronous serving engine: scheduler + model runner + stop handling.

The reference drives vLLM's ``AsyncLLMEngine.generate`` (llm/serve_llm.py:504-612); this
engine provides the same contract (prompt in, streamed outputs, TTFT = time to the first
yielded output) on the MI355X-native runner.  ``async_engine.AsyncEngine`` wraps it with
a background step loop for the HTTP front end.
"""
from __future__ import annotations

import random
import threading
import time
from dataclasses import dataclass, field

import numpy as np

from ..config import EngineConfig, resolve_model
from ..utils import roctx
from .guided import START, Guide, GuideCompiler
from .model_runner import ModelRunner
from .scheduler import Batch, Scheduler
from .sequence import SamplingParams, Sequence, SeqStatus
from .spec_decode import Proposer, make_proposer
from .tokenizer import get_tokenizer

PENDING_TOKEN = -1  # output slot of a launched step whose token the host has not seen yet


@dataclass
class RequestOutput:
    request_id: str
    token_ids: list
    finished: bool
    finish_reason: str | None = None
    prompt_tokens: int = 0
    cached_prompt_tokens: int = 0
    arrival_time: float = 0.0
    first_token_time: float | None = None
    first_scheduled_time: float | None = None
    finish_time: float | None = None
    new_token_ids: list = field(default_factory=list)
    # SamplingParams.logprobs set: one entry per entry of token_ids (the first token, which
    # comes out of the prefill step, included) - the token's logprob, and its position's
    # [(token id, logprob), ...] alternatives, most likely first (empty lists for logprobs=0)
    logprobs: list | None = None
    top_logprobs: list | None = None
    # SamplingParams.prompt_logprobs set: one entry per prompt token - None for the first, then
    # log p(prompt[i] | prompt[:i]) - and None, then each position's [(token id, logprob), ...]
    # alternatives (empty lists for prompt_logprobs=0).  Complete once the prompt is prefilled,
    # i.e. in every output that carries a token.
    prompt_logprobs: list | None = None
    prompt_top_logprobs: list | None = None

    @property
    def completion_tokens(self) -> int:
        return len(self.token_ids)

    @property
    def ttft(self) -> float | None:
        if self.first_token_time is None:
            return None
        return self.first_token_time - self.arrival_time

    @property
    def queue_wait(self) -> float | None:
        if self.first_scheduled_time is None:
            return None
        return self.first_scheduled_time - self.arrival_time


@dataclass
class StepStats:
    num_seqs: int
    num_tokens: int
    num_decode: int
    seconds: float


@dataclass
class _Inflight:
    batch: object
    handle: dict
    marks: list      # (seq, output index of this step's token, num_computed after it)
    t0: float


class LLMEngine:
    def __init__(self, cfg: EngineConfig, runner: ModelRunner | None = None, device=None):
        self.cfg = cfg
        self.model_cfg, weights_dir = resolve_model(cfg.model)
        self.tokenizer = get_tokenizer(weights_dir or cfg.model, self.model_cfg.vocab_size)
        dev = device or cfg.device
        self.runner = runner or ModelRunner(cfg, self.model_cfg, dev, weights_dir=weights_dir)
        self.scheduler = Scheduler(self.runner.bm, cfg.max_num_seqs, cfg.max_num_batched_tokens,
                                   cfg.max_model_len, cfg.long_prefill_token_threshold)
        self.eos_ids = set(self.model_cfg.eos_token_ids) | {self.tokenizer.eos_token_id}
        self.lock = threading.RLock()
        self.last_step: StepStats | None = None
        self.total_steps = 0
        self.total_generated = 0
        self.total_prompt = 0
        self.batch_size_history: list = []
        # host-side step breakdown (seconds): scheduler, runner.execute (prep + GPU + sync),
        # output processing
        self.timing = {"schedule": 0.0, "execute": 0.0, "post": 0.0, "steps": 0,
                       "lookahead_steps": 0}
        self._rng = random.Random(cfg.seed)
        # async look-ahead decode: the step launched but not yet collected (see step())
        self._inflight: _Inflight | None = None
        self._last_collect = 0.0
        # speculative decoding (cfg.speculative): the draft proposer - settable, None = off -
        # and its counters (verify steps run, draft tokens verified, drafts accepted)
        self.proposer: Proposer | None = make_proposer(cfg)
        self.spec_stats = {"verify_steps": 0, "draft_tokens": 0, "accepted_tokens": 0}
        # guided decoding: the guide compiler and its cache, built with the first guided request
        self._guides: GuideCompiler | None = None
        self._guides_lock = threading.Lock()
        # (a TP engine warms up itself once its worker group is fully set up)
        if cfg.startup_warmup and self.runner.is_cuda and not getattr(self, "_defer_warmup",
                                                                      False):
            self.warmup()

    def warmup(self) -> None:
        """Serve throw-away requests of the fan-out workload's step shapes - a 17-row
        planning step, a 5 x 17-row burst (wide kernel), 200 / 600-row prefills (mid-M kernel
        + tuned library GEMMs), a long prefill (library + flash prefill tiles), their decode
        steps and one top-k / top-p sampled request - then drop their prefix-cache entries
        and reset the engine's statistics and request-seed stream.  Every code object those
        paths reach (HIP translation units, PyTorch kernels, library solutions) is then loaded
        before the first real request: bench/coldstart.py measures first vs repeat TTFT per
        shape."""
        r = self.runner
        room = min(self.cfg.max_model_len - 8,
                   r.num_blocks * r.block_size // 2, self.cfg.max_num_batched_tokens * 4)
        vocab = max(8, min(self.model_cfg.vocab_size, 32000))
        rng = np.random.default_rng(0)

        def toks(n):
            return rng.integers(min(1000, vocab // 2), vocab, size=n).tolist()

        greedy = SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True)
        t0 = time.perf_counter()
        shapes = [[17], [17] * 5] + [[n] for n in (200, 600, 3000) if n <= room]
        for sizes in shapes:
            if sum(sizes) <= room:
                self.generate([toks(n) for n in sizes], greedy)
        self.generate([toks(17)], SamplingParams(temperature=0.7, top_p=0.9, top_k=40,
                                                 max_tokens=2, ignore_eos=True, seed=1))
        if self.proposer is not None and r.verify_rows() > 0:
            # one verify step, so the multi-query attention's code object (and the fused
            # kernels at its row count) load before the first request: drafts that repeat the
            # last token, whatever the samples turn out to be
            live, self.proposer = self.proposer, _RepeatProposer()
            try:
                self.generate([toks(17)] * 2, SamplingParams(temperature=0.0, max_tokens=6,
                                                              ignore_eos=True))
            finally:
                self.proposer = live
            self.spec_stats = {k: 0 for k in self.spec_stats}
        r.reset_state()
        self.total_steps = self.total_generated = self.total_prompt = 0
        self.batch_size_history = []
        self.last_step = None
        self.timing = {k: (0 if k.endswith("steps") else 0.0) for k in self.timing}
        self._rng = random.Random(self.cfg.seed)
        self.warmup_seconds = time.perf_counter() - t0

    # ------------------------------------------------------------------------------------
    def check_sampling(self, sampling: SamplingParams) -> None:
        """Raise ValueError for sampling parameters this engine cannot serve: a bad field
        (``SamplingParams.check``, with this model's vocabulary bounding the logit_bias keys),
        or a penalised request on a tensor-parallel engine - the token counts live in one
        process's device memory; a TP group would need the state replicated per rank and a
        seeding message to the workers."""
        sampling.check(self.model_cfg.vocab_size)
        if sampling.penalised and self.runner.tp_size > 1:
            raise ValueError("presence_penalty, frequency_penalty, repetition_penalty and "
                             "logit_bias are not served by a tensor-parallel engine")
        if sampling.guided and self.runner.tp_size > 1:
            # the automaton states live in one process's device memory, as the counts do
            raise ValueError("guided_regex, guided_choice and guided_json are not served by a "
                             "tensor-parallel engine")
        if sampling.prompt_logprobs is not None and self.runner.tp_size > 1:
            # the step message carries no score fields and the shards have no merge
            raise ValueError("prompt_logprobs is not served by a tensor-parallel engine")

    def compile_guide(self, sampling: SamplingParams) -> Guide | None:
        """The compiled guide of ``sampling`` (None without one), from the cache or compiled
        now - ``ValueError`` for a pattern or schema outside the dialect, a guide larger than
        the pool, or ignore_eos with a pattern that can only end.  Thread-safe and free of
        engine state: the HTTP front end calls it in an executor before it submits a request,
        so that a compile never runs on the engine thread between two decode steps."""
        self.check_sampling(sampling)
        if not sampling.guided:
            return None
        with self._guides_lock:
            if self._guides is None:
                self._guides = GuideCompiler(
                    self.tokenizer.token_bytes(), self.model_cfg.vocab_size, self.eos_ids,
                    max_states=self.cfg.guided_pool_states - 1)
        return self._guides.compile(sampling)

    def add_request(self, request_id: str, prompt_ids, sampling: SamplingParams,
                    arrival_time: float | None = None) -> Sequence:
        guide = self.compile_guide(sampling)  # (checks the parameters; a cache hit after /chat)
        if sampling.penalised:
            with self.lock:  # device state on first need - here, never inside a graph capture
                self.runner.ensure_penalty_state()
        if sampling.prompt_logprobs is not None:
            with self.lock:  # the scoring workspace likewise
                self.runner.ensure_score_state()
        ids = list(map(int, prompt_ids))
        if not ids:
            ids = [self.tokenizer.bos_token_id]
        limit = self.cfg.max_model_len - 1
        if len(ids) > limit:
            ids = ids[:limit]
        seq = Sequence(request_id=request_id, prompt_ids=ids, sampling=sampling)
        if arrival_time is not None:
            seq.arrival_time = arrival_time
        seq.seed = sampling.seed if sampling.seed is not None else self._rng.getrandbits(62)
        with self.lock:
            if guide is not None:
                # device state on first need, then the guide's rows in the pool (ValueError if
                # it has no room: the request is not queued)
                self.runner.guide_reserve(seq.seq_id, guide)
                seq.guide, seq.guide_state = guide, START
            self.scheduler.add(seq)
        return seq

    def abort(self, request_id: str):
        with self.lock:
            for seq in self.scheduler.abort(request_id):
                self.runner.penalty_release(seq.seq_id)
                self.runner.guide_release(seq.seq_id)

    def _finish(self, seq: Sequence, reason: str) -> None:
        self.scheduler.finish(seq, reason)
        self.runner.penalty_release(seq.seq_id)  # (a no-op for an unpenalised sequence)
        self.runner.guide_release(seq.seq_id)    # (and for an unguided one)

    def _guide_step(self, seq: Sequence, tok: int, idx: int) -> bool:
        """Advance a guided sequence's host shadow state by output token ``idx`` = ``tok``.
        A token the host table does not allow (the device mask and the host table disagree:
        a bug, never a property of the model) fails the request: the token and everything after
        it are dropped, the sequence finishes with reason "error" and False is returned."""
        if seq.guide is None:
            return True
        nxt = seq.guide.advance(seq.guide_state, tok)
        if nxt >= 0:
            seq.guide_state = nxt
            return True
        del seq.output_ids[idx:]
        seq._ids_np = None
        self._finish(seq, "error")
        return False

    def has_unfinished(self) -> bool:
        return self.scheduler.has_work() or self._inflight is not None

    # ------------------------------------------------------------------------------------
    def step(self) -> list[RequestOutput]:
        """One engine step; returns the outputs it produced.

        Async look-ahead decode (``EngineConfig.async_decode``): a decode-only graph step is
        launched, then - before the host waits for its tokens - the step that continues
        every one of its sequences is launched too, its input tokens taken on the device
        from the first step's samples (``ops.embed`` feed_prev path).  The host's scheduling,
        metadata packing and output processing then overlap the GPU instead of sitting
        between two replays.  Look-ahead stops (one plain step drains it) whenever requests
        are waiting for admission, a sequence finishes by length, or the KV pool is full,
        so outputs are identical to the synchronous engine: a look-ahead token of a sequence
        that stopped on EOS is discarded."""
        with self.lock:
            if self._inflight is None:
                ts = time.perf_counter()
                with roctx.range("engine.schedule"):
                    batch = self.scheduler.schedule()
                for seq in batch.preempted:  # re-seeded from its outputs when it comes back
                    self.runner.penalty_release(seq.seq_id)
                    self.runner.guide_release(seq.seq_id, keep_guide=True)
                if batch.empty:
                    return []
                t0 = time.perf_counter()
                self.timing["schedule"] += t0 - ts
                if self.proposer is not None:
                    # speculation on: no async look-ahead (it would need the token that
                    # drafting needs); a step without drafts is a plain synchronous step
                    drafts = self._drafts(batch)
                    if drafts is not None:
                        with roctx.range("engine.verify_step"):
                            return self._verify_step(batch, drafts, t0)
                if self.proposer is not None or not (self.cfg.async_decode
                                                     and self.runner.launchable(batch)):
                    with roctx.range("engine.sync_step" if batch.num_decode == len(batch.seqs)
                                     else "engine.prefill_step"):
                        return self._sync_step(batch, t0)
                with roctx.range("engine.launch"):
                    self._inflight = self._launch(batch, lookahead=False)
            cur = self._inflight
            nxt = self._lookahead_batch(cur)
            if nxt is not None:
                with roctx.range("engine.launch_lookahead"):
                    self._inflight = self._launch(nxt, lookahead=True)
            else:
                self._inflight = None
            with roctx.range("engine.collect"):
                return self._collect(cur)

    def _launch(self, batch, lookahead: bool) -> "_Inflight":
        t0 = time.perf_counter()
        h = self.runner.launch(batch, lookahead=lookahead)  # metadata from pre-step state
        marks = []
        for seq in batch.seqs:
            seq.num_computed += 1
            marks.append((seq, len(seq.output_ids), seq.num_computed))
            seq.append(PENDING_TOKEN)  # filled in by _collect
        if lookahead:
            self.timing["lookahead_steps"] += 1
        return _Inflight(batch, h, marks, t0)

    def _lookahead_batch(self, cur: "_Inflight"):
        """The decode batch continuing ``cur`` row for row, or None to drain."""
        if not self.cfg.async_decode or self.scheduler.waiting:
            return None
        for seq, idx, _ in cur.marks:
            if seq.status != SeqStatus.RUNNING:
                return None
            if idx + 1 >= seq.sampling.max_tokens or \
                    seq.num_prompt + idx + 1 >= self.cfg.max_model_len:
                return None  # finishes by length at cur: nothing to look ahead for
        for seq in cur.batch.seqs:
            if not self.runner.bm.ensure(seq.seq_id, seq.num_tokens):
                return None  # KV pool full: the scheduler decides (preemption)
        n = len(cur.batch.seqs)
        return Batch(seqs=list(cur.batch.seqs), q_start=[s.num_computed for s in cur.batch.seqs],
                     q_len=[1] * n, num_decode=n)

    def _collect(self, cur: "_Inflight") -> list[RequestOutput]:
        toks = self.runner.collect(cur.handle)
        lps = self.runner.collect_logprobs(cur.handle)  # row i belongs to token i
        now = time.perf_counter()
        self.timing["execute"] += now - max(cur.t0, self._last_collect)
        self._last_collect = now
        self.timing["steps"] += 1
        outs = []
        for row, ((seq, idx, ncomp), tok) in enumerate(zip(cur.marks, toks)):
            if seq.status == SeqStatus.FINISHED:
                continue  # aborted while in flight
            tok = int(tok)
            seq.output_ids[idx] = tok
            seq._ids_np = None
            self._record_logprob(seq, idx, lps, row)
            if seq.first_token_time is None:
                seq.first_token_time = now
            if not self._guide_step(seq, tok, idx):
                outs.append(self._output(seq, []))
                continue
            self.runner.bm.commit(seq.seq_id, seq.token_array(), ncomp)
            reason = self._stop_reason(seq, tok, idx + 1)
            if reason:
                del seq.output_ids[idx + 1:]  # drop a look-ahead placeholder
                seq._ids_np = None
                self._finish(seq, reason)
            outs.append(self._output(seq, [tok], upto=idx + 1))
        self._account(cur.batch, len(outs), now - cur.t0)
        self.timing["post"] += time.perf_counter() - now
        return outs

    def _record_prompt_logprobs(self) -> None:
        """Store the last executed step's prompt logprobs with their sequences (each entry
        once, in position order: ``Sequence.set_prompt_logprob``)."""
        res = self.runner.last_prompt_logprobs
        if res is None:
            return
        lp, ids, vals = res
        for k, (seq, idx, _) in enumerate(self.runner.last_scored):
            seq.set_prompt_logprob(idx, lp[k], ((), ()) if ids is None else (ids[k], vals[k]))

    @staticmethod
    def _record_logprob(seq: Sequence, idx: int, lps, row: int) -> None:
        """Store row ``row`` of a step's logprob arrays as output token ``idx`` of a sequence
        that asked for logprobs (a step runs the mode of its most demanding sequence; the
        others get nothing)."""
        if seq.logprobs is None:
            return
        lp, ids, vals = lps
        seq.set_logprob(idx, lp[row], ((), ()) if ids is None else (ids[row], vals[row]))

    def _account(self, batch, n_out: int, seconds: float):
        self.total_steps += 1
        self.total_generated += n_out
        self.last_step = StepStats(len(batch.seqs), batch.num_tokens, batch.num_decode, seconds)
        self.batch_size_history.append(len(batch.seqs))
        if len(self.batch_size_history) > 4096:
            del self.batch_size_history[:2048]

    def _sync_step(self, batch, t0: float) -> list[RequestOutput]:
        with self.lock:
            toks = self.runner.execute(batch)
            lps = self.runner.last_logprobs
            self._record_prompt_logprobs()
            now = time.perf_counter()
            self.timing["execute"] += now - t0
            self.timing["steps"] += 1
            outs = []
            for row, (seq, n, tok) in enumerate(zip(batch.seqs, batch.q_len, toks)):
                seq.num_computed += n
                if seq.num_computed < seq.num_tokens:
                    self.runner.bm.commit(seq.seq_id, seq.token_array(), seq.num_computed)
                    continue  # chunked prefill not finished: sampled token discarded
                tok = int(tok)
                seq.append(tok)
                # (a prefill recomputed after a preemption lands here too: one entry, for the
                # one newly sampled token)
                self._record_logprob(seq, len(seq.output_ids) - 1, lps, row)
                if seq.first_token_time is None:
                    seq.first_token_time = now
                if not self._guide_step(seq, tok, len(seq.output_ids) - 1):
                    outs.append(self._output(seq, []))
                    continue
                self.runner.bm.commit(seq.seq_id, seq.token_array(), seq.num_computed)
                reason = self._stop_reason(seq, tok)
                if reason:
                    self._finish(seq, reason)
                outs.append(self._output(seq, [tok]))
            self._account(batch, len(outs), now - t0)
            self.timing["post"] += time.perf_counter() - now
            return outs

    # -- speculative decoding -------------------------------------------------------------
    def _drafts(self, batch) -> list | None:
        """Draft tokens per sequence of a decode-only batch, or None when no sequence gets one
        (the step is then a plain decode step).  Sequence i gets k_i <= min(spec_tokens,
        16 // G - 1, max_tokens - n - 1, room to max_model_len) tokens of the proposer, none if
        the KV pool cannot hold them (drafts never preempt); the step's rows are kept within
        the runner's cap by trimming the longest draft, lowest batch index first."""
        r = self.runner
        S = len(batch.seqs)
        cap = r.verify_rows()
        if not (0 < S == batch.num_decode and S < cap) or any(n != 1 for n in batch.q_len):
            return None
        if r.is_cuda and r._special(batch):
            return None  # a top-k / top-p row: the whole step samples through that kernel
        if any(seq.sampling.logprobs is not None for seq in batch.seqs):
            return None  # logprobs come from plain decode steps (verify rows record none)
        if r._penalised(batch):
            return None  # a verify row's counts would depend on which drafts are accepted
        if r._guided(batch):
            return None  # a verify row's automaton state would depend on the rows before it
        if any(seq.scoring for seq in batch.seqs):
            return None  # a one-token chunk of a prompt that is being scored
        max_kv = r.verify_max_kv(S)
        if any(seq.num_tokens > max_kv for seq in batch.seqs):
            return None
        drafts = []
        for seq in batch.seqs:
            n = len(seq.output_ids)
            k = min(r.spec_tokens, seq.sampling.max_tokens - n - 1,
                    self.cfg.max_model_len - seq.num_tokens - 1, max_kv - seq.num_tokens)
            d = list(self.proposer.propose(seq, k))[:k] if k > 0 else []
            if d and not r.bm.ensure(seq.seq_id, seq.num_tokens + len(d)):
                d = []
            drafts.append([int(t) for t in d])
        rows = S + sum(len(d) for d in drafts)
        while rows > cap:
            i = max(range(S), key=lambda j: (len(drafts[j]), -j))
            drafts[i].pop()
            rows -= 1
        return drafts if any(drafts) else None

    def _verify_step(self, batch, drafts: list, t0: float) -> list[RequestOutput]:
        """Rows [o_{n-1}, d_1 .. d_k] give samples s_0 .. s_k; with a the largest value such
        that d_i == s_{i-1} for all i <= a, the tokens s_0 .. s_a are what plain decode would
        have produced: they are emitted in order, cut at the first stop.  The KV of rejected
        rows is overwritten by later steps; the prefix cache sees accepted tokens only."""
        with self.lock:
            vb = Batch(seqs=list(batch.seqs), q_start=list(batch.q_start),
                       q_len=[1 + len(d) for d in drafts], num_decode=len(batch.seqs))
            samples = self.runner.verify(vb, drafts)
            now = time.perf_counter()
            self.timing["execute"] += now - t0
            self.timing["steps"] += 1
            st = self.spec_stats
            st["verify_steps"] += 1
            outs, n_new = [], 0
            for seq, d, smp in zip(batch.seqs, drafts, samples):
                a = 0
                while a < len(d) and d[a] == int(smp[a]):
                    a += 1
                st["draft_tokens"] += len(d)
                st["accepted_tokens"] += a
                new, reason = [], None
                for tok in smp[:a + 1]:
                    tok = int(tok)
                    seq.append(tok)
                    seq.num_computed += 1
                    new.append(tok)
                    reason = self._stop_reason(seq, tok)
                    if reason:
                        break
                if seq.first_token_time is None:
                    seq.first_token_time = now
                self.runner.bm.commit(seq.seq_id, seq.token_array(), seq.num_computed)
                if reason:
                    self._finish(seq, reason)
                outs.append(self._output(seq, new))
                n_new += len(new)
            self._account(vb, n_new, now - t0)
            self.timing["post"] += time.perf_counter() - now
            return outs

    def _stop_reason(self, seq: Sequence, tok: int, n_out: int | None = None) -> str | None:
        """``n_out``: output tokens up to and including ``tok`` (default: all of them)."""
        sp = seq.sampling
        n_out = len(seq.output_ids) if n_out is None else n_out
        if not sp.ignore_eos and (tok in self.eos_ids or tok in sp.stop_token_ids):
            return "stop"
        if n_out >= sp.max_tokens:
            return "length"
        if seq.num_prompt + n_out >= self.cfg.max_model_len:
            return "length"
        return None

    def _output(self, seq: Sequence, new, upto: int | None = None) -> RequestOutput:
        ids = seq.output_ids if upto is None else seq.output_ids[:upto]
        return RequestOutput(
            request_id=seq.request_id, token_ids=list(ids), finished=seq.finished,
            finish_reason=seq.finish_reason, prompt_tokens=seq.num_prompt,
            cached_prompt_tokens=seq.num_cached_prompt, arrival_time=seq.arrival_time,
            first_token_time=seq.first_token_time, first_scheduled_time=seq.first_scheduled_time,
            finish_time=seq.finish_time, new_token_ids=list(new),
            logprobs=None if seq.logprobs is None else list(seq.logprobs[:len(ids)]),
            top_logprobs=(None if seq.top_logprobs is None
                          else list(seq.top_logprobs[:len(ids)])),
            prompt_logprobs=(None if seq.prompt_logprobs is None
                             else list(seq.prompt_logprobs)),
            prompt_top_logprobs=(None if seq.prompt_top_logprobs is None
                                 else list(seq.prompt_top_logprobs)))

    # ------------------------------------------------------------------------------------
    def generate(self, prompts, sampling: SamplingParams | list) -> list[RequestOutput]:
        """Blocking batch generation (prompts: list of token-id lists or strings)."""
        if not isinstance(sampling, list):
            sampling = [sampling] * len(prompts)
        ids = []
        for i, p in enumerate(prompts):
            toks = self.tokenizer.encode(p) if isinstance(p, str) else p
            rid = f"gen-{time.monotonic_ns()}-{i}"
            self.add_request(rid, toks, sampling[i])
            ids.append(rid)
        final: dict[str, RequestOutput] = {}
        while self.has_unfinished():
            for o in self.step():
                if o.finished:
                    final[o.request_id] = o
        return [final[r] for r in ids if r in final]

    # ------------------------------------------------------------------------------------
    def kv_cache_info(self) -> dict:
        r = self.runner
        return {
            "num_gpu_blocks": r.num_blocks,
            "block_size": r.block_size,
            "total_tokens": r.kv_total_tokens,
            "free_blocks": r.bm.num_free_blocks(),
            "cached_blocks": r.bm.num_cached_blocks(),
            "prefix_queries": r.bm.prefix_queries(),
            "prefix_hits": r.bm.prefix_hits(),
        }

    def shutdown(self):
        """Release engine resources (TP engines stop their worker ranks)."""

    def est_max_concurrency(self) -> float:
        return self.runner.kv_total_tokens / max(1, self.cfg.max_model_len)


class _RepeatProposer(Proposer):
    """Warm-up drafts: the last token, k times."""

    def propose(self, seq, k: int) -> list:
        return [int(seq.token_array()[-1])] * k


def token_array(ids) -> np.ndarray:
    return np.asarray(ids, dtype=np.int64)
