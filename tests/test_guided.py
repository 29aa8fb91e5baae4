"""Guided decoding on the CPU backend: the regex front end against Python's ``re``, the token
table against a brute-force byte walk, the JSON-schema subset against hand-written instances,
the engine against a teacher-forced host oracle at every position (plain, top-k / top-p,
penalised, mixed batch, preemption, length cut, ignore_eos, TP refusal, pool bookkeeping) and
the infinite Gumbel draw that makes -inf the mask value.

The oracle: ``helpers.dense_logits`` on the engine's own prefix, masked to -inf by the host table
row of the prefix's automaton state, then ``ops.reference`` sampling with the request's seed and
the position as step.  The engine's token must be the oracle's, or within test_penalties.py's
near-tie tolerance of its score (0.05 logit on the CPU, no position may need it there)."""
import json
import random
import re

import numpy as np
import pytest
import torch

from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine import guided as gd
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.engine.tokenizer import SyntheticTokenizer
from agentic_traffic_testing_amd.ops import reference as ref
from helpers import dense_logits
from test_penalties import penalised_logits

# ---- the regex front end against re ----------------------------------------------------------
PATTERNS = [
    r"abc", r"a|bc|", r"(ab)*c+", r"[0-9]{3}-[0-9]{4}", r"\d+\.\d*", r"\w+@\w+\.(com|org)",
    r'"[^"]*"', r".+", r"a.c", r"x{2,}", r"y{0,3}z", r"(?:ab|cd){2}", r"\s*\S+\s*", r"[a-c-]+",
    r"[\]\\^]+", r"é+ü", r"\xe9\u00fc?\x41", r"^ab?c$", r"[^a-z\n]{1,3}", r"\D\W", r"(a|b)*abb",
    r"\{\"k\": ?\d\}", r"[\d\s]+x", r"\t\n\r", r"-?(0|[1-9][0-9]*)(\.[0-9]+)?", r"[é]a|b",
    r"\.\*\+\?\(\)\[\]\|\$\^", r"([a-z]+ )+", r"(a?){3}b", r"[^\"\\\x00-\x1f]*",
]
REJECTED = [
    (r"(a)\1", "backreference"), (r"(?=a)b", "look-around"), (r"(?!a)b", "look-around"),
    (r"(?<=a)b", "look-around"), (r"(?<!a)b", "look-around"), (r"a*?", "lazy"),
    (r"a+?", "lazy"), (r"a{2}?", "lazy"), (r"a++", "possessive"), (r"(?i)a", "flags"),
    (r"\bfoo", "assertion"), (r"(?P<n>a)", "named group"), (r"[a-é]", "non-ASCII range"),
    (r"a{2", "'{'"), (r"a$b", r"'\$'"), (r"a^b", r"'\^'"), (r"[^é]", "negated class"),
    (r"(a", "unbalanced"), (r"a)", "unbalanced"), (r"*a", "nothing to repeat"),
    (r"[abc", "unterminated"), ("a\\", "backslash"), (r"a{3,2}", "repeat"), (r"\pL", "escape"),
]
NOISE = b"ab01 -.\"\n\\x{}z\xc3\xa9\xff"


def strings_of(dfa, rng, n=120):
    """Random walks of the DFA to accepting states, the same strings with one byte mutated or
    the tail cut, and random strings."""
    dist = np.where(dfa.accept, 0, 1 << 30)      # bytes to the nearest accepting state
    for _ in range(dfa.num_states):
        dist = np.minimum(dist, 1 + np.append(dist, 1 << 30)[dfa.trans].min(axis=1))
    out = []
    for k in range(n):
        s, buf = 0, bytearray()
        for _ in range(rng.randint(0, 14)):
            nz = np.nonzero(dfa.trans[s] >= 0)[0]
            if len(nz) == 0:
                break
            b = int(rng.choice(nz.tolist()))
            buf.append(b)
            s = int(dfa.trans[s, b])
        while not dfa.accept[s]:     # trimmed: every state has a shortest way to accept
            nxt = dfa.trans[s]
            nz = np.nonzero((nxt >= 0) & (np.append(dist, 1 << 30)[nxt] < dist[s]))[0]
            b = int(rng.choice(nz.tolist()))
            buf.append(b)
            s = int(dfa.trans[s, b])
        out.append(bytes(buf))
        if buf:
            m = bytearray(buf)
            m[rng.randrange(len(m))] = rng.randrange(256)
            out.append(bytes(m))
            out.append(bytes(buf[:rng.randrange(len(buf))]))
        out.append(bytes(rng.choice(NOISE) for _ in range(rng.randint(0, 6))))
    return out


def re_fullmatch(pattern: str, data: bytes) -> bool:
    """Python's verdict: \\d \\w \\s are the ASCII sets (re.ASCII), the text is UTF-8 - bytes that
    are not well-formed UTF-8 match nothing."""
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return re.fullmatch(pattern, text, re.ASCII) is not None


@pytest.mark.parametrize("pattern", PATTERNS)
def test_dfa_agrees_with_re(pattern):
    dfa = gd.compile_regex(pattern)
    rng = random.Random(len(pattern))
    strings = strings_of(dfa, rng)
    accepted = 0
    for s in strings:
        want = re_fullmatch(pattern, s)
        assert dfa.matches(s) == want, (pattern, s, want)
        accepted += want
    assert accepted >= 120 and accepted < len(strings)     # both verdicts were exercised
    # trimmed and minimal enough: every state reaches an accepting one
    live = dfa.accept.copy()
    for _ in range(dfa.num_states):
        live |= np.append(live, False)[dfa.trans].any(axis=1)
    assert live.all()


@pytest.mark.parametrize("pattern,what", REJECTED)
def test_rejected_constructs_raise(pattern, what):
    with pytest.raises(ValueError, match=what):
        gd.compile_regex(pattern)


def test_choice_is_the_alternation_of_the_escaped_strings():
    choices = ["yes", "no (maybe)", "a|b", "1.5*", "né"]
    dfa = gd.compile_regex(gd.choice_regex(choices))
    for c in choices:
        assert dfa.matches(c.encode())
    for bad in ("", "ye", "yess", "a", "b", "no maybe", "1x5*", "1.55"):
        assert not dfa.matches(bad.encode())
    for bad in ([], ["a", 3], "ab", [""]):
        with pytest.raises(ValueError):
            gd.choice_regex(bad)


# ---- the token table ---------------------------------------------------------------------------
DIGITS = r"[0-9]{3}-[0-9]{4}"


def brute(dfa, piece, s):
    """Row after walking ``piece`` from table row ``s`` (1 + DFA state), or -1."""
    st = dfa.walk(piece, s - 1)
    return st + 1 if st >= 0 else -1


def check_table_invariants(table, dfa, tok, eos):
    V = tok.vocab_size
    special = np.arange(tok.num_ordinary, V)
    not_eos = np.setdiff1d(special, eos)
    assert (table[:, not_eos] == -1).all()                       # special tokens: nowhere
    assert (table[0, eos] == 0).all() and (np.delete(table[0], eos) == -1).all()   # done row
    acc = np.concatenate([[False], dfa.accept])
    assert (table[acc][:, eos] == 0).all()                       # EOS -> done where accepting
    assert (table[1:][~dfa.accept][:, eos] == -1).all()          # ... and nowhere else
    assert (table[:, :tok.num_ordinary] != 0).all()              # only end tokens reach done
    assert (table >= 0).any(axis=1).all()                        # every state allows a token
    assert table.dtype == np.int16 and table.shape == (dfa.num_states + 1, V)


@pytest.mark.parametrize("pattern", [DIGITS, r"(yes|no|maybe so)", r'\{"a": ?"[^"\\]{0,4}é?"\}'])
def test_token_table_small_vocabulary_equals_the_byte_walk(pattern):
    tok = SyntheticTokenizer(vocab_size=3000)
    assert tok.vocab_size % 8 == 0
    pieces = tok.token_bytes()
    assert len(pieces) == 3000 and pieces[:256] == [bytes([i]) for i in range(256)]
    assert all(p is None for p in pieces[tok.num_ordinary:])
    assert all(tok.decode([i]) == p.decode("utf-8", "replace") for i, p in
               enumerate(pieces[256:tok.num_ordinary], 256))
    dfa = gd.compile_regex(pattern)
    eos = [tok.eos_token_id, tok.num_ordinary + 1]
    table = gd.token_table(dfa, pieces, tok.vocab_size, eos)
    for s in range(1, dfa.num_states + 1):
        for v in range(tok.num_ordinary):
            assert table[s, v] == brute(dfa, pieces[v], s), (s, v, pieces[v])
    check_table_invariants(table, dfa, tok, np.array(sorted(eos)))
    # without end tokens (ignore_eos): the same table but for the EOS columns
    open_table = gd.token_table(gd.compile_regex(r"([a-z]+ )+"), pieces, tok.vocab_size, eos,
                                permit_eos=False)
    assert (open_table[1:, eos] == -1).all() and (open_table[1:] >= 0).any(axis=1).all()


def test_token_table_llama_vocabulary_sampled_pairs():
    tok = SyntheticTokenizer(vocab_size=128256)
    pieces = tok.token_bytes()
    dfa = gd.compile_regex(DIGITS)
    eos = np.array([tok.num_ordinary + 1, tok.eos_token_id])
    table = gd.token_table(dfa, pieces, tok.vocab_size, eos)
    rng = np.random.default_rng(0)
    for s, v in zip(rng.integers(1, dfa.num_states + 1, 20000).tolist(),
                    rng.integers(0, tok.num_ordinary, 20000).tolist()):
        assert table[s, v] == brute(dfa, pieces[v], s), (s, v, pieces[v])
    check_table_invariants(table, dfa, tok, eos)
    allowed = int((table[1] >= 0).sum())
    assert 1000 <= allowed <= 1300, allowed     # "7", "42", "581": under 1 % of the vocabulary


# ---- JSON schemas --------------------------------------------------------------------------
SCHEMA = {
    "type": "object",
    "properties": {
        "name": {"type": "string", "minLength": 1, "maxLength": 8},
        "age": {"type": "integer"},
        "score": {"type": "number"},
        "ok": {"type": "boolean"},
        "tag": {"enum": ["a", "b c", 3, None, True]},
        "kind": {"const": "x"},
        "list": {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3},
        "opt": {"anyOf": [{"type": "null"}, {"type": "string"}]},
        "in": {"type": "object", "properties": {"z": {"type": ["integer", "null"]}}},
    },
    "required": ["name"],
}
VALID = ('{"name": "Zoë", "age": -12, "score": 1.5e-3, "ok": true, "tag": "b c", "kind": "x", '
         '"list": [1, 2, 3], "opt": null, "in": {"z": 0}}')


def test_schema_accepts_canonical_instances():
    dfa = gd.compile_regex(gd.schema_regex(SCHEMA))
    compact = VALID.replace(": ", ":").replace(", ", ",")
    for text in (VALID, compact, VALID.replace('"tag": "b c"', '"tag": null'),
                 VALID.replace('"tag": "b c"', '"tag": 3').replace("[1, 2, 3]", "[7]"),
                 VALID.replace('"Zoë"', r'"a\"\\\n\u00e9"').replace("null, ", '"s", '),
                 VALID.replace("1.5e-3", "0").replace('"z": 0', '"z": null')):
        json.loads(text)
        assert dfa.matches(text.encode()), text
    assert gd.compile_regex(gd.schema_regex(json.dumps(SCHEMA))).num_states == dfa.num_states


@pytest.mark.parametrize("old,new", [
    ('"age": -12', '"age": "12"'), ('"age": -12', '"age": 1.5'), ('"age": -12', '"age": 012'),
    ('"ok": true', '"ok": 1'), ('"tag": "b c"', '"tag": "d"'), ('"kind": "x"', '"kind": "y"'),
    ("[1, 2, 3]", "[]"), ("[1, 2, 3]", "[1, 2, 3, 4]"), ('"Zoë"', '""'), ('"Zoë"', '"123456789"'),
    ('"Zoë"', '"a\nb"'), ('"Zoë"', r'"a\qb"'), ('"opt": null', '"opt": 1'),
    ('"age": -12, ', ""),                                             # a missing property
    ('"age": -12, "score": 1.5e-3', '"score": 1.5e-3, "age": -12'),   # reordered
    ('"name": ', '"name":  '), ('{"name"', '{ "name"'), ("[1, 2, 3]", "[1 , 2, 3]"),
    ('{"z": 0}}', '{"z": 0} }'), ('{"z": 0}}', '{"z": 0}}\n'), ('"ok": true', '"ok":\ttrue'),
])
def test_schema_rejects(old, new):
    dfa = gd.compile_regex(gd.schema_regex(SCHEMA))
    assert old in VALID
    assert not dfa.matches(VALID.replace(old, new).encode())


@pytest.mark.parametrize("schema,what", [
    ({"$ref": "#/x"}, r"\$ref"), ({"type": "object", "additionalProperties": False},
                                  "additionalProperties"),
    ({"type": "string", "pattern": "a+"}, "pattern"), ({"type": "integer", "minimum": 0}, "minimum"),
    ({"type": "array"}, "items"), ({"type": "tuple"}, "type"), ({}, "type"),
    ({"enum": [[1]]}, "scalars"), ({"type": "string", "format": "date"}, "format"),
    ({"type": "object", "properties": {"a": {"$ref": "#"}}}, r"\$ref"),
    ({"oneOf": [{"type": "null"}]}, "type"), ("{not json", "valid JSON"),
    ({"type": "string", "maxLength": -1}, "maxLength"),
])
def test_schema_unsupported_raises(schema, what):
    with pytest.raises(ValueError, match=what):
        gd.schema_regex(schema)


# ---- the engine against the oracle -----------------------------------------------------------
CHOICES = ["yes", "no", "maybe so", "ask again later"]
BOUNDED = {"type": "object", "properties": {
    "verdict": {"enum": ["pass", "fail", "retry"]},
    "final": {"type": "boolean"},
    "note": {"type": "string", "maxLength": 6},
    "steps": {"type": "array", "items": {"enum": [1, 2, 3]}, "maxItems": 3}}}
GUIDES = {"choice": dict(guided_choice=CHOICES), "regex": dict(guided_regex=DIGITS),
          "json": dict(guided_json=BOUNDED)}
MODES = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=0.8, seed=5),
         "topkp": dict(temperature=0.8, seed=6, top_k=40, top_p=0.9)}
# the longest match of any guide below is BOUNDED's: 70 bytes of canonical JSON with six
# \uXXXX escapes in the note, 100 bytes - at worst one token a byte, then the end token
LONGEST = 101
MAX_TOKENS = 200
SHAPES = ((0, 12), (1, 40), (2, 23))   # (seed, prompt length)


def engine(**kw):
    base = dict(model="small", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def prompts(hi=30000):
    return [np.random.default_rng(seed).integers(10, hi, n).tolist() for seed, n in SHAPES]


def validate_bounded(text):
    obj = json.loads(text)
    assert list(obj) == ["verdict", "final", "note", "steps"]
    assert obj["verdict"] in ("pass", "fail", "retry") and isinstance(obj["final"], bool)
    assert isinstance(obj["note"], str) and len(obj["note"]) <= 6
    assert isinstance(obj["steps"], list) and len(obj["steps"]) <= 3
    assert all(s in (1, 2, 3) and not isinstance(s, bool) for s in obj["steps"])


def check_text(kind, text):
    if kind == "choice":
        assert text in CHOICES
    elif kind == "regex":
        assert re.fullmatch(DIGITS, text)
    else:
        validate_bounded(text)


def check_guided(eng, prompt, out, sp, tol=0.05, max_bad=0, ended=True):
    """Every position teacher-forced through the host oracle.  Returns the number of positions
    whose UNMASKED argmax is a token the guide does not allow there."""
    guide = eng.compile_guide(sp)
    ids = list(out.token_ids)
    state, outs, bad, steered = gd.START, [], 0, 0
    for step, t in enumerate(ids):
        raw = dense_logits(eng.runner.model, list(prompt) + outs).float().cpu()
        if sp.penalised:    # penalties first, then the mask (test_penalties.py's formula)
            raw = penalised_logits(raw, prompt, outs, sp).float()
        row = torch.from_numpy(guide.next[state].astype(np.int64))
        masked = torch.where(row < 0, torch.tensor(float("-inf")), raw)[None]
        steered += int(row[int(torch.argmax(raw))]) < 0
        temp = torch.tensor([sp.temperature])
        seeds, steps = torch.tensor([sp.seed or 0]), torch.tensor([step])
        if sp.top_p < 1.0 or sp.top_k > 0:
            want = int(ref.sample_topkp(masked, temp, torch.tensor([sp.top_p]),
                                        torch.tensor([sp.top_k], dtype=torch.int32), seeds,
                                        steps)[0])
        else:
            want = int(ref.sample(masked, temp, seeds, steps)[0])
        assert int(row[t]) >= 0, (step, t, "a token the guide does not allow")
        if want != t:   # test_penalties.py's near-tie rule, on the scores the sampler compares
            sc = ref._nan_loses(ref._sample_scores(masked, 0, temp, seeds, steps, 0))
            scale = sp.temperature if sp.temperature > 1e-5 else 1.0
            gap = float(sc[want] - sc[t]) * scale
            assert 0 <= gap < tol, (step, t, want, gap)
            bad += 1
        state = int(row[t])
        outs.append(t)
    assert bad <= max_bad, (bad, len(ids))
    if ended:
        assert out.finish_reason == "stop" and ids[-1] in eng.eos_ids and state == gd.DONE
        assert len(ids) <= LONGEST < MAX_TOKENS     # it ends on EOS, well inside max_tokens
    return steered


@pytest.fixture(scope="module")
def eng():
    return engine()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", list(GUIDES))
def test_engine_matches_oracle_at_every_position(eng, kind, mode):
    ps = prompts()
    sp = SamplingParams(max_tokens=MAX_TOKENS, **MODES[mode], **GUIDES[kind])
    outs = eng.generate(ps, sp)
    for p, o in zip(ps, outs):
        text = eng.tokenizer.decode(o.token_ids)
        check_text(kind, text)
        steered = check_guided(eng, p, o, sp)
        print(f"{kind}/{mode} prompt {len(p)}: {text!r}, {len(o.token_ids)} tokens, unmasked "
              f"argmax disallowed at {steered}")
        # an unconstrained model would not have produced this: the guide decided most positions
        assert 2 * steered >= len(o.token_ids)
    r = eng.runner
    assert not r._guide_slots and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
    assert all(e["refs"] == 0 for e in r._guide_pool.values()) and not r._guide_of


def test_guided_and_penalised(eng):
    p = prompts()[0]
    pattern = r"[0-9]{12}"
    plain = SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS, guided_regex=pattern)
    b = eng.generate([p], plain)[0]
    letter = eng.tokenizer.encode("the")[0]
    # the plain run's first token is banned, a token outside the pattern gets +100, and what was
    # generated is penalised: the bias moves the choice among the allowed tokens only
    sp = SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS, guided_regex=pattern,
                        frequency_penalty=2.0, presence_penalty=2.0, repetition_penalty=1.5,
                        logit_bias={b.token_ids[0]: -100.0, letter: 100.0})
    a = eng.generate([p], sp)[0]
    ta, tb = eng.tokenizer.decode(a.token_ids), eng.tokenizer.decode(b.token_ids)
    assert re.fullmatch(pattern, ta) and re.fullmatch(pattern, tb)
    assert a.finish_reason == b.finish_reason == "stop"
    assert a.token_ids[0] != b.token_ids[0] and letter not in a.token_ids
    assert check_guided(eng, p, a, sp) == len(a.token_ids)    # +100 on a disallowed token
    assert check_guided(eng, p, b, plain) >= len(b.token_ids) // 2
    assert not eng.runner._pen_slot and not eng.runner._guide_slots


def test_mixed_batch_leaves_the_unguided_request_alone(eng):
    ps = prompts()
    free = SamplingParams(temperature=0.8, max_tokens=15, ignore_eos=True, seed=11)
    alone = engine().generate([ps[1]], free)[0].token_ids
    assert engine().runner.guide is None
    sp = SamplingParams(temperature=0.8, seed=5, max_tokens=MAX_TOKENS, guided_choice=CHOICES)
    outs = eng.generate([ps[1], ps[0]], [free, sp])
    assert outs[0].token_ids == alone               # bit-equal to the run without a guide
    assert eng.tokenizer.decode(outs[1].token_ids) in CHOICES
    check_guided(eng, ps[0], outs[1], sp)


def test_preemption_continues_mid_pattern(eng):
    ps = prompts()
    pattern = r"([0-9]-){20}"        # no piece spans a digit and a dash: 40 tokens and the end
    sp = SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS, guided_regex=pattern)
    want = [o.token_ids for o in eng.generate(ps, sp)]
    assert [len(w) for w in want] == [41] * 3
    # 8 blocks of 16 tokens cannot hold the 12 + 40 + 23 + 3 * 41 tokens the three end with
    small = engine(max_model_len=96, num_kv_blocks=8, enable_prefix_caching=False)
    outs = small.generate(ps, sp)
    assert small.scheduler.num_preemptions > 0
    assert [o.token_ids for o in outs] == want
    for o in outs:
        assert re.fullmatch(pattern, small.tokenizer.decode(o.token_ids))
    assert not small.runner._guide_slots and not small.runner._guide_of


def test_max_tokens_cut_gives_a_valid_prefix(eng):
    p = prompts()[2]
    sp = SamplingParams(temperature=0.0, max_tokens=4, guided_regex=r"[0-9]{40}")
    o = eng.generate([p], sp)[0]
    assert o.finish_reason == "length" and len(o.token_ids) == 4
    text = eng.tokenizer.decode(o.token_ids)
    assert re.fullmatch(r"[0-9]{4,12}", text)
    assert eng.compile_guide(sp).dfa.walk(text.encode()) >= 0        # a live state: a prefix
    check_guided(eng, p, o, sp, ended=False)


def test_ignore_eos_rules(eng):
    p = prompts()[0]
    # a pattern that can go on: the guide never allows an end token, the run is cut by length
    sp = SamplingParams(temperature=0.8, seed=2, max_tokens=20, ignore_eos=True,
                        guided_regex=r"([a-z]+ )+")
    o = eng.generate([p], sp)[0]
    assert o.finish_reason == "length" and len(o.token_ids) == 20
    assert not set(o.token_ids) & eng.eos_ids
    assert re.fullmatch(r"([a-z]+ )*[a-z]* ?", eng.tokenizer.decode(o.token_ids))
    check_guided(eng, p, o, sp, ended=False)
    # a pattern that can only end: nothing but EOS could follow its last state
    for kw in (dict(guided_regex=DIGITS), dict(guided_choice=CHOICES), dict(guided_json=BOUNDED)):
        with pytest.raises(ValueError, match="ignore_eos"):
            eng.add_request("r", p, SamplingParams(ignore_eos=True, **kw))
    assert not eng.has_unfinished()


@pytest.mark.parametrize("bad", [
    dict(guided_regex=""), dict(guided_regex=5), dict(guided_regex=r"a(?=b)"),
    dict(guided_choice=[]), dict(guided_choice="yes"), dict(guided_choice=["a", 1]),
    dict(guided_json=[1]), dict(guided_json="{"), dict(guided_json={"type": "string", "x": 1}),
    dict(guided_regex="a", guided_choice=["a"]), dict(guided_regex="a", guided_json={}),
    dict(guided_choice=["a"], guided_json={"type": "null"}),
    dict(guided_regex=r"[0-9]{5000}"),
])
def test_bad_guides_raise_and_leave_the_engine_idle(bad):
    e = engine(model="tiny")
    with pytest.raises(ValueError):
        e.add_request("r", [1, 2, 3], SamplingParams(**bad))
    assert not e.has_unfinished()
    assert e.runner.guide is None       # nothing allocated for a refused request


def test_tp2_gloo_refuses_guided_requests():
    from agentic_traffic_testing_amd.parallel.tp_engine import TPEngine

    base = dict(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    e = TPEngine(EngineConfig(tensor_parallel_size=2, **base))
    try:
        for kw in GUIDES.values():
            with pytest.raises(ValueError, match="tensor-parallel"):
                e.add_request("r", [1, 2, 3], SamplingParams(**kw))
        assert not e.has_unfinished()
    finally:
        e.shutdown()


def test_pool_full_and_eviction_of_an_unused_guide():
    e = engine(model="tiny", guided_pool_states=24)          # 23 rows for guides
    r = e.runner
    with pytest.raises(ValueError, match="pool"):            # 31 states: larger than the pool
        e.add_request("big", [1, 2], SamplingParams(guided_regex=r"[0-9]{30}"))
    assert r.guide is None
    a = SamplingParams(temperature=0.0, max_tokens=30, guided_regex=r"a{9}")     # 10 states
    b = SamplingParams(temperature=0.0, max_tokens=30, guided_regex=r"b{9}")
    c = SamplingParams(temperature=0.0, max_tokens=30, guided_regex=r"c{9}")
    e.add_request("a", [1, 2], a)
    e.add_request("b", [1, 2], b)
    assert sorted(x["base"] for x in r._guide_pool.values()) == [1, 11]
    with pytest.raises(ValueError, match="no room"):         # both are held by a request
        e.add_request("c", [1, 2], c)
    done = {}
    while e.has_unfinished():
        for o in e.step():
            if o.finished:
                done[o.request_id] = e.tokenizer.decode(o.token_ids)
    assert done == {"a": "a" * 9, "b": "b" * 9}
    assert [x["refs"] for x in r._guide_pool.values()] == [0, 0]
    again = e.generate([[1, 2]], b)[0]                       # b is used again: a is the LRU
    assert e.tokenizer.decode(again.token_ids) == "b" * 9
    out = e.generate([[1, 2]], c)[0]                         # c evicts a and takes its rows
    assert e.tokenizer.decode(out.token_ids) == "c" * 9
    assert {k[1]: x["base"] for k, x in r._guide_pool.items()} == {"b{9}": 11, "c{9}": 1}
    assert e._guides.compiles == 3
    assert e.tokenizer.decode(e.generate([[1, 2]], a)[0].token_ids) == "a" * 9   # and back


def test_unguided_requests_keep_variant_code_and_layout():
    from agentic_traffic_testing_amd.engine import model_runner as mr

    assert mr.V_GUIDE == 16
    for topkp in (False, True):
        for lp in (mr.LP_NONE, mr.LP_SAMPLED, mr.LP_TOPN):
            for pen in (False, True):
                old = mr.variant_code(topkp, lp, pen)
                assert old == int(topkp) | lp << 1 | 8 * pen and mr.variant_lp(old) == lp
                new = mr.variant_code(topkp, lp, pen, guide=True)
                assert new == old | 16 and mr.variant_lp(new) == lp
    for pen in (False, True):
        plain = mr.MetaLayout(7, 3, 4, 2, penalty=pen)
        guided = mr.MetaLayout(7, 3, 4, 2, penalty=pen, guide=True)
        for name, field in plain.fields.items():         # existing offsets do not move
            assert guided.fields[name] == field
        assert list(guided.fields)[len(plain.fields):] == ["guide_slot"]
        assert guided.size > plain.size and "guide_slot" not in plain.fields
    e = engine(model="tiny")
    sp = SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True)
    assert not sp.guided and e.compile_guide(sp) is None
    e.generate([[5, 6, 7]], sp)
    assert e.runner.guide is None and e._guides is None and e.runner._f32_logits is None


def test_compile_cache_is_shared_and_thread_safe():
    import threading

    e = engine(model="tiny")
    sps = [SamplingParams(guided_json=BOUNDED), SamplingParams(guided_json=json.dumps(BOUNDED)),
           SamplingParams(guided_choice=CHOICES), SamplingParams(guided_regex=DIGITS)]
    got = []
    threads = [threading.Thread(target=lambda sp=sp: got.append(e.compile_guide(sp)))
               for sp in sps * 3]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(got) == 12 and len({id(g) for g in got}) == 3    # dict and text: one guide
    assert e.compile_guide(sps[0]) is e.compile_guide(sps[1])
    assert e.compile_guide(SamplingParams(guided_regex=r"([a-z]+ )+", ignore_eos=True)) is not \
        e.compile_guide(SamplingParams(guided_regex=r"([a-z]+ )+"))


# ---- the infinite Gumbel draw ------------------------------------------------------------------
INF_SEED, INF_STEP, INF_ID = 0, 218, 2043     # found by a vectorised search over ref.gumbel_noise


def test_the_infinite_draw_never_beats_a_masked_token():
    g = ref.gumbel_noise(INF_SEED, INF_STEP, torch.tensor([INF_ID]))
    assert torch.isinf(g).all() and float(g) > 0         # u rounds to 1: -log(-log(1)) = +inf
    V, other = max(INF_ID + 8, 64), INF_ID + 3
    logits = torch.full((1, V), float("-inf"))
    logits[0, other] = -5.0                              # the one allowed token
    temp, seeds, steps = torch.tensor([0.8]), torch.tensor([INF_SEED]), torch.tensor([INF_STEP])
    sc = ref._sample_scores(logits, 0, temp, seeds, steps, 0)
    assert torch.isnan(sc[INF_ID])                       # -inf + inf: what a finite mask would win
    finite = torch.where(torch.isinf(logits), torch.tensor(-1e30), logits)
    assert int(torch.argmax(ref._sample_scores(finite, 0, temp, seeds, steps, 0))) == INF_ID
    assert int(ref.sample(logits, temp, seeds, steps)[0]) == other
    top_p, top_k = torch.tensor([0.9]), torch.tensor([5], dtype=torch.int32)
    assert int(ref.sample_topkp(logits, temp, top_p, top_k, seeds, steps)[0]) == other


def test_hf_tokenizer_token_bytes_inverts_the_byte_level_map(tmp_path):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers

    from agentic_traffic_testing_amd.engine.tokenizer import HFTokenizer, _bytes_to_unicode

    b2u = _bytes_to_unicode()
    assert len(set(b2u.values())) == 256 and b2u[ord("A")] == "A" and b2u[ord(" ")] == "Ġ"
    vocab = {b2u[b]: b for b in range(256)}
    merges = []
    for word in (" the", "é", "12", "\n\n"):          # a few multi-byte pieces
        cs = [b2u[b] for b in word.encode()]
        while len(cs) > 1:
            merges.append((cs[0], cs[1]))
            cs[:2] = [cs[0] + cs[1]]
            vocab.setdefault(cs[0], len(vocab))
    tok = Tokenizer(models.BPE(vocab=vocab, merges=merges))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    tok.decoder = decoders.ByteLevel()
    tok.add_special_tokens(["<|begin_of_text|>", "<|eot_id|>"])
    tok.save(str(tmp_path / "tokenizer.json"))
    hf = HFTokenizer(str(tmp_path))
    pieces = hf.token_bytes()
    assert len(pieces) == hf.vocab_size == len(vocab) + 2
    assert pieces[hf.eos_token_id] is None and pieces[hf.bos_token_id] is None
    assert sorted(p for p in pieces[:256]) == [bytes([b]) for b in range(256)]
    for word in (" the", "é", "12", "\n\n"):
        ids = hf.encode(word)
        assert len(ids) == 1 and pieces[ids[0]] == word.encode()
    text = "the é 12 the\n\n"
    assert b"".join(pieces[i] for i in hf.encode(text)) == text.encode()
    # and a guide compiles over it
    table = gd.token_table(gd.compile_regex(r"( the|é|12)+"), pieces, hf.vocab_size,
                           [hf.eos_token_id])
    assert table[gd.START, hf.encode(" the")[0]] > 0 and table[gd.START, hf.encode("\n\n")[0]] < 0
