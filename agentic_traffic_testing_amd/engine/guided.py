"""Guided decoding, host side: regex / choice list / JSON schema -> byte DFA -> token table.

A guide constrains what a request may generate (``SamplingParams.guided_regex`` /
``guided_choice`` / ``guided_json``).  It is compiled here, in pure Python + numpy, into a table
over the tokenizer's vocabulary that the device kernels (ops/csrc/guided.hip) index:

1. **Pattern -> byte DFA** (``compile_regex``): an own regex front end (no ``re`` internals).
   The dialect: literals, ``.``, the escapes ``\\d \\w \\s \\D \\W \\S \\n \\t \\r \\f \\v \\xHH
   \\uXXXX`` and escaped metacharacters, classes ``[...]`` with ranges and negation, groups
   ``( )`` / ``(?: )``, ``|`` and the quantifiers ``* + ? {n} {n,} {n,m}``.  Full-match
   semantics; a leading ``^`` and a trailing ``$`` are tolerated.  ``\\d \\w \\s`` are the ASCII
   sets (Python's ``re.ASCII``).  Everything else - backreferences, look-around, named groups,
   lazy or possessive quantifiers, flags, ``\\b`` - raises ``ValueError`` naming the construct.
   The automaton runs over UTF-8 bytes: a non-ASCII literal is its byte sequence, ``.`` (any
   character but a newline) and negated classes match any well-formed UTF-8 character other
   than the excluded ones; a class that lists a non-ASCII range (or negates a non-ASCII
   character) is refused.  Thompson NFA, subset construction, minimisation (partition
   refinement), then trimming: every remaining state can reach an accepting state.

2. **Choice / JSON schema -> pattern** (``choice_regex``, ``schema_regex``): a choice list is the
   alternation of the escaped strings; a JSON-Schema subset (object, string, integer, number,
   boolean, null, enum / const of scalars, array, nested objects, anyOf) becomes a regex of the
   canonical form - every property, in declaration order, at most one space after ``:`` and
   ``,`` and whitespace nowhere else.

3. **Byte DFA -> token table** (``token_table``): ``next[s][v]`` = the state after walking token
   v's bytes from state s, or -1 if the walk leaves the DFA.  Row 0 is the shared *done* state
   (only the end tokens, each back to 0); the DFA's states are rows 1 .. n, the start is row 1.
   In an accepting state every end token leads to 0; special tokens are -1 everywhere else.

``GuideCompiler`` keeps compiled guides in a thread-safe LRU keyed by (kind, canonical spec).
"""
from __future__ import annotations

import json
import threading
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np

MAX_REPEAT = 4096          # largest count in {n,m}
MAX_DFA_STATES = 32000     # subset construction gives up beyond this (int16 table entries)

_ALL = (1 << 256) - 1


def _mask(*ranges) -> int:
    m = 0
    for lo, hi in ranges:
        m |= ((1 << (hi - lo + 1)) - 1) << lo
    return m


_DIGIT = _mask((0x30, 0x39))
_WORD = _DIGIT | _mask((0x41, 0x5A), (0x61, 0x7A), (0x5F, 0x5F))
_SPACE = _mask((0x09, 0x0D), (0x20, 0x20))
_ASCII = _mask((0, 0x7F))
_CONT = _mask((0x80, 0xBF))
# well-formed UTF-8 beyond ASCII: (lead byte set, then one set per continuation byte)
_UTF8_TAILS = (
    (_mask((0xC2, 0xDF)), _CONT),
    (_mask((0xE0, 0xE0)), _mask((0xA0, 0xBF)), _CONT),
    (_mask((0xE1, 0xEC), (0xEE, 0xEF)), _CONT, _CONT),
    (_mask((0xED, 0xED)), _mask((0x80, 0x9F)), _CONT),          # no surrogates
    (_mask((0xF0, 0xF0)), _mask((0x90, 0xBF)), _CONT, _CONT),
    (_mask((0xF1, 0xF3)), _CONT, _CONT, _CONT),
    (_mask((0xF4, 0xF4)), _mask((0x80, 0x8F)), _CONT, _CONT),
)
_META = set("\\.[](){}|*+?^$")


def escape(text: str) -> str:
    """``text`` as a pattern of this dialect that matches exactly it."""
    return "".join("\\" + c if c in _META else c for c in text)


# ---- parser: pattern -> AST ------------------------------------------------------------------
# nodes: ("set", ascii_mask, any_non_ascii: bool) | ("lit", bytes) | ("cat", [nodes]) |
#        ("alt", [nodes]) | ("rep", node, lo, hi | None)
class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError(f"a pattern must be a string, got {pattern!r}")
        self.p = pattern
        self.i = 0

    def fail(self, what: str):
        raise ValueError(f"unsupported in a guided pattern: {what} (at offset {self.i} of "
                         f"{self.p!r})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        if self.peek() == "^":
            self.i += 1
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            if self.peek() == "$":
                rest = self.p[self.i + 1:]
                if rest == "":       # a trailing '$' is tolerated
                    self.i += 1
                    break
                self.fail("'$' before the end of the pattern")
            if self.peek() == "^":
                self.fail("'^' after the start of the pattern")
            items.append(self.quantified())
        return items[0] if len(items) == 1 else ("cat", items)

    def quantified(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "?":
                lo, hi = 0, 1
            elif c == "{":
                lo, hi = self.braces()
            else:
                return node
            if c != "{":
                self.i += 1
            if self.peek() == "?":
                self.fail("lazy quantifier")
            if self.peek() == "+":
                self.fail("possessive quantifier")
            node = ("rep", node, lo, hi)

    def braces(self):
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j > 0 else ""
        parts = body.split(",")
        if j < 0 or len(parts) > 2 or not parts[0].isdigit() or \
                (len(parts) == 2 and parts[1] and not parts[1].isdigit()) or not body.isascii():
            self.fail("'{' that is not {n}, {n,} or {n,m} (escape a literal brace)")
        lo = int(parts[0])
        hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if lo > MAX_REPEAT or (hi is not None and (hi > MAX_REPEAT or hi < lo)):
            self.fail(f"repeat count outside 0 .. {MAX_REPEAT} or min > max")
        self.i = j + 1
        return lo, hi

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("look-around")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    self.fail("named group")
                elif nxt[:1] == "#":
                    self.fail("comment group")
                else:
                    self.fail("inline flags or a (?...) extension")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.cls()
        if c == ".":
            self.i += 1
            return ("set", _ASCII & ~(1 << 0x0A), True)
        if c == "\\":
            kind, val = self.escape_seq(in_class=False)
            if kind == "set":
                return val
            return _char_node(val)
        if c in "*+?{":
            self.fail(f"quantifier {c!r} with nothing to repeat")
        if c in "]}":
            self.fail(f"unescaped {c!r}")
        self.i += 1
        return _char_node(ord(c))

    def escape_seq(self, in_class: bool):
        """After a backslash: ("chr", code point) or ("set", set node)."""
        self.i += 1
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        sets = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
        if c in sets:
            return "set", ("set", sets[c], False)
        if c in "DWS":
            return "set", ("set", _ASCII & ~sets[c.lower()], True)
        simple = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B}
        if c in simple:
            return "chr", simple[c]
        if c in "xu":
            n = 2 if c == "x" else 4
            h = self.p[self.i:self.i + n]
            if len(h) != n or any(d not in "0123456789abcdefABCDEF" for d in h):
                self.fail(f"\\{c} without {n} hex digits")
            self.i += n
            cp = int(h, 16)
            if 0xD800 <= cp <= 0xDFFF:
                self.fail("a surrogate code point")
            return "chr", cp
        if c.isdigit():
            self.fail("backreference or octal escape")
        if c in "bBAZ" and not (in_class and c == "b"):
            self.fail(f"the assertion \\{c}")
        if c.isalnum():
            self.fail(f"the escape \\{c}")
        return "chr", ord(c)

    def cls(self):
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        mask, non_ascii, any_high, first = 0, [], False, True
        while True:
            c = self.peek()
            if c == "":
                self.fail("unterminated '['")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i + 1:self.i + 2] == ":":
                self.fail("POSIX class")
            lo = self.cls_item()
            if isinstance(lo, tuple):           # \d, \W ... inside a class
                mask |= lo[1]
                any_high |= lo[2]
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.cls_item()
                if isinstance(hi, tuple):
                    self.fail("a range ending in a class escape")
                if hi < lo:
                    self.fail("a reversed range")
                if hi > 0x7F:
                    self.fail("a non-ASCII range in a class")
                mask |= _mask((lo, hi))
            elif lo > 0x7F:
                non_ascii.append(lo)
            else:
                mask |= 1 << lo
        if neg:
            if non_ascii or any_high:
                self.fail("a negated class that excludes non-ASCII characters")
            return ("set", _ASCII & ~mask, True)
        node = ("set", mask, any_high)
        if non_ascii:
            return ("alt", ([node] if mask or any_high else [])
                    + [_char_node(cp) for cp in dict.fromkeys(non_ascii)])
        if not mask and not any_high:
            self.fail("an empty class")
        return node

    def cls_item(self):
        c = self.peek()
        if c == "\\":
            return self.escape_seq(in_class=True)[1]   # a code point or a set node
        self.i += 1
        return ord(c)


def _char_node(cp: int):
    if cp < 0x80:
        return ("set", 1 << cp, False)
    return ("lit", chr(cp).encode("utf-8"))


# ---- AST -> NFA -> DFA ------------------------------------------------------------------------
class _NFA:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.trans: list[list[tuple[int, int]]] = []

    def new(self) -> int:
        self.eps.append([])
        self.trans.append([])
        return len(self.eps) - 1

    def build(self, node) -> tuple[int, int]:
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            if node[1]:
                self.trans[s].append((node[1], e))
            if node[2]:
                for lead, *tails in _UTF8_TAILS:
                    cur = s
                    for m in (lead, *tails[:-1]):
                        nxt = self.new()
                        self.trans[cur].append((m, nxt))
                        cur = nxt
                    self.trans[cur].append((tails[-1], e))
            return s, e
        if kind == "lit":
            s = cur = self.new()
            for b in node[1]:
                nxt = self.new()
                self.trans[cur].append((1 << b, nxt))
                cur = nxt
            return s, cur
        if kind == "cat":
            s = cur = self.new()
            for sub in node[1]:
                a, b = self.build(sub)
                self.eps[cur].append(a)
                cur = b
            return s, cur
        if kind == "alt":
            s, e = self.new(), self.new()
            for sub in node[1]:
                a, b = self.build(sub)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, lo, hi = node
        s = cur = self.new()
        for _ in range(lo):
            a, b = self.build(sub)
            self.eps[cur].append(a)
            cur = b
        if hi is None:
            a, b = self.build(sub)
            loop = self.new()
            self.eps[cur].append(loop)
            self.eps[loop].append(a)
            self.eps[b].append(loop)
            return s, loop
        e = self.new()
        for _ in range(hi - lo):
            self.eps[cur].append(e)
            a, b = self.build(sub)
            self.eps[cur].append(a)
            cur = b
        self.eps[cur].append(e)
        return s, e


@dataclass
class ByteDFA:
    """trans [n, 256] int32 (-1: no transition), accept [n] bool; state 0 is the start.  Trimmed:
    every state is reachable and reaches an accepting state."""
    trans: np.ndarray
    accept: np.ndarray

    @property
    def num_states(self) -> int:
        return self.trans.shape[0]

    def walk(self, data: bytes, state: int = 0) -> int:
        for b in data:
            if state < 0:
                return -1
            state = int(self.trans[state, b])
        return state

    def matches(self, data: bytes) -> bool:
        s = self.walk(data)
        return s >= 0 and bool(self.accept[s])


def _subset(nfa: _NFA, start: int, end: int, max_states: int):
    def closure(states):
        seen = set(states)
        stack = list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    s0 = closure([start])
    ids = {s0: 0}
    order = [s0]
    rows = []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        out = [tr for s in cur for tr in nfa.trans[s]]
        # atoms: the coarsest partition of the bytes that no transition's set splits
        atoms = [_ALL]
        for m in {m for m, _ in out}:
            nxt = []
            for a in atoms:
                if a & m:
                    nxt.append(a & m)
                if a & ~m:
                    nxt.append(a & ~m)
            atoms = nxt
        row = np.full(256, -1, dtype=np.int32)
        for a in atoms:
            tgt = [t for m, t in out if m & a]
            if not tgt:
                continue
            d = closure(tgt)
            j = ids.get(d)
            if j is None:
                j = ids[d] = len(order)
                order.append(d)
                if j >= max_states:
                    raise ValueError(f"the pattern needs more than {max_states} automaton "
                                     "states")
            bits = np.frombuffer(a.to_bytes(32, "little"), dtype=np.uint8)
            row[np.unpackbits(bits, bitorder="little").astype(bool)] = j
        rows.append(row)
    trans = np.stack(rows)
    accept = np.array([end in s for s in order], dtype=bool)
    return trans, accept


def _minimise(trans: np.ndarray, accept: np.ndarray):
    """Partition refinement over the byte classes (columns that agree everywhere are one)."""
    cols = np.unique(trans, axis=1)
    labels = accept.astype(np.int64)
    count = len(np.unique(labels))
    while True:
        ext = np.append(labels, -1)            # index -1: the dead state
        sig = np.concatenate([labels[:, None], ext[cols]], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        n = int(new.max()) + 1
        labels = new
        if n == count:
            break
        count = n
    # renumber with the start's class first, in order of first appearance
    _, first = np.unique(labels, return_index=True)
    rank = np.empty(count, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(count)
    labels = rank[labels]
    rep = np.zeros(count, dtype=np.int64)
    rep[labels[::-1]] = np.arange(len(labels))[::-1]
    t = trans[rep]
    t = np.where(t >= 0, np.append(labels, -1)[t], -1).astype(np.int32)
    return t, accept[rep]


def _trim(trans: np.ndarray, accept: np.ndarray):
    live = accept.copy()
    while True:
        ext = np.append(live, False)
        new = live | ext[trans].any(axis=1)
        if (new == live).all():
            break
        live = new
    if not live[0]:
        raise ValueError("the pattern matches no string")
    idx = np.full(len(live) + 1, -1, dtype=np.int32)
    idx[:-1][live] = np.arange(int(live.sum()), dtype=np.int32)
    return idx[trans[live]], accept[live]


def compile_regex(pattern: str, max_states: int = MAX_DFA_STATES) -> ByteDFA:
    """The minimal trimmed byte DFA that full-matches ``pattern`` (module docstring: dialect)."""
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    start, end = nfa.build(ast)
    trans, accept = _subset(nfa, start, end, max_states)
    trans, accept = _minimise(trans, accept)
    trans, accept = _trim(trans, accept)
    return ByteDFA(np.ascontiguousarray(trans), accept)


# ---- choice lists and JSON schemas -> patterns --------------------------------------------
def choice_regex(choices) -> str:
    if not isinstance(choices, (list, tuple)) or not choices or \
            not all(isinstance(c, str) and c for c in choices):
        raise ValueError(f"guided_choice must be a non-empty list of non-empty strings, got "
                         f"{choices!r}")
    return "(" + "|".join(escape(c) for c in choices) + ")"


_STR_CHAR = r'([^"\\\x00-\x1f]|\\(["\\/bfnrt]|u[0-9a-fA-F]{4}))'
_INTEGER = r"-?(0|[1-9][0-9]*)"
_NUMBER = _INTEGER + r"(\.[0-9]+)?([eE][+-]?[0-9]+)?"
_SEP = ", ?"
_SCHEMA_KEYS = {
    "object": {"properties", "required"},
    "array": {"items", "minItems", "maxItems"},
    "string": {"minLength", "maxLength"},
    "integer": set(), "number": set(), "boolean": set(), "null": set(),
}
_ANNOTATIONS = {"title", "description"}


def _count(schema: dict, key: str, default):
    v = schema.get(key, default)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_REPEAT:
        raise ValueError(f"JSON schema: {key} must be an integer in 0 .. {MAX_REPEAT}, got {v!r}")
    return v


def _repeat(lo: int, hi) -> str:
    if hi is None:
        return "*" if lo == 0 else f"{{{lo},}}"
    return f"{{{lo},{hi}}}"


def _scalar_regex(v) -> str:
    if v is not None and not isinstance(v, (str, int, float, bool)):
        raise ValueError(f"JSON schema: enum / const take scalars, got {v!r}")
    return escape(json.dumps(v, ensure_ascii=False))


def schema_regex(schema, _depth: int = 0) -> str:
    """The canonical-form regex of a JSON-Schema subset (module docstring); ``ValueError``
    naming any keyword outside it."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except json.JSONDecodeError as exc:
            raise ValueError(f"guided_json is not valid JSON: {exc}") from None
    if not isinstance(schema, dict):
        raise ValueError(f"a JSON schema must be an object, got {schema!r}")
    if _depth > 32:
        raise ValueError("JSON schema: nested deeper than 32 levels")
    for bad in ("$ref", "$defs", "definitions"):
        if bad in schema:
            raise ValueError(f"JSON schema: {bad} (references and recursion) is not supported")
    keys = set(schema) - _ANNOTATIONS
    if "enum" in schema or "const" in schema:
        extra = keys - {"enum", "const", "type"}
        if extra:
            raise ValueError(f"JSON schema: unsupported keyword {sorted(extra)[0]!r} next to "
                             "enum / const")
        vals = schema["enum"] if "enum" in schema else [schema["const"]]
        if not isinstance(vals, list) or not vals:
            raise ValueError("JSON schema: enum must be a non-empty list")
        return "(" + "|".join(_scalar_regex(v) for v in vals) + ")"
    if "anyOf" in schema:
        extra = keys - {"anyOf"}
        if extra:
            raise ValueError(f"JSON schema: unsupported keyword {sorted(extra)[0]!r} next to "
                             "anyOf")
        subs = schema["anyOf"]
        if not isinstance(subs, list) or not subs:
            raise ValueError("JSON schema: anyOf must be a non-empty list")
        return "(" + "|".join(schema_regex(s, _depth + 1) for s in subs) + ")"
    typ = schema.get("type")
    if isinstance(typ, list):
        rest = {k: v for k, v in schema.items() if k != "type"}
        return "(" + "|".join(schema_regex({"type": t, **{
            k: v for k, v in rest.items() if k in _SCHEMA_KEYS.get(t, ()) or k in _ANNOTATIONS
        }}, _depth + 1) for t in typ) + ")"
    if typ not in _SCHEMA_KEYS:
        raise ValueError(f"JSON schema: unsupported or missing type {typ!r}")
    extra = keys - {"type"} - _SCHEMA_KEYS[typ]
    if extra:
        raise ValueError(f"JSON schema: unsupported keyword {sorted(extra)[0]!r} for type "
                         f"{typ!r}")
    if typ == "string":
        lo, hi = _count(schema, "minLength", 0), _count(schema, "maxLength", None)
        if hi is not None and hi < lo:
            raise ValueError("JSON schema: maxLength < minLength")
        return '"' + _STR_CHAR + _repeat(lo, hi) + '"'
    if typ == "integer":
        return _INTEGER
    if typ == "number":
        return _NUMBER
    if typ == "boolean":
        return "(true|false)"
    if typ == "null":
        return "null"
    if typ == "array":
        lo, hi = _count(schema, "minItems", 0), _count(schema, "maxItems", None)
        if hi is not None and hi < lo:
            raise ValueError("JSON schema: maxItems < minItems")
        if "items" not in schema:
            raise ValueError("JSON schema: an array needs items")
        item = schema_regex(schema["items"], _depth + 1)
        if hi == 0:
            return r"\[\]"
        more = "(" + _SEP + item + ")" + _repeat(max(lo - 1, 0), None if hi is None else hi - 1)
        body = item + more
        return r"\[" + (body if lo > 0 else "(" + body + ")?") + r"\]"
    props = schema.get("properties", {})
    if not isinstance(props, dict):
        raise ValueError("JSON schema: properties must be an object")
    req = schema.get("required", [])
    if not isinstance(req, list) or any(r not in props for r in req):
        raise ValueError("JSON schema: required must list declared properties")
    fields = [escape(json.dumps(str(name), ensure_ascii=False)) + ": ?"
              + schema_regex(sub, _depth + 1) for name, sub in props.items()]
    return r"\{" + _SEP.join(fields) + r"\}"


# ---- byte DFA -> token table ---------------------------------------------------------------
DONE = 0     # row 0 of every table and of the device pool
START = 1    # the DFA's start state


def token_table(dfa: ByteDFA, token_bytes, vocab_size: int, eos_ids, permit_eos: bool = True):
    """int16 [n + 1, vocab_size]: row 0 the done state, row 1 + s the DFA's state s.  An entry
    is the row after the token, or -1.  ``token_bytes[v]`` is token v's bytes, None for a
    special token (ids beyond the list have none either).  ``permit_eos=False`` (a request
    with ignore_eos) leaves the end tokens out: the guide then never ends the sequence."""
    n = dfa.num_states
    if n + 1 > 32767:
        raise ValueError(f"a guide of {n} states does not fit int16 table entries")
    V = int(vocab_size)
    # walking table with a dead row n: -1 -> n, row n stays n
    t = np.where(dfa.trans >= 0, dfa.trans, n).astype(np.int16)
    t = np.concatenate([t, np.full((1, 256), n, dtype=np.int16)])
    table = np.full((n + 1, V), -1, dtype=np.int16)
    lens = np.zeros(V, dtype=np.int64)
    for v, b in enumerate(token_bytes[:V]):
        if b:
            lens[v] = len(b)
    for L in np.unique(lens):
        if L == 0:
            continue
        ids = np.nonzero(lens == L)[0]
        data = np.frombuffer(b"".join(token_bytes[v] for v in ids), dtype=np.uint8)
        data = data.reshape(len(ids), int(L))
        step = max(1, (1 << 23) // len(ids))          # states per chunk: bounded temporaries
        for s0 in range(0, n, step):
            cur = np.broadcast_to(np.arange(s0, min(n, s0 + step), dtype=np.int16)[:, None],
                                  (min(n, s0 + step) - s0, len(ids)))
            for j in range(int(L)):                   # one gather per byte position
                cur = t[cur, data[:, j]]
            table[1 + s0:1 + s0 + cur.shape[0], ids] = np.where(cur == n, -1, cur + 1)
    eos = [e for e in sorted(set(int(e) for e in eos_ids)) if 0 <= e < V]
    if eos:
        table[:, eos] = -1
        table[DONE, eos] = DONE
        if permit_eos:
            table[1:][np.ix_(dfa.accept, eos)] = DONE
    allowed = (table >= 0).any(axis=1)
    if not permit_eos:
        allowed[DONE] = True    # (no end token is ever sampled: row 0 is never entered)
    assert allowed.all(), "a guide state allows no token: the vocabulary lacks a single byte"
    return table


@dataclass
class Guide:
    kind: str               # "regex" | "choice" | "json"
    pattern: str            # the regex the spec compiled to
    dfa: ByteDFA
    next: np.ndarray        # token_table(): int16 [num_states + 1, vocab]
    key: tuple = ()

    @property
    def num_states(self) -> int:
        """Rows this guide takes in the device pool (the done row is shared)."""
        return self.next.shape[0] - 1

    def advance(self, state: int, token: int) -> int:
        """The row after ``token``, or -1 if the table does not allow it."""
        if not 0 <= token < self.next.shape[1]:
            return -1
        return int(self.next[state, token])


def guide_spec(sampling) -> tuple | None:
    """(kind, canonical spec) of a request's guide, None without one; ``ValueError`` for more
    than one of the three fields or a badly typed one."""
    fields = [(k, getattr(sampling, "guided_" + k, None)) for k in ("regex", "choice", "json")]
    given = [(k, v) for k, v in fields if v is not None]
    if not given:
        return None
    if len(given) > 1:
        raise ValueError("only one of guided_regex, guided_choice and guided_json may be set, "
                         "got " + " and ".join("guided_" + k for k, _ in given))
    kind, v = given[0]
    if kind == "regex":
        if not isinstance(v, str) or not v:
            raise ValueError(f"guided_regex must be a non-empty string, got {v!r}")
        return kind, v
    if kind == "choice":
        choice_regex(v)
        return kind, tuple(v)
    if isinstance(v, str):
        try:
            v = json.loads(v)
        except json.JSONDecodeError as exc:
            raise ValueError(f"guided_json is not valid JSON: {exc}") from None
    if not isinstance(v, dict):
        raise ValueError(f"guided_json must be a schema object or its JSON text, got {v!r}")
    try:
        return kind, json.dumps(v, ensure_ascii=False)   # key order kept: it orders properties
    except (TypeError, ValueError) as exc:
        raise ValueError(f"guided_json is not JSON-serialisable: {exc}") from None


class GuideCompiler:
    """Compiles guides for one tokenizer and keeps them in a thread-safe LRU.  ``compile`` may
    be called from any thread (the HTTP front end compiles in an executor before it submits a
    request); the lock covers the cache only, never a compile."""

    def __init__(self, token_bytes, vocab_size: int, eos_ids, max_states: int,
                 capacity: int = 16):
        self.token_bytes = token_bytes
        self.vocab_size = int(vocab_size)
        self.eos_ids = sorted(int(e) for e in eos_ids)
        self.max_states = int(max_states)    # rows a guide may take in the pool
        self.capacity = capacity
        self._lock = threading.Lock()
        self._cache: OrderedDict = OrderedDict()
        self.compiles = 0

    def compile(self, sampling) -> Guide | None:
        spec = guide_spec(sampling)
        if spec is None:
            return None
        permit_eos = not getattr(sampling, "ignore_eos", False)
        key = (*spec, permit_eos)
        with self._lock:
            g = self._cache.get(key)
            if g is not None:
                self._cache.move_to_end(key)
                return g
        kind, canon = spec
        pattern = canon if kind == "regex" else (
            choice_regex(list(canon)) if kind == "choice" else schema_regex(json.loads(canon)))
        dfa = compile_regex(pattern)
        if dfa.num_states > self.max_states:
            raise ValueError(f"the guide needs {dfa.num_states} automaton states, the pool "
                             f"(guided_pool_states) holds {self.max_states} per guide")
        if not permit_eos and (dfa.accept & (dfa.trans < 0).all(axis=1)).any():
            raise ValueError("ignore_eos with a guide whose pattern can end with nothing to "
                             "follow: only an end token could come next")
        g = Guide(kind, pattern, dfa, token_table(dfa, self.token_bytes, self.vocab_size,
                                                  self.eos_ids, permit_eos), key)
        with self._lock:
            self.compiles += 1
            g = self._cache.setdefault(key, g)
            self._cache.move_to_end(key)
            while len(self._cache) > self.capacity:
                self._cache.popitem(last=False)
        return g


__all__ = ["ByteDFA", "Guide", "GuideCompiler", "DONE", "START", "compile_regex", "choice_regex",
           "schema_regex", "token_table", "guide_spec", "escape"]
