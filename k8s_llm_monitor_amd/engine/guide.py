"""Guides for constrained decoding: a choice list, a regular expression or a JSON schema compiled
to one minimal DFA over **bytes**.

The sampler (``ops.GuideState``) keeps the DFA and one token bitmask per state on the device; a
guided row reads its logits through the mask of its current state and the sampler's final kernel
walks the drawn token's bytes, so a captured decode step advances the guide by itself.  This
module is the host side only: pure Python + numpy, run on the caller's thread.

``compile_guide(spec)`` takes plain data (it travels to data-parallel replicas pickled):

* ``{"choice": [str, ...]}``   - exactly one of the strings;
* ``{"regex": str}``           - a whole-string match (``re.fullmatch``) of the subset below;
* ``{"json_schema": dict}``    - *compact* JSON (separators ``,`` and ``:``, no whitespace) of the
  schema subset below.

Regex subset: literals, ``\\d \\w \\s \\D \\W \\S`` (the ASCII classes, as under ``re.ASCII``),
``\\n \\t \\r \\f \\v``, ``\\xHH``, ``\\uHHHH``, escaped metacharacters, classes with ranges and
negation, ``.`` (anything but ``\\n``), ``|``, groups ``( )`` / ``(?: )`` and the greedy quantifiers
``? * + {m} {m,} {m,n}``.  A leading ``^`` and a trailing ``$`` are accepted and ignored.  Non-ASCII
literals and class members are their UTF-8 byte sequences; ``.``, negated classes and ``\\D \\W \\S``
match one well-formed UTF-8 scalar outside the excluded set, never a lone continuation byte.
Everything else (back-references, look-around, lazy / possessive quantifiers, inline flags, named
groups, inner anchors) raises ``ValueError``.

Schema subset: ``object`` (every property, in the listed order; ``required`` and
``additionalProperties`` are ignored), ``string`` (``minLength`` / ``maxLength``), ``integer``,
``number``, ``boolean``, ``null``, ``enum`` / ``const`` of scalars, ``array`` (``items``,
``minItems`` / ``maxItems``), nested without recursion.  Any other keyword raises ``ValueError``.
"""
from __future__ import annotations

import json
import re
import threading
from collections import OrderedDict
from typing import Optional

import numpy as np

DEFAULT_MAX_STATES = 512
_BLOWUP = 4  # subset construction gives up past this multiple of the state limit
_CACHE_SIZE = 64
_MAX_CP = 0x10FFFF

# ---------------------------------------------------------------------------------------------
# AST: ("set", ranges) one scalar out of sorted code-point ranges | ("cat", [..]) | ("alt", [..])
#      | ("rep", node, lo, hi or None)


def _norm(ranges) -> list:
    """Sorted, merged code-point ranges without the surrogates (not encodable as UTF-8)."""
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    res = []
    for lo, hi in out:
        if lo < 0xD800:
            res.append((lo, min(hi, 0xD7FF)))
        if hi > 0xDFFF:
            res.append((max(lo, 0xE000), hi))
    return res


def _negate(ranges) -> list:
    out, nxt = [], 0
    for lo, hi in _norm(ranges):
        if lo > nxt:
            out.append((nxt, lo - 1))
        nxt = hi + 1
    if nxt <= _MAX_CP:
        out.append((nxt, _MAX_CP))
    return _norm(out)


_DIGIT = [(0x30, 0x39)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_SPACE = [(0x09, 0x0D), (0x20, 0x20)]
_CLASSES = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _negate(_DIGIT), "W": _negate(_WORD), "S": _negate(_SPACE)}
_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11}


def _lit(text: str):
    return ("cat", [("set", [(ord(c), ord(c))]) for c in text])


def _set(ranges):
    return ("set", _norm(ranges))


class _Parser:
    def __init__(self, pat: str):
        if not isinstance(pat, str):
            raise ValueError("regex must be a string")
        self.p, self.i = pat, 0
        self.end = len(pat)
        if pat.startswith("^"):
            self.i = 1
        if pat.endswith("$") and not self._escaped_at(len(pat) - 1) and len(pat) > self.i:
            self.end -= 1

    def _escaped_at(self, k: int) -> bool:
        n = 0
        while k - 1 - n >= 0 and self.p[k - 1 - n] == "\\":
            n += 1
        return n % 2 == 1

    def err(self, what: str):
        return ValueError(f"regex: {what} at position {self.i} is not supported")

    def parse(self):
        node = self.alt()
        if self.i < self.end:
            raise self.err(f"unbalanced {self.p[self.i]!r}")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.i < self.end and self.p[self.i] == "|":
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.i < self.end and self.p[self.i] not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        atom = self.atom()
        while self.i < self.end:
            c = self.p[self.i]
            if c == "?":
                lo, hi, n = 0, 1, 1
            elif c == "*":
                lo, hi, n = 0, None, 1
            elif c == "+":
                lo, hi, n = 1, None, 1
            elif c == "{":
                m = re.compile(r"\{(\d+)(,(\d*))?\}").match(self.p, self.i, self.end)
                if m is None:
                    break  # a literal brace, as in Python's re
                lo = int(m.group(1))
                hi = lo if m.group(2) is None else (int(m.group(3)) if m.group(3) else None)
                if hi is not None and hi < lo:
                    raise self.err("a repeat with max < min")
                n = m.end() - self.i
            else:
                break
            self.i += n
            if self.i < self.end and self.p[self.i] in "?+":
                raise self.err("a lazy or possessive quantifier")
            atom = ("rep", atom, lo, hi)
        return atom

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            self.i += 1
            if self.p.startswith("?:", self.i, self.end):
                self.i += 2
            elif self.i < self.end and self.p[self.i] == "?":
                raise self.err("a (?...) group (look-around, flags, named groups)")
            node = self.alt()
            if self.i >= self.end or self.p[self.i] != ")":
                raise self.err("an unclosed group")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            self.i += 1
            return _set(_negate([(10, 10)]))
        if c in "^$":
            raise self.err(f"an inner anchor {c!r}")
        if c in "?*+":
            raise self.err("a quantifier with nothing to repeat")
        if c == "\\":
            r = self.escape(False)
            return _set(r)
        self.i += 1
        return _set([(ord(c), ord(c))])

    def escape(self, in_class: bool) -> list:
        """The ranges an escape at ``self.i`` stands for."""
        self.i += 1
        if self.i >= self.end:
            raise self.err("a trailing backslash")
        c = self.p[self.i]
        self.i += 1
        if c in _CLASSES:
            return list(_CLASSES[c])
        if c in _ESC:
            return [(_ESC[c], _ESC[c])]
        if c in "xu":
            n = 2 if c == "x" else 4
            h = self.p[self.i:self.i + n]
            if len(h) != n or re.fullmatch(r"[0-9a-fA-F]+", h) is None:
                raise self.err(f"a malformed \\{c} escape")
            self.i += n
            v = int(h, 16)
            if 0xD800 <= v <= 0xDFFF:
                raise self.err("a surrogate code point")
            return [(v, v)]
        if c == "0" and not (self.i < self.end and self.p[self.i].isdigit()):
            return [(0, 0)]
        if c.isalnum() and c.isascii():
            raise self.err(f"the escape \\{c} (back-references and zero-width assertions included)")
        return [(ord(c), ord(c))]

    def klass(self):
        self.i += 1
        neg = self.i < self.end and self.p[self.i] == "^"
        if neg:
            self.i += 1
        ranges, first = [], True
        while True:
            if self.i >= self.end:
                raise self.err("an unclosed class")
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p.startswith("[:", self.i):
                raise self.err("a POSIX class")
            if c == "\\":
                r = self.escape(True)
                single = len(r) == 1 and r[0][0] == r[0][1]
            else:
                self.i += 1
                r, single = [(ord(c), ord(c))], True
            if (single and self.i + 1 < self.end and self.p[self.i] == "-" and self.p[self.i + 1] != "]"):
                self.i += 1
                if self.p[self.i] == "\\":
                    r2 = self.escape(True)
                    if not (len(r2) == 1 and r2[0][0] == r2[0][1]):
                        raise self.err("a class as a range end")
                else:
                    r2 = [(ord(self.p[self.i]), ord(self.p[self.i]))]
                    self.i += 1
                if r2[0][0] < r[0][0]:
                    raise self.err("a reversed range")
                r = [(r[0][0], r2[0][0])]
            ranges += r
        return _set(_negate(ranges) if neg else ranges)


# ---------------------------------------------------------------------------------------------
# code-point ranges -> UTF-8 byte-range sequences

_UTF8_MAX = (0x7F, 0x7FF, 0xFFFF, _MAX_CP)


def _utf8(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def _utf8_seqs(lo: int, hi: int, out: list) -> None:
    """Append byte-range sequences [(b_lo, b_hi), ...] that together match exactly [lo, hi]
    (no surrogates inside)."""
    for mx in _UTF8_MAX:  # split by encoded length
        if lo <= mx < hi:
            _utf8_seqs(lo, mx, out)
            _utf8_seqs(mx + 1, hi, out)
            return
    if hi <= 0x7F:
        out.append([(lo, hi)])
        return
    for k in (1, 2, 3):  # split so that the trailing k continuation bytes span their full range
        m = (1 << (6 * k)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                _utf8_seqs(lo, lo | m, out)
                _utf8_seqs((lo | m) + 1, hi, out)
                return
            if (hi & m) != m:
                _utf8_seqs(lo, (hi & ~m) - 1, out)
                _utf8_seqs(hi & ~m, hi, out)
                return
    a, b = _utf8(lo), _utf8(hi)
    out.append(list(zip(a, b)))


# ---------------------------------------------------------------------------------------------
# Thompson NFA over byte ranges


class _NFA:
    def __init__(self, cap: int):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple]] = []  # (lo, hi, target)
        self.cap = cap

    def new(self) -> int:
        if len(self.eps) >= self.cap:
            raise ValueError(f"guide too large: more than {self.cap} NFA states")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node, s: int) -> int:
        """Add ``node`` starting at state ``s``; returns its end state."""
        kind = node[0]
        if kind == "set":
            e = self.new()
            seqs: list = []
            for lo, hi in node[1]:
                _utf8_seqs(lo, hi, seqs)
            for seq in seqs:
                cur = s
                for j, (a, b) in enumerate(seq):
                    nxt = e if j == len(seq) - 1 else self.new()
                    self.edges[cur].append((a, b, nxt))
                    cur = nxt
            return e
        if kind == "cat":
            for ch in node[1]:
                s = self.build(ch, s)
            return s
        if kind == "alt":
            e = self.new()
            for ch in node[1]:
                a = self.new()
                self.eps[s].append(a)
                self.eps[self.build(ch, a)].append(e)
            return e
        if kind == "rep":
            _, ch, lo, hi = node
            for _ in range(lo):
                s = self.build(ch, s)
            if hi is None:
                a, e = self.new(), self.new()
                self.eps[s] += [a, e]
                b = self.build(ch, a)
                self.eps[b] += [a, e]
                return e
            e = self.new()
            for _ in range(hi - lo):
                self.eps[s].append(e)
                a = self.new()
                self.eps[s].append(a)
                s = self.build(ch, a)
            self.eps[s].append(e)
            return e
        raise AssertionError(kind)


def _to_dfa(nfa: _NFA, start: int, final: int, limit: int) -> tuple:
    """Subset construction; gives up past ``limit`` states."""
    eps, edges = nfa.eps, nfa.edges

    def closure(states) -> frozenset:
        seen, stack = set(states), list(states)
        while stack:
            for t in eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    s0 = closure([start])
    ids = {s0: 0}
    order = [s0]
    rows = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        es = [e for s in cur for e in edges[s]]
        row = np.full(256, -1, dtype=np.int32)
        if es:
            cuts = sorted({e[0] for e in es} | {e[1] + 1 for e in es})
            for a, b in zip(cuts, cuts[1:]):
                tg = [e[2] for e in es if e[0] <= a and b - 1 <= e[1]]
                if not tg:
                    continue
                nxt = closure(tg)
                j = ids.get(nxt)
                if j is None:
                    j = ids[nxt] = len(order)
                    order.append(nxt)
                    if j >= limit:
                        raise ValueError(f"guide too large: more than {limit} DFA states before minimisation")
                row[a:b] = j
        rows.append(row)
    trans = np.stack(rows)
    accept = np.array([final in s for s in order], dtype=bool)
    return trans, accept


def _trim_minimise(trans: np.ndarray, accept: np.ndarray) -> tuple:
    """Drop states that reach no accepting state, merge equivalent ones, number from the start
    state in breadth-first order."""
    n = trans.shape[0]
    # co-reachability by a backwards sweep
    live = accept.copy()
    while True:
        ext = np.concatenate([live, [False]])
        new = live | ext[trans].any(axis=1)
        if (new == live).all():
            break
        live = new
    if not live[0]:
        raise ValueError("the guide matches nothing")
    ext = np.concatenate([live, [False]])
    trans = np.where(ext[trans], trans, -1)
    keep = np.flatnonzero(live)
    remap = np.full(n + 1, -1, dtype=np.int64)
    remap[keep] = np.arange(len(keep))
    trans = remap[trans[keep]]  # -1 indexes the last entry: stays -1
    accept = accept[keep]
    # Moore refinement over byte classes (identical columns), so each round compares short rows
    _, col_first = np.unique(trans, axis=1, return_index=True)
    cols = trans[:, np.sort(col_first)]
    cls = accept.astype(np.int64)
    ncls = len(np.unique(cls))
    while True:
        ext_c = np.concatenate([cls, [-1]])
        sig = np.concatenate([cls[:, None], ext_c[cols]], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        k = int(new.max()) + 1
        cls = new
        if k == ncls:
            break
        ncls = k
    # one representative per class, numbered breadth-first from the start state's class
    rep = np.full(ncls, -1, dtype=np.int64)
    for s in range(len(cls) - 1, -1, -1):
        rep[cls[s]] = s
    ext_c = np.concatenate([cls, [-1]])
    ctrans = ext_c[trans[rep]]  # [ncls, 256] class -> class
    order, seen = [int(cls[0])], {int(cls[0])}
    i = 0
    while i < len(order):
        for t in ctrans[order[i]]:
            t = int(t)
            if t >= 0 and t not in seen:
                seen.add(t)
                order.append(t)
        i += 1
    pos = np.full(ncls + 1, -1, dtype=np.int64)
    pos[np.array(order)] = np.arange(len(order))
    out = pos[ctrans[np.array(order)]].astype(np.int32)
    acc = accept[rep[np.array(order)]]
    return out, acc


# ---------------------------------------------------------------------------------------------
# JSON schema -> AST

_ANNOTATIONS = {"title", "description", "$schema", "$id", "default", "examples"}
_INT = ("cat", [("rep", _lit("-"), 0, 1),
                ("alt", [_lit("0"), ("cat", [_set([(0x31, 0x39)]), ("rep", _set(_DIGIT), 0, 17)])])])
_NUMBER = ("cat", [_INT, ("rep", ("cat", [_lit("."), ("rep", _set(_DIGIT), 1, 17)]), 0, 1),
                   ("rep", ("cat", [_set([(0x45, 0x45), (0x65, 0x65)]),
                                    ("rep", _set([(0x2B, 0x2B), (0x2D, 0x2D)]), 0, 1),
                                    ("rep", _set(_DIGIT), 1, 2)]), 0, 1)])
_HEX = _set([(0x30, 0x39), (0x41, 0x46), (0x61, 0x66)])
_STR_CHAR = ("alt", [_set(_negate([(0, 0x1F), (0x22, 0x22), (0x5C, 0x5C)])),
                     ("cat", [_lit("\\"), ("alt", [_set([(ord(c), ord(c)) for c in '"\\/bfnrt']),
                                                  ("cat", [_lit("u"), ("rep", _HEX, 4, 4)])])])])


def _keys(schema: dict, allowed: set, what: str) -> None:
    bad = sorted(set(schema) - allowed - _ANNOTATIONS)
    if bad:
        raise ValueError(f"json_schema: keyword {bad[0]!r} is not supported ({what})")


def _count(schema: dict, key: str) -> Optional[int]:
    v = schema.get(key)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"json_schema: {key} must be a non-negative integer")
    return v


def _scalar(v):
    if v is not None and not isinstance(v, (str, int, float, bool)):
        raise ValueError("json_schema: enum / const values must be scalars")
    if isinstance(v, float) and (v != v or v in (float("inf"), float("-inf"))):
        raise ValueError("json_schema: enum / const values must be finite")
    return _lit(json.dumps(v, ensure_ascii=False, separators=(",", ":")))


def _schema(s, depth: int = 0):
    if not isinstance(s, dict):
        raise ValueError("json_schema: a schema must be an object")
    if depth > 32:
        raise ValueError("json_schema: nested too deeply")
    if "const" in s:
        _keys(s, {"const", "type"}, "const")
        return _scalar(s["const"])
    if "enum" in s:
        _keys(s, {"enum", "type"}, "enum")
        if not isinstance(s["enum"], list) or not s["enum"]:
            raise ValueError("json_schema: enum must be a non-empty list")
        return ("alt", [_scalar(v) for v in s["enum"]])
    t = s.get("type")
    if not isinstance(t, str):
        for k in ("$ref", "anyOf", "oneOf", "allOf", "not"):
            if k in s:
                raise ValueError(f"json_schema: keyword {k!r} is not supported")
        raise ValueError("json_schema: every schema needs a single 'type', an 'enum' or a 'const'")
    if t == "object":
        _keys(s, {"type", "properties", "required", "additionalProperties"}, "object")
        props = s.get("properties") or {}
        if not isinstance(props, dict):
            raise ValueError("json_schema: properties must be an object")
        items = [_lit("{")]
        for i, (k, v) in enumerate(props.items()):
            items += [_lit(("," if i else "") + json.dumps(str(k), ensure_ascii=False) + ":"), _schema(v, depth + 1)]
        return ("cat", items + [_lit("}")])
    if t == "array":
        _keys(s, {"type", "items", "minItems", "maxItems"}, "array")
        if "items" not in s:
            raise ValueError("json_schema: an array needs 'items'")
        item = _schema(s["items"], depth + 1)
        lo, hi = _count(s, "minItems") or 0, _count(s, "maxItems")
        if hi is not None and hi < lo:
            raise ValueError("json_schema: maxItems < minItems")
        if hi == 0:
            return _lit("[]")
        more = ("rep", ("cat", [_lit(","), item]), max(lo - 1, 0), None if hi is None else hi - 1)
        body = ("cat", [item, more])
        return ("cat", [_lit("["), body if lo > 0 else ("rep", body, 0, 1), _lit("]")])
    if t == "string":
        _keys(s, {"type", "minLength", "maxLength"}, "string")
        lo, hi = _count(s, "minLength") or 0, _count(s, "maxLength")
        if hi is not None and hi < lo:
            raise ValueError("json_schema: maxLength < minLength")
        return ("cat", [_lit('"'), ("rep", _STR_CHAR, lo, hi), _lit('"')])
    if t in ("integer", "number", "boolean", "null"):
        _keys(s, {"type"}, t)
        return {"integer": _INT, "number": _NUMBER, "boolean": ("alt", [_lit("true"), _lit("false")]),
                "null": _lit("null")}[t]
    raise ValueError(f"json_schema: type {t!r} is not supported")


# ---------------------------------------------------------------------------------------------


class Guide:
    """A trimmed, minimal DFA over bytes: ``trans`` int32 ``[n, 256]`` (-1 = dead), ``accept`` bool
    ``[n]``, start state 0; every state reaches an accepting one.  ``key`` is the canonical spec
    text (what resident guides are keyed by)."""

    def __init__(self, trans: np.ndarray, accept: np.ndarray, key: str):
        self.trans = np.ascontiguousarray(trans, dtype=np.int32)
        self.accept = np.ascontiguousarray(accept, dtype=bool)
        self.key = key
        self.trans.setflags(write=False)
        self.accept.setflags(write=False)

    @property
    def n(self) -> int:
        return int(self.trans.shape[0])

    def walk(self, state: int, data: bytes) -> int:
        """The state after ``data`` from ``state`` (-1: dead)."""
        t = self.trans
        for b in data:
            if state < 0:
                break
            state = int(t[state, b])
        return state

    def matches(self, data) -> bool:
        if isinstance(data, str):
            data = data.encode("utf-8")
        s = self.walk(0, data)
        return s >= 0 and bool(self.accept[s])


def canonical_spec(spec) -> str:
    """The spec as canonical text (the cache key); ``ValueError`` for anything but one of the
    three forms."""
    if not isinstance(spec, dict) or len(spec) != 1:
        raise ValueError("a guide is one of {'choice': [...]}, {'regex': '...'}, {'json_schema': {...}}")
    (kind, val), = spec.items()
    if kind == "choice":
        if not isinstance(val, (list, tuple)) or not val or not all(isinstance(c, str) for c in val):
            raise ValueError("guide choice: a non-empty list of strings")
        val = list(val)
    elif kind == "regex":
        if not isinstance(val, str):
            raise ValueError("guide regex: a string")
    elif kind == "json_schema":
        if not isinstance(val, dict):
            raise ValueError("guide json_schema: a schema object")
        if val.get("type") == "json_object" or not val:
            raise ValueError("a JSON schema is needed: free-form JSON is not a regular language")
    else:
        raise ValueError(f"unknown guide kind {kind!r}: choice, regex or json_schema")
    try:
        return json.dumps({kind: val}, ensure_ascii=False, separators=(",", ":"))  # key order is part of a schema
    except (TypeError, ValueError) as e:
        raise ValueError(f"guide spec is not plain data: {e}") from None


_cache: "OrderedDict[tuple, Guide]" = OrderedDict()
_cache_lock = threading.Lock()


def compile_guide(spec, max_states: int = DEFAULT_MAX_STATES) -> Guide:
    """Compile (or fetch from the LRU cache) the guide for ``spec``; ``ValueError`` for a spec
    outside the supported subsets or a DFA of more than ``max_states`` states."""
    key = canonical_spec(spec)
    max_states = int(max_states)
    with _cache_lock:
        g = _cache.get((key, max_states))
        if g is not None:
            _cache.move_to_end((key, max_states))
            return g
    (kind, val), = spec.items()
    if kind == "choice":
        ast = ("alt", [_lit(c) for c in val])
    elif kind == "regex":
        ast = _Parser(val).parse()
    else:
        ast = _schema(val)
    nfa = _NFA(cap=max(20000, 64 * max_states))
    start = nfa.new()
    final = nfa.build(ast, start)
    trans, accept = _to_dfa(nfa, start, final, _BLOWUP * max_states)
    trans, accept = _trim_minimise(trans, accept)
    if trans.shape[0] > max_states:
        raise ValueError(f"guide too large: {trans.shape[0]} states, the limit (guide_max_states) is {max_states}")
    g = Guide(trans, accept, key)
    with _cache_lock:
        _cache[(key, max_states)] = g
        while len(_cache) > _CACHE_SIZE:
            _cache.popitem(last=False)
    return g
