"""Byte-level automata that constrain sampling (pure Python and NumPy; no device code here).

A ``Dfa`` reads the UTF-8 bytes of the generated text.  ``runtime.compile_constraint`` turns
one into per-state token masks (cs_dfa_token_masks); the sampling entries then draw only
tokens whose bytes keep the automaton alive (cs_vocab_sample_dfa, cs_sample_step_dfa).

``compile_regex`` serves a subset of Python's ``re`` syntax with FULL-match semantics (the
whole generated text must match):

    literals and escapes   a  \\.  \\n \\t \\r \\f \\v \\a \\0  \\xHH  \\uHHHH  \\UHHHHHHHH
    any character          .            one well-formed UTF-8 character except "\\n"
    classes                [abc] [a-z0-9_] [^"\\\\]   a negated class matches one well-formed
                                        UTF-8 character outside the set ("\\n" included)
    shorthands             \\d \\w \\s and \\D \\W \\S, ASCII as under re.ASCII; \\d \\w \\s also
                                        inside a class
    groups, alternation    ( ) (?: ) |
    repetition             * + ? {m} {m,} {,n} {m,n}    (greedy spelling only: a full match
                                        does not depend on greed)

A non-ASCII literal stands for its UTF-8 bytes.  Everything else -- anchors (^ $ \\A \\Z \\b
\\B), backreferences, lookaround, named groups, inline flags, lazy and possessive quantifiers,
negated shorthands inside a class -- raises ValueError naming the construct.

``json_object`` is the grammar of one RFC 8259 object with a bounded nesting depth, built from
an explicit stack machine, not through a regex.  ``union`` puts several automata into one
table so that the streams of one batch differ in their start state only.
"""
from __future__ import annotations

import functools
import hashlib
from typing import Callable, Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import CSError

MAX_STATES = 1024          # the device entries' limit (cs_dfa_token_masks)
_MAX_RAW_STATES = 1 << 16  # before minimisation
_MAX_CP = 0x10FFFF


class Dfa:
    """A trimmed deterministic automaton over bytes: ``trans`` int16 [n_states, 256] (-1:
    dead), ``accept`` bool [n_states], ``start``.  Every state can reach an accepting one."""

    def __init__(self, trans: np.ndarray, accept: np.ndarray, start: int) -> None:
        trans = np.array(trans, dtype=np.int16, order="C")          # copies: frozen below
        accept = np.array(accept, dtype=bool, order="C")
        if trans.ndim != 2 or trans.shape[1] != 256 or accept.shape != (trans.shape[0],):
            raise ValueError("trans must be [n_states, 256] and accept [n_states]")
        if trans.shape[0] > MAX_STATES:
            raise CSError(f"automaton has {trans.shape[0]} states, the limit is {MAX_STATES}")
        if not 0 <= int(start) < trans.shape[0]:
            raise ValueError("start is not a state")
        trans.setflags(write=False)                     # shared by caches: never edited
        accept.setflags(write=False)
        self.trans, self.accept, self.start = trans, accept, int(start)
        self._key: Optional[str] = None

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    def walk(self, state: int, data: bytes) -> int:
        """The state after ``data`` from ``state``; -1 once a byte has no transition."""
        q = int(state)
        for b in bytes(data):
            if q < 0:
                return -1
            q = int(self.trans[q, b])
        return q

    def accepts(self, data: bytes) -> bool:
        q = self.walk(self.start, data)
        return q >= 0 and bool(self.accept[q])

    def key(self) -> str:
        """A digest of the table (cache key of the masks built from it)."""
        if self._key is None:
            h = hashlib.sha256(self.trans.tobytes())
            h.update(np.packbits(self.accept).tobytes() + b"%d" % self.start)
            self._key = h.hexdigest()
        return self._key


# --- from a raw table to a Dfa: trim, minimise, renumber --------------------------------------

def _finish(trans: np.ndarray, accept: np.ndarray, start: int) -> Dfa:
    """Trim (drop states that cannot reach an accepting one), minimise (Moore's partition
    refinement) and renumber in breadth-first order from the start state."""
    n = trans.shape[0]
    trans = trans.astype(np.int64)
    # co-reachable states: a backward fixed point
    live = accept.copy()
    while True:
        tgt_live = np.concatenate([live, [False]])[trans]          # -1 -> the appended False
        new = live | tgt_live.any(axis=1)
        if (new == live).all():
            break
        live = new
    if not live[start]:
        raise ValueError("the pattern matches nothing")
    trans = np.where(np.concatenate([live, [False]])[trans], trans, -1)
    # reachable states
    seen = np.zeros(n, dtype=bool)
    seen[start] = True
    frontier = [start]
    while frontier:
        nxt = np.unique(trans[frontier])
        nxt = nxt[nxt >= 0]
        nxt = nxt[~seen[nxt]]
        seen[nxt] = True
        frontier = nxt.tolist()
    keep = np.flatnonzero(seen & live)
    remap = np.full(n + 1, -1, dtype=np.int64)
    remap[keep] = np.arange(keep.size)
    trans, accept, start = remap[trans[keep]], accept[keep], int(remap[start])
    # Moore: refine by (own class, classes of the 256 successors) until stable; dead = class 0
    # (bytes that every state treats alike form one column: a chain of n states takes n rounds)
    cols = np.unique(trans, axis=1)
    labels = accept.astype(np.int64) + 1
    count = len(np.unique(labels))
    while True:
        succ = np.concatenate([labels, [0]])[cols]
        sig = np.concatenate([labels[:, None], succ], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1) + 1
        k = int(new.max())
        labels = new
        if k == count:
            break
        count = k
    k = count
    rep = np.zeros(k, dtype=np.int64)
    rep[labels - 1] = np.arange(labels.size)          # any member represents its class
    ctrans = np.concatenate([labels - 1, [-1]])[trans[rep]]
    caccept = accept[rep]
    cstart = int(labels[start] - 1)
    # breadth-first renumbering: one spelling per language
    order, pos = [cstart], {cstart: 0}
    for q in order:
        for t in ctrans[q].tolist():
            if t >= 0 and t not in pos:
                pos[t] = len(order)
                order.append(t)
    perm = np.full(k + 1, -1, dtype=np.int64)
    perm[order] = np.arange(len(order))
    if len(order) > MAX_STATES:
        raise CSError(f"automaton has {len(order)} states, the limit is {MAX_STATES}")
    return Dfa(perm[ctrans[order]].astype(np.int16), caccept[order], 0)


def _explore(start: Hashable, step: Callable[[Hashable, int], Optional[Hashable]],
             accepting: Callable[[Hashable], bool]) -> Dfa:
    """The automaton of a step function over hashable states, enumerated from ``start``."""
    ids: Dict[Hashable, int] = {start: 0}
    order = [start]
    rows: List[List[int]] = []
    for st in order:
        row = [-1] * 256
        for b in range(256):
            nx = step(st, b)
            if nx is None:
                continue
            if nx not in ids:
                if len(order) >= _MAX_RAW_STATES:
                    raise CSError("automaton too large")
                ids[nx] = len(order)
                order.append(nx)
            row[b] = ids[nx]
        rows.append(row)
    return _finish(np.asarray(rows, dtype=np.int64),
                   np.asarray([accepting(s) for s in order], dtype=bool), 0)


# --- UTF-8 ------------------------------------------------------------------------------------

def _utf8_seqs(lo: int, hi: int) -> List[List[Tuple[int, int]]]:
    """Byte-range sequences that match exactly the UTF-8 encodings of code points [lo, hi]
    (surrogates excluded)."""
    out: List[List[Tuple[int, int]]] = []
    if lo <= 0xDFFF and hi >= 0xD800:                  # cut the surrogates out
        if lo < 0xD800:
            out += _utf8_seqs(lo, 0xD7FF)
        if hi > 0xDFFF:
            out += _utf8_seqs(0xE000, hi)
        return out
    for n, (a, b) in enumerate(((0, 0x7F), (0x80, 0x7FF), (0x800, 0xFFFF), (0x10000, _MAX_CP)), 1):
        l, h = max(lo, a), min(hi, b)
        if l <= h:
            _split_utf8(l, h, n, out)
    return out


def _split_utf8(l: int, h: int, n: int, out) -> None:
    if n == 1:
        out.append([(l, h)])
        return
    for i in range(1, n):
        m = (1 << (6 * i)) - 1
        if (l & ~m) != (h & ~m):
            if l & m:
                _split_utf8(l, l | m, n, out)
                _split_utf8((l | m) + 1, h, n, out)
                return
            if (h & m) != m:
                _split_utf8(l, (h & ~m) - 1, n, out)
                _split_utf8(h & ~m, h, n, out)
                return
    a, b = chr(l).encode("utf-8"), chr(h).encode("utf-8")
    out.append(list(zip(a, b)))


def _norm(ranges) -> List[Tuple[int, int]]:
    """Sorted, merged code point ranges."""
    out: List[List[int]] = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(a, b) for a, b in out]


def _negate(ranges) -> List[Tuple[int, int]]:
    out, at = [], 0
    for lo, hi in _norm(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= _MAX_CP:
        out.append((at, _MAX_CP))
    return out


# --- the regex subset -------------------------------------------------------------------------

_DIGIT = [(0x30, 0x39)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_SPACE = [(0x09, 0x0D), (0x20, 0x20)]
_SHORT = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_CTRL = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "a": 7, "0": 0}
_HEXLEN = {"x": 2, "u": 4, "U": 8}


class _Parser:
    """Pattern -> tree of ("set", ranges) / ("cat", nodes) / ("alt", nodes) /
    ("rep", node, m, n or None)."""

    def __init__(self, pattern: str) -> None:
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"unsupported in a constraint pattern: {what} (at offset {self.i} of "
                         f"{self.p!r})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced parenthesis")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.repeat())
        return ("cat", items)

    def quantifier(self) -> Optional[Tuple[int, Optional[int]]]:
        c = self.peek()
        if c == "*":
            self.i += 1
            return 0, None
        if c == "+":
            self.i += 1
            return 1, None
        if c == "?":
            self.i += 1
            return 0, 1
        if c == "{":
            j = self.p.find("}", self.i)
            body = self.p[self.i + 1:j] if j > 0 else None
            if body is None:
                return None
            lo, sep, hi = body.partition(",")
            if not (lo.isdigit() or (lo == "" and sep)) or not (hi.isdigit() or hi == "") \
                    or not (lo + hi).isascii() or body in ("", ","):
                return None                            # a literal brace, as in re
            m = int(lo) if lo else 0
            n = m if not sep else (int(hi) if hi else None)
            if n is not None and n < m:
                self.fail("a repetition {m,n} with n < m")
            self.i = j + 1
            return m, n
        return None

    def repeat(self):
        node = self.atom()
        q = self.quantifier()
        if q is None:
            return node
        if self.peek() == "?":
            self.fail("lazy quantifier")
        if self.peek() == "+":
            self.fail("possessive quantifier")
        if self.peek() in ("*",) or (self.peek() == "{" and self.quantifier_ahead()):
            self.fail("multiple repeat")
        return ("rep", node, q[0], q[1])

    def quantifier_ahead(self) -> bool:
        at = self.i
        try:
            return self.quantifier() is not None
        finally:
            self.i = at

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("lookaround")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    self.fail("named group")
                elif nxt[:1] == "#":
                    self.fail("comment group")
                else:
                    self.fail("inline flags or a conditional group")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced parenthesis")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            self.i += 1
            return ("set", _negate([(10, 10)]))
        if c in "^$":
            self.fail(f"anchor {c}")
        if c in "*+?":
            self.fail("nothing to repeat")
        if c == "\\":
            kind, val = self.escape(in_class=False)
            return ("set", val if kind == "set" else [(val, val)])
        self.i += 1
        return ("set", [(ord(c), ord(c))])

    def escape(self, in_class: bool):
        """After a backslash: ("cp", code point) or ("set", ranges)."""
        self.i += 1
        c = self.peek()
        if c == "":
            self.fail("a trailing backslash")
        self.i += 1
        if c in _SHORT:
            return "set", list(_SHORT[c])
        if c in "DWS":
            if in_class:
                self.fail(f"negated shorthand \\{c} inside a class")
            return "set", _negate(_SHORT[c.lower()])
        if c in _HEXLEN:
            n = _HEXLEN[c]
            digits = self.p[self.i:self.i + n]
            if len(digits) != n or any(d not in "0123456789abcdefABCDEF" for d in digits):
                self.fail(f"incomplete escape \\{c}")
            self.i += n
            cp = int(digits, 16)
            if cp > _MAX_CP or 0xD800 <= cp <= 0xDFFF:
                self.fail("an escape that is no Unicode scalar value")
            return "cp", cp
        if c in _CTRL:
            if c == "0" and self.peek().isdigit():
                self.fail("octal escape")
            return "cp", _CTRL[c]
        if c.isdigit():
            self.fail("backreference")
        if c in "AZbB" and not (in_class and c == "b"):
            self.fail(f"anchor \\{c}")
        if c == "b":
            return "cp", 8
        if c.isalpha() and c.isascii():
            self.fail(f"escape \\{c}")
        return "cp", ord(c)

    def char_class(self):
        self.i += 1
        negated = self.peek() == "^"
        if negated:
            self.i += 1
        ranges: List[Tuple[int, int]] = []
        first = True
        while True:
            c = self.peek()
            if c == "":
                self.fail("unterminated class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i + 1:self.i + 2] == ":":
                self.fail("POSIX class")
            if c == "\\":
                kind, val = self.escape(in_class=True)
                if kind == "set":
                    ranges += val
                    continue
                lo = val
            else:
                self.i += 1
                lo = ord(c)
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                if self.peek() == "\\":
                    kind, hi = self.escape(in_class=True)
                    if kind == "set":
                        self.fail("a range that ends in a shorthand")
                else:
                    hi = ord(self.peek())
                    self.i += 1
                if hi < lo:
                    self.fail("a reversed range")
                ranges.append((lo, hi))
            else:
                ranges.append((lo, lo))
        return ("set", _negate(ranges) if negated else _norm(ranges))


class _Nfa:
    def __init__(self) -> None:
        self.eps: List[List[int]] = []
        self.arcs: List[List[Tuple[int, int, int]]] = []

    def new(self) -> int:
        self.eps.append([])
        self.arcs.append([])
        if len(self.eps) > (1 << 20):
            raise CSError("pattern too large")
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            for lo, hi in node[1]:
                for seq in _utf8_seqs(lo, hi):
                    at = s
                    for k, (a, b) in enumerate(seq):
                        to = e if k == len(seq) - 1 else self.new()
                        self.arcs[at].append((a, b, to))
                        at = to
            return s, e
        if kind == "cat":
            s = e = self.new()
            for sub in node[1]:
                a, b = self.build(sub)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for sub in node[1]:
                a, b = self.build(sub)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, m, n = node
        s = e = self.new()
        for _ in range(m):
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        if n is None:                                   # a star after the m copies
            a, b = self.build(sub)
            hub = self.new()
            self.eps[e].append(hub)
            self.eps[hub].append(a)
            self.eps[b].append(hub)
            return s, hub
        end = self.new()
        for _ in range(n - m):                          # optional copies, each may leave
            self.eps[e].append(end)
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        self.eps[e].append(end)
        return s, end


def compile_regex(pattern: str) -> Dfa:
    """The minimal automaton of ``pattern`` (the subset in the module's docstring), full match."""
    if not isinstance(pattern, str):
        raise TypeError("pattern must be a str")
    tree = _Parser(pattern).parse()
    nfa = _Nfa()
    s0, final = nfa.build(tree)
    closures: Dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out = set()
        for s in states:
            c = closures.get(s)
            if c is None:
                acc, stack = {s}, [s]
                while stack:
                    for t in nfa.eps[stack.pop()]:
                        if t not in acc:
                            acc.add(t)
                            stack.append(t)
                c = closures[s] = frozenset(acc)
            out |= c
        return frozenset(out)

    start = closure([s0])
    ids = {start: 0}
    order = [start]
    rows = []
    for cur in order:
        row = np.full(256, -1, dtype=np.int64)
        arcs = [a for s in cur for a in nfa.arcs[s]]
        cuts = sorted({a[0] for a in arcs} | {a[1] + 1 for a in arcs})
        for lo, hi in zip(cuts, cuts[1:]):
            tg = {t for a, b, t in arcs if a <= lo <= b}
            if not tg:
                continue
            nx = closure(tg)
            if nx not in ids:
                if len(order) >= _MAX_RAW_STATES:
                    raise CSError(f"pattern needs more than {_MAX_RAW_STATES} states before "
                                  f"minimisation; the limit after it is {MAX_STATES}")
                ids[nx] = len(order)
                order.append(nx)
            row[lo:hi] = ids[nx]
        rows.append(row)
    return _finish(np.stack(rows), np.asarray([final in s for s in order], dtype=bool), 0)


# --- JSON -------------------------------------------------------------------------------------

_WS = (0x20, 0x0A)
_MAX_WS = 2
_HEX = frozenset(b"0123456789abcdefABCDEF")
_ESC = frozenset(b'"\\/bfnrt')
_LITERALS = {ord("t"): b"rue", ord("f"): b"alse", ord("n"): b"ull"}


def _utf8_lead(b: int):
    """(continuation bytes left, range of the next byte) after lead byte b, or None."""
    if 0xC2 <= b <= 0xDF:
        return 1, (0x80, 0xBF)
    if b == 0xE0:
        return 2, (0xA0, 0xBF)
    if b == 0xED:
        return 2, (0x80, 0x9F)
    if 0xE1 <= b <= 0xEF:
        return 2, (0x80, 0xBF)
    if b == 0xF0:
        return 3, (0x90, 0xBF)
    if 0xF1 <= b <= 0xF3:
        return 3, (0x80, 0xBF)
    if b == 0xF4:
        return 3, (0x80, 0x8F)
    return None


def json_object(max_depth: int = 2) -> Dfa:
    """The automaton of one JSON object (see _json_object), built once per depth."""
    max_depth = int(max_depth)
    if not 1 <= max_depth <= 3:
        raise ValueError("json_object: max_depth must be 1, 2 or 3")
    return _json_object(max_depth)


@functools.lru_cache(maxsize=None)
def _json_object(max_depth: int) -> Dfa:
    """The automaton of ONE JSON object (RFC 8259) whose values nest at most ``max_depth``
    levels (the top object is level 1; 1 <= max_depth <= 3).  Strings hold printable ASCII,
    the JSON escapes and well-formed multi-byte UTF-8; numbers follow JSON's grammar; between
    tokens at most two bytes of whitespace from {space, "\\n"} are allowed, none before the
    opening or after the closing brace.

    A state is (stack of open containers, mode, detail): the stack is explicit and bounded,
    which is what keeps the language regular."""
    # modes that sit between tokens carry the whitespace count as their detail:
    #   "obj0" after "{": a key or "}"      "key" after "," in an object: a key
    #   "colon" after a key: ":"            "val" after ":" / "," in an array: a value
    #   "arr0" after "[": a value or "]"    "after" after a value: "," or the closing bracket
    def value_start(stack, b):
        if b == 0x22:
            return (stack, "str", False)
        if b == 0x2D:
            return (stack, "num", "-")
        if b == 0x30:
            return (stack, "num", "0")
        if 0x31 <= b <= 0x39:
            return (stack, "num", "i")
        if b in _LITERALS:
            return (stack, "lit", _LITERALS[b])
        if b == 0x7B and len(stack) < max_depth:
            return (stack + "O", "obj0", 0)
        if b == 0x5B and len(stack) < max_depth:
            return (stack + "A", "arr0", 0)
        return None

    def after_value(stack, b, ws):
        if b in _WS:
            return (stack, "after", ws + 1) if ws < _MAX_WS else None
        top = stack[-1]
        if b == 0x2C:
            return (stack, "key" if top == "O" else "val", 0)
        if b == (0x7D if top == "O" else 0x5D):
            return closed(stack[:-1])
        return None

    def closed(stack):
        return (stack, "end", 0) if not stack else (stack, "after", 0)

    def step(st, b):
        stack, mode, d = st
        if mode == "start":
            return ("O", "obj0", 0) if b == 0x7B else None
        if mode == "end":
            return None
        if mode in ("obj0", "key", "colon", "val", "arr0") and b in _WS:
            return (stack, mode, d + 1) if d < _MAX_WS else None
        if mode == "obj0":
            if b == 0x7D:
                return closed(stack[:-1])
            return (stack, "str", True) if b == 0x22 else None
        if mode == "key":
            return (stack, "str", True) if b == 0x22 else None
        if mode == "colon":
            return (stack, "val", 0) if b == 0x3A else None
        if mode == "val":
            return value_start(stack, b)
        if mode == "arr0":
            return closed(stack[:-1]) if b == 0x5D else value_start(stack, b)
        if mode == "after":
            return after_value(stack, b, d)
        if mode == "lit":
            if b != d[0]:
                return None
            return (stack, "lit", d[1:]) if len(d) > 1 else (stack, "after", 0)
        if mode == "num":
            digit = 0x30 <= b <= 0x39
            if d == "-":
                return (stack, "num", "0" if b == 0x30 else "i") if digit else None
            if d in ("0", "i", "f", "x"):               # a complete number: may go on or end
                if digit and d != "0":
                    return st
                if b == 0x2E and d in ("0", "i"):
                    return (stack, "num", ".")
                if b in (0x65, 0x45) and d != "x":
                    return (stack, "num", "e")
                return after_value(stack, b, 0)
            if d == ".":
                return (stack, "num", "f") if digit else None
            if d == "e":
                if b in (0x2B, 0x2D):
                    return (stack, "num", "s")
                return (stack, "num", "x") if digit else None
            return (stack, "num", "x") if digit else None          # "s": after the sign
        # strings: d is True for a key; the sub-modes carry (is key, detail)
        if mode == "str":
            if b == 0x22:
                return (stack, "colon", 0) if d else (stack, "after", 0)
            if b == 0x5C:
                return (stack, "esc", d)
            if 0x20 <= b <= 0x7E:
                return st
            lead = _utf8_lead(b)
            return (stack, "u8", (d, lead[0], lead[1])) if lead else None
        if mode == "esc":
            if b in _ESC:
                return (stack, "str", d)
            return (stack, "hex", (d, 4)) if b == 0x75 else None
        if mode == "hex":
            if b not in _HEX:
                return None
            return (stack, "hex", (d[0], d[1] - 1)) if d[1] > 1 else (stack, "str", d[0])
        if mode == "u8":
            key, left, (lo, hi) = d
            if not lo <= b <= hi:
                return None
            return (stack, "u8", (key, left - 1, (0x80, 0xBF))) if left > 1 else (stack, "str", key)
        raise AssertionError(mode)

    return _explore(("", "start", 0), step, lambda st: st[1] == "end")


# --- several automata in one table ------------------------------------------------------------

def union(dfas: Sequence[Dfa]) -> Tuple[Dfa, List[int]]:
    """(one Dfa holding every automaton of ``dfas`` side by side, their start states): the
    parts are disjoint, so a stream started in starts[k] follows dfas[k] alone.  The table's
    own ``start`` is starts[0].  Equal automata share one copy."""
    dfas = list(dfas)
    if not dfas:
        raise ValueError("union of no automata")
    offs: Dict[str, int] = {}
    parts, starts, total = [], [], 0
    for d in dfas:
        if d.key() not in offs:
            offs[d.key()] = total
            parts.append(d)
            total += d.n_states
        starts.append(offs[d.key()] + d.start)
    if total > MAX_STATES:
        raise CSError(f"the automata have {total} states together, the limit is {MAX_STATES}")
    trans = np.full((total, 256), -1, dtype=np.int16)
    accept = np.zeros(total, dtype=bool)
    at = 0
    for d in parts:
        n = d.n_states
        trans[at:at + n] = np.where(d.trans >= 0, d.trans + at, -1)
        accept[at:at + n] = d.accept
        at += n
    return Dfa(trans, accept, starts[0]), starts
