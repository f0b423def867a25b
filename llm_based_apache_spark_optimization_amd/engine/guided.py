"""Regex-constrained decoding, host side: a regular expression compiled to a byte-level DFA.

The pattern is matched against the UTF-8 bytes of the generated text, anchored at both ends (a full match).  The
compiled table is what ``ops.dfa_mask`` (kernels/guided.hip) walks on the device, one vocabulary token per thread:

    cls[256]      u8   byte -> equivalence class (bytes no transition tells apart share a class)
    trans[S * C]  u16  trans[s * C + cls[byte]] -> next state, DEAD (0xFFFF) when no match can follow
    accept[S]     u8   1 where the text read so far is a full match
    start              the state before any byte (always 0 after the renumbering)

Every state from which no accepting state can be reached is folded into DEAD, so "the token keeps the DFA alive" is
one comparison.  ``S * C <= MAX_TABLE`` (32768 entries = 64 KiB of u16): the table then sits in the LDS whole.

Supported syntax: literals (a non-ASCII literal is its UTF-8 byte sequence, quantified as a whole), the escapes
``\\d \\w \\s \\n \\t \\r`` (ASCII classes, as ``re`` on a bytes pattern) and an escaped metacharacter, ``.`` (any byte but
``\\n``), classes ``[a-z0-9_]`` / ``[^...]`` (over bytes, ASCII members only), groups ``( )``, alternation ``|``, the
quantifiers ``* + ? {m} {m,} {m,n}`` and a leading ``(?i)`` (ASCII case-insensitivity).  Anything else -- anchors,
back-references, look-around, lazy or possessive quantifiers, ``(?:`` and inline flags elsewhere -- raises ValueError
naming the offending position.
"""
from __future__ import annotations

import functools
from typing import Optional

import numpy as np

DEAD = 0xFFFF
MAX_TABLE = 32768       # S * C entries of u16: 64 KiB, the kernel's LDS table
MAX_TOKEN_BYTES = 32    # longer vocabulary entries are never allowed under a constraint
_MAX_NFA = 1 << 16      # Thompson states (bounded repeats are expanded)
_MAX_RAW_DFA = 1 << 16  # subset-construction states before minimisation


class GuidedRequestError(ValueError):
    """A request's regex cannot be served: unsupported syntax, a table past the size rule, an engine built without
    guided decoding, or a combination the engine rejects.  The HTTP layer answers it with 400."""


_ALL = (1 << 256) - 1


def _mask(chars) -> int:
    m = 0
    for c in chars:
        m |= 1 << c
    return m


_DIGIT = _mask(range(0x30, 0x3A))
_WORD = _DIGIT | _mask(range(0x41, 0x5B)) | _mask(range(0x61, 0x7B)) | (1 << 0x5F)
_SPACE = _mask(b" \t\n\r\f\v")
_ESC_CLASS = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_ESC_CHAR = {"n": 0x0A, "t": 0x09, "r": 0x0D}


def _fold(m: int) -> int:
    """ASCII case closure of a byte set."""
    up = (m >> 0x41) & ((1 << 26) - 1)
    lo = (m >> 0x61) & ((1 << 26) - 1)
    return m | (lo << 0x41) | (up << 0x61)


class _Parser:
    """Recursive descent into a small AST: ("set", mask) | ("cat", [..]) | ("alt", [..]) | ("rep", node, lo, hi)."""

    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0
        self.icase = False
        if pattern.startswith("(?i)"):
            self.icase = True
            self.i = 4

    def err(self, what: str, pos: Optional[int] = None):
        pos = self.i if pos is None else pos
        return ValueError(f"unsupported regex syntax at position {pos}: {what} (pattern {self.p!r})")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            raise self.err("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.seq()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.seq())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def seq(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        node = self.atom()
        if self.i < len(self.p) and self.p[self.i] in "*+?{":
            c = self.p[self.i]
            if c == "{":
                lo, hi = self.braces()
            else:
                self.i += 1
                lo, hi = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
            if self.i < len(self.p) and self.p[self.i] in "?+":
                raise self.err("lazy / possessive quantifier")
            if self.i < len(self.p) and self.p[self.i] in "*{":
                raise self.err("multiple repeat")
            node = ("rep", node, lo, hi)
        return node

    def braces(self):
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j > 0 else ""
        parts = body.split(",")
        if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and
                                                                 not parts[1].isdigit()):
            raise self.err("malformed {m,n} quantifier")
        lo = int(parts[0])
        hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if hi is not None and hi < lo:
            raise self.err("{m,n} with n < m")
        self.i = j + 1
        return lo, hi

    def lit(self, byte: int):
        m = 1 << byte
        return ("set", _fold(m) if self.icase else m)

    def escape(self, in_class: bool) -> int:
        """The byte set of the escape at self.i (pointing at the backslash); advances past it."""
        if self.i + 1 >= len(self.p):
            raise self.err("trailing backslash")
        c = self.p[self.i + 1]
        if c in _ESC_CLASS:
            m = _ESC_CLASS[c]
        elif c in _ESC_CHAR:
            m = 1 << _ESC_CHAR[c]
        elif ord(c) < 128 and not c.isalnum():
            m = 1 << ord(c)
        else:
            raise self.err(f"escape \\{c}")
        self.i += 2
        return m

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            if self.p.startswith("(?", self.i):
                raise self.err("group extension (only a leading (?i) is supported)")
            self.i += 1
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                raise self.err("missing ')'")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            self.i += 1
            return ("set", _ALL & ~(1 << 0x0A))
        if c == "\\":
            m = self.escape(False)
            return ("set", _fold(m) if self.icase else m)
        if c in "*+?{":
            raise self.err("nothing to repeat")
        if c in "^$":
            raise self.err("anchor (the pattern is always a full match)")
        if c in "]}":
            raise self.err(f"unescaped {c!r}")
        self.i += 1
        if ord(c) < 128:
            return self.lit(ord(c))
        return ("cat", [("set", 1 << b) for b in c.encode("utf-8")])

    def klass(self):
        start = self.i
        self.i += 1
        neg = self.i < len(self.p) and self.p[self.i] == "^"
        if neg:
            self.i += 1
        m, first = 0, True
        while True:
            if self.i >= len(self.p):
                raise self.err("missing ']'", start)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "\\":
                one = self.escape(True)
                single = one if one & (one - 1) == 0 else None
            else:
                if ord(c) >= 128:
                    raise self.err("non-ASCII character in a class")
                if c == "[" and self.p.startswith("[:", self.i):
                    raise self.err("POSIX class")
                one = 1 << ord(c)
                single = one
                self.i += 1
            if (single is not None and self.i + 1 < len(self.p) and self.p[self.i] == "-"
                    and self.p[self.i + 1] != "]"):
                self.i += 1
                d = self.p[self.i]
                if d == "\\":
                    hi_m = self.escape(True)
                    if hi_m & (hi_m - 1):
                        raise self.err("class escape as a range end")
                else:
                    if ord(d) >= 128:
                        raise self.err("non-ASCII character in a class")
                    hi_m = 1 << ord(d)
                    self.i += 1
                lo_b, hi_b = single.bit_length() - 1, hi_m.bit_length() - 1
                if hi_b < lo_b:
                    raise self.err("reversed range in a class")
                one = _mask(range(lo_b, hi_b + 1))
            m |= one
        if self.icase:
            m = _fold(m)
        return ("set", (_ALL & ~m) if neg else m)


class _Nfa:
    def __init__(self):
        self.eps: list = []   # state -> list of states
        self.edge: list = []  # state -> (mask, target) or None

    def new(self) -> int:
        if len(self.eps) >= _MAX_NFA:
            raise ValueError("pattern too large: more than %d NFA states" % _MAX_NFA)
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node) -> tuple:
        """Thompson fragment (entry, exit) of an AST node."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edge[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for br in node[1]:
                x, y = self.build(br)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if hi is None:  # star of one more copy
            x, y = self.build(sub)
            out = self.new()
            self.eps[b] += [x, out]
            self.eps[y] += [x, out]
            return a, out
        out = self.new()
        for _ in range(hi - lo):  # each optional copy may skip to the exit
            x, y = self.build(sub)
            self.eps[b] += [x, out]
            b = y
        self.eps[b].append(out)
        return a, out

    def closure(self, states) -> frozenset:
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


class Dfa:
    """A compiled pattern (module docstring).  ``cls`` uint8 [256], ``trans`` uint16 [S * C], ``accept`` uint8 [S]."""

    def __init__(self, pattern: str, cls: np.ndarray, trans: np.ndarray, accept: np.ndarray, start: int = 0):
        self.pattern = pattern
        self.cls, self.trans, self.accept, self.start = cls, trans, accept, int(start)
        self.n_states = int(accept.shape[0])
        self.n_classes = int(trans.shape[0]) // max(1, self.n_states)
        self._cls = cls.tolist()
        self._trans = trans.tolist()

    def walk(self, state: int, data: bytes) -> int:
        """The state after reading ``data`` from ``state``: the host twin of the device walk."""
        C, tr, cl = self.n_classes, self._trans, self._cls
        for byte in bytes(data):
            if state == DEAD:
                return DEAD
            state = tr[state * C + cl[byte]]
        return state

    def accepts(self, state: int) -> bool:
        return state != DEAD and bool(self.accept[state])

    def fullmatch(self, data: bytes) -> bool:
        return self.accepts(self.walk(self.start, data))


def _byte_classes(masks) -> tuple:
    """Partition the 256 bytes by which edge sets they belong to: (cls list[256], C, one representative per class)."""
    sig_to_cls, cls, reps = {}, [0] * 256, []
    masks = sorted(set(masks))
    for byte in range(256):
        sig = tuple((m >> byte) & 1 for m in masks)
        k = sig_to_cls.get(sig)
        if k is None:
            k = sig_to_cls[sig] = len(reps)
            reps.append(byte)
        cls[byte] = k
    return cls, len(reps), reps


def _minimise(trans: list, accept: list, C: int) -> tuple:
    """Hopcroft partition refinement of a complete DFA whose last state is the sink.  Returns block ids per state."""
    n = len(accept)
    inv = [[[] for _ in range(n)] for _ in range(C)]
    for s in range(n):
        row = trans[s]
        for c in range(C):
            inv[c][row[c]].append(s)
    acc = {s for s in range(n) if accept[s]}
    blocks = [b for b in (acc, set(range(n)) - acc) if b]
    block_of = [0] * n
    for i, b in enumerate(blocks):
        for s in b:
            block_of[s] = i
    work = set(range(len(blocks)))
    while work:
        a = list(blocks[work.pop()])
        for c in range(C):
            hit: dict = {}
            ic = inv[c]
            for t in a:
                for s in ic[t]:
                    hit.setdefault(block_of[s], set()).add(s)
            for bi, x in hit.items():
                y = blocks[bi]
                if len(x) == len(y):
                    continue
                rest = y - x
                small, large = (x, rest) if len(x) <= len(rest) else (rest, x)
                blocks[bi] = large
                blocks.append(small)
                ni = len(blocks) - 1
                for s in small:
                    block_of[s] = ni
                work.add(ni)  # (bi in work: both halves are then in it; otherwise the smaller half suffices)
    return block_of


def _compile(pattern: str) -> Dfa:
    ast = _Parser(pattern).parse()
    nfa = _Nfa()
    entry, final = nfa.build(ast)
    cls, C, reps = _byte_classes([e[0] for e in nfa.edge if e is not None])
    # subset construction over the byte classes
    start = nfa.closure([entry])
    index = {start: 0}
    order = [start]
    rows: list = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        row = []
        for rep in reps:
            nxt = [nfa.edge[s][1] for s in cur if nfa.edge[s] is not None and (nfa.edge[s][0] >> rep) & 1]
            if not nxt:
                row.append(-1)
                continue
            t = nfa.closure(nxt)
            k = index.get(t)
            if k is None:
                if len(order) >= _MAX_RAW_DFA:
                    raise ValueError(f"pattern too large: more than {_MAX_RAW_DFA} DFA states before minimisation "
                                     f"(pattern {pattern!r})")
                k = index[t] = len(order)
                order.append(t)
            row.append(k)
        rows.append(row)
    n = len(order)
    accept = [final in st for st in order]
    # states that reach an accepting state (reverse reachability); the others become the sink
    back = [[] for _ in range(n)]
    for s, row in enumerate(rows):
        for t in set(row):
            if t >= 0:
                back[t].append(s)
    live = {s for s in range(n) if accept[s]}
    stack = list(live)
    while stack:
        for s in back[stack.pop()]:
            if s not in live:
                live.add(s)
                stack.append(s)
    if 0 not in live:
        raise ValueError(f"pattern matches nothing: {pattern!r}")
    sink = n
    full = [[(t if (t >= 0 and t in live) else sink) for t in row] if s in live else [sink] * C
            for s, row in enumerate(rows)] + [[sink] * C]
    block_of = _minimise(full, accept + [False], C)
    # renumber the blocks breadth first from the start state; the sink's block is DEAD
    dead_block = block_of[sink]
    rep_state: dict = {}
    for s in range(n + 1):
        rep_state.setdefault(block_of[s], s)
    new_id = {block_of[0]: 0}
    queue = [block_of[0]]
    out_rows, out_acc = [], []
    qi = 0
    while qi < len(queue):
        blk = queue[qi]
        qi += 1
        s = rep_state[blk]
        row = []
        for c in range(C):
            tb = block_of[full[s][c]]
            if tb == dead_block:
                row.append(DEAD)
                continue
            if tb not in new_id:
                new_id[tb] = len(queue)
                queue.append(tb)
            row.append(new_id[tb])
        out_rows.append(row)
        out_acc.append(1 if accept[s] else 0)
    S = len(out_rows)
    if S * C > MAX_TABLE or S >= DEAD:
        raise ValueError(f"pattern too large: {S} states x {C} byte classes = {S * C} table entries, the limit is "
                         f"{MAX_TABLE} (pattern {pattern!r})")
    return Dfa(pattern, np.asarray(cls, dtype=np.uint8), np.asarray(out_rows, dtype=np.uint16).reshape(-1),
               np.asarray(out_acc, dtype=np.uint8), 0)


@functools.lru_cache(maxsize=32)
def compile_regex(pattern: str) -> Dfa:
    """Compile ``pattern`` (full match over UTF-8 bytes) to a minimal byte DFA; cached by pattern string.  Raises
    ValueError for unsupported syntax and for a pattern whose table exceeds ``S * C <= 32768``."""
    if not isinstance(pattern, str):
        raise GuidedRequestError("regex must be a string")
    try:
        return _compile(pattern)
    except GuidedRequestError:
        raise
    except ValueError as e:
        raise GuidedRequestError(str(e)) from None
