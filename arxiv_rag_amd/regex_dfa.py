"""Regular expressions for Chroma's `$regex` / `$not_regex` document filters, compiled on the host to the byte-level DFA tables that
`arx_text_regex` walks over the chunk texts in HBM (include/arx.h, csrc/textscan.hip).  Pure Python + numpy, no GPU.

    dfa = compile_regex(r"\\d{4}\\.\\d{4,5}")               # ValueError names what it refuses, before anything is launched
    match_host(dfa, "arXiv:2101.00001".encode())          # True: the table interpreter, the definition the kernel is tested against
    tables, table_off = pack_tables([dfa])                # the flat uint8 / int32 arrays of one launch (1..8 regexes)

The test is unanchored "does the row contain a match" (`is_match` of the Rust `regex` crate that Chroma uses, `bool(re.search(...))` in
Python).  Accepted is the subset on which that crate and Python's `re` agree: literals (any Unicode character, as its UTF-8 bytes), the
escapes \\\\ \\. \\* \\+ \\? \\( \\) \\[ \\] \\{ \\} \\| \\^ \\$ \\- \\/ \\n \\t \\r and \\xHH (HH <= 7F), `.` (one whole code point except \\n), classes
`[abc]` `[a-z]` `[^...]` over code-point ranges, \\d \\w \\s \\D \\W \\S inside and outside classes, groups `( )` `(?: )`, alternation,
the quantifiers `* + ? {m} {m,} {m,n}` (their lazy forms mean the same for a yes/no answer), `^` / `$` as the start / end of the row's
text, and one leading flag group out of `(?i)` `(?s)` `(?is)` `(?si)` (`(?s)`: `.` matches \\n too).  A pattern that matches the
empty string matches every row, empty rows included.

Two deviations from the Rust crate: \\d \\w \\s are ASCII ([0-9], [A-Za-z0-9_], [ \\t\\n\\r\\f\\v]; their negations match any other whole
code point), and `(?i)` folds the ASCII letters only.

Refused (ValueError naming the construct and the pattern): the empty pattern, more than 256 bytes as UTF-8, backreferences,
look-around, \\b \\B \\A \\z \\Z, \\p{...}, [[:alpha:]]-style classes, named groups, other flags or flags elsewhere, \\xHH above 7F, a
counted repetition above 255, unbalanced or dangling syntax, and whatever the two engines read differently (a bare `{`, a doubled
quantifier, `[` or `&&` `--` `~~` inside a class).  Limits: at most 256 states after minimisation, at most 256 byte classes, and the
subset construction is abandoned past 4096 raw states; there is no host path for a pattern beyond them.

Pipeline: parse -> Thompson NFA over BYTES (a code-point range becomes the well-formed UTF-8 range automaton of 1 to 4 byte
sequences, so a multi-byte character is one step of the regex) with an any-byte self-loop on the start for the unanchored search
(`^` is an edge only the closure of the start follows, so a branch that begins with `^` does not see the loop) -> subset construction
over byte equivalence classes -> minimisation.  A state's flags: MATCHED (absorbing: the scan can stop), ACCEPT_AT_END (the row
matches if it ends here: `$`), DEAD (no accepting state can be reached: the scan can stop).

Behaviour is defined on well-formed UTF-8.  A row that holds a lone surrogate (`where_document.encode_text` uses `surrogatepass`) is
scanned as its bytes, and `.` or a negated class does not match its ill-formed sequence.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_PATTERN_BYTES = 256
MAX_STATES = 256
MAX_CLASSES = 256
MAX_RAW_STATES = 4096
MAX_REPEAT = 255
MAX_NFA_STATES = 50000
MAX_TABLES = 8
MATCHED, ACCEPT_AT_END, DEAD = 1, 2, 4
HEADER_BYTES = 4                                              # uint16 n_states, uint16 n_classes, little-endian

_META = "\\.*+?()[]{}|^$-/"
_DIGIT = [(0x30, 0x39)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_SPACE = [(0x09, 0x0D), (0x20, 0x20)]
_MAX_CP = 0x10FFFF


@dataclass(frozen=True, eq=False)
class RegexDFA:
    """`trans[s, class_of[b]]` is the state after byte `b` in state `s`; the start state is 0."""
    pattern: str
    n_states: int
    n_classes: int
    class_of: np.ndarray                                      # uint8 [256]
    flags: np.ndarray                                         # uint8 [n_states]: MATCHED | ACCEPT_AT_END | DEAD
    trans: np.ndarray                                         # uint8 [n_states, n_classes]


def _show(pattern: str) -> str:
    return repr(pattern if len(pattern) <= 48 else pattern[:45] + "...")


def _normalise(ranges) -> List[Tuple[int, int]]:
    out: List[Tuple[int, int]] = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def _negate(ranges) -> List[Tuple[int, int]]:
    out, at = [], 0
    for lo, hi in _normalise(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= _MAX_CP:
        out.append((at, _MAX_CP))
    return out


def _fold_ascii(ranges) -> List[Tuple[int, int]]:
    out = list(ranges)
    for lo, hi in ranges:
        a, b = max(lo, 0x41), min(hi, 0x5A)
        if a <= b:
            out.append((a + 32, b + 32))
        a, b = max(lo, 0x61), min(hi, 0x7A)
        if a <= b:
            out.append((a - 32, b - 32))
    return _normalise(out)


class _Parser:
    """Recursive descent -> ("set", ranges) | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None) | ("bol",) | ("eol",)."""

    def __init__(self, pattern: str):
        self.p, self.i, self.fold, self.dotall = pattern, 0, False, False

    def fail(self, what: str):
        raise ValueError(f"regex: {what} in {_show(self.p)}")

    def peek(self) -> Optional[str]:
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        for flags in ("(?i)", "(?s)", "(?is)", "(?si)"):
            if self.p.startswith(flags):
                self.i, self.fold, self.dotall = len(flags), "i" in flags, "s" in flags
                break
        node = self.alternation()
        if self.peek() == ")":
            self.fail("unbalanced ')'")
        assert self.i == len(self.p)
        return node

    def alternation(self):
        branches = [self.concatenation()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.concatenation())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def concatenation(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.repetition())
        return items[0] if len(items) == 1 else ("cat", items)

    def repetition(self):
        c = self.peek()
        if c in "*+?":
            self.fail(f"dangling quantifier '{c}' (nothing to repeat)")
        if c == "{":
            self.fail("dangling '{' (nothing to repeat; escape a literal brace)")
        atom = self.atom()
        c = self.peek()
        if c is None or c not in "*+?{":
            return atom
        if atom[0] in ("bol", "eol"):
            self.fail(f"quantifier '{c}' on an anchor")
        if c == "{":
            m, n = self.counted()
        else:
            self.i += 1
            m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
        if self.peek() == "?":                                # lazy: the same yes/no answer
            self.i += 1
        if self.peek() is not None and self.peek() in "*+?{":
            self.fail(f"doubled quantifier '{self.peek()}' (the engines read it differently)")
        return ("rep", atom, m, n)

    def counted(self) -> Tuple[int, Optional[int]]:
        end = self.p.find("}", self.i)
        body = self.p[self.i + 1:end] if end >= 0 else ""
        lo, comma, hi = body.partition(",")
        ok = end >= 0 and lo.isascii() and lo.isdigit() and (not comma or hi == "" or (hi.isascii() and hi.isdigit()))
        if not ok:
            self.fail("bare or malformed '{' (a counted repetition is {m}, {m,} or {m,n}; escape a literal brace)")
        m = int(lo)
        n = m if not comma else (None if hi == "" else int(hi))
        if m > MAX_REPEAT or (n is not None and n > MAX_REPEAT):
            self.fail(f"counted repetition {{{body}}} above {MAX_REPEAT}")
        if n is not None and n < m:
            self.fail(f"counted repetition {{{body}}} with max below min")
        self.i = end + 1
        return m, n

    def single(self, cp: int):
        return ("set", _fold_ascii([(cp, cp)]) if self.fold else [(cp, cp)])

    def atom(self):
        c = self.p[self.i]
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                rest = self.p[self.i:self.i + 3]
                if rest.startswith("?:"):
                    self.i += 2
                elif rest.startswith("?P") or (rest.startswith("?<") and rest[2:3] not in ("=", "!")):
                    self.fail("named group")
                elif rest[1:2] in ("=", "!") or rest.startswith("?<"):
                    self.fail("look-around")
                else:
                    self.fail("flag group (only one leading (?i), (?s), (?is) or (?si) is supported)")
            node = self.alternation()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            return ("set", [(0, _MAX_CP)] if self.dotall else [(0, 9), (11, _MAX_CP)])
        if c == "^":
            return ("bol",)
        if c == "$":
            return ("eol",)
        if c == "\\":
            kind, val = self.escape(in_class=False)
            return ("set", val) if kind == "set" else self.single(val)
        if c in "]}":
            self.fail(f"unbalanced '{c}' (escape a literal one)")
        if 0xD800 <= ord(c) <= 0xDFFF:
            self.fail("lone surrogate")
        return self.single(ord(c))

    def escape(self, in_class: bool):
        """After a backslash -> ("set", ranges) or ("cp", code point)."""
        c = self.peek()
        if c is None:
            self.fail("dangling backslash")
        self.i += 1
        if c in _META:
            return "cp", ord(c)
        if c in "ntr":
            return "cp", {"n": 10, "t": 9, "r": 13}[c]
        if c in "dwsDWS":
            base = {"d": _DIGIT, "w": _WORD, "s": _SPACE}[c.lower()]
            return "set", (list(base) if c.islower() else _negate(base))
        if c == "x":
            hh = self.p[self.i:self.i + 2]
            if len(hh) != 2 or any(h not in "0123456789abcdefABCDEF" for h in hh):
                self.fail("malformed \\x escape (two hex digits)")
            if int(hh, 16) > 0x7F:
                self.fail(f"\\x{hh} above 7F (a byte that is no character)")
            self.i += 2
            return "cp", int(hh, 16)
        if c.isdigit():
            self.fail(f"backreference or octal escape \\{c}")
        if c in "bBAzZ":
            self.fail(f"\\{c} (word boundaries and \\A \\z \\Z are not supported; ^ and $ are the row's start and end)")
        if c in "pP":
            self.fail(f"\\{c}{{...}} Unicode class")
        self.fail(f"unknown escape \\{c}")

    def char_class(self):
        negated = self.peek() == "^"
        if negated:
            self.i += 1
        ranges: List[Tuple[int, int]] = []
        first = True
        while True:
            c = self.peek()
            if c is None:
                self.fail("unbalanced '['")
            if c == "]":
                if first:
                    self.fail("empty class '[]' (escape a literal ']')")
                self.i += 1
                break
            first = False
            if c == "[":
                self.fail("[[:alpha:]]-style class" if self.p[self.i + 1:self.i + 2] == ":" else "'[' inside a class (escape it)")
            if c in "&-~" and self.p[self.i + 1:self.i + 2] == c:
                self.fail(f"'{c}{c}' inside a class (a set operation in one engine, two literals in the other)")
            kind, lo = self.class_item()
            if kind == "set":
                ranges.extend(lo)
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                kind2, hi = self.class_item()
                if kind2 == "set":
                    self.fail("class escape as the end of a range")
                if hi < lo:
                    self.fail("reversed range in a class")
                ranges.append((lo, hi))
            else:
                ranges.append((lo, lo))
        ranges = _normalise(ranges)
        if self.fold:
            ranges = _fold_ascii(ranges)
        return ("set", _negate(ranges) if negated else ranges)

    def class_item(self):
        c = self.p[self.i]
        self.i += 1
        if c == "\\":
            return self.escape(in_class=True)
        if 0xD800 <= ord(c) <= 0xDFFF:
            self.fail("lone surrogate")
        return "cp", ord(c)


def _utf8(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def utf8_sequences(lo: int, hi: int) -> List[List[Tuple[int, int]]]:
    """The code points [lo, hi] without the surrogates, as sequences of byte ranges: a byte string is the UTF-8 of one of them exactly
    when it matches one sequence byte for byte."""
    out, stack = [], [(lo, hi)]
    while stack:
        lo, hi = stack.pop()
        if lo > hi:
            continue
        if lo <= 0xDFFF and hi >= 0xD800:
            stack += [(lo, 0xD7FF), (0xE000, hi)]
            continue
        cut = next((m for m in (0x7F, 0x7FF, 0xFFFF) if lo <= m < hi), None)
        if cut is not None:
            stack += [(lo, cut), (cut + 1, hi)]
            continue
        if hi <= 0x7F:
            out.append([(lo, hi)])
            continue
        split = False
        for i in range(1, len(_utf8(hi))):
            m = (1 << (6 * i)) - 1
            if (lo & ~m) != (hi & ~m):
                if lo & m:
                    stack += [(lo, lo | m), ((lo | m) + 1, hi)]
                    split = True
                elif (hi & m) != m:
                    stack += [(lo, (hi & ~m) - 1), (hi & ~m, hi)]
                    split = True
                if split:
                    break
        if not split:
            out.append(list(zip(_utf8(lo), _utf8(hi))))
    return out


class _NFA:
    def __init__(self, pattern: str):
        self.pattern = pattern
        self.eps: List[List[int]] = []
        self.eps_bol: List[List[int]] = []                    # followed only in the closure of the start (`^`)
        self.eps_eol: List[List[int]] = []                    # followed only when the row ends (`$`)
        self.edges: List[List[Tuple[int, int, int]]] = []     # (byte lo, byte hi, target)

    def new(self) -> int:
        if len(self.eps) >= MAX_NFA_STATES:
            raise ValueError(f"regex: more than {MAX_NFA_STATES} NFA states (the counted repetitions multiply) in {_show(self.pattern)}")
        for lst in (self.eps, self.eps_bol, self.eps_eol, self.edges):
            lst.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        kind = node[0]
        a, b = self.new(), self.new()
        if kind == "set":
            for lo, hi in node[1]:
                for seq in utf8_sequences(lo, hi):
                    at = a
                    for j, (blo, bhi) in enumerate(seq):
                        to = b if j == len(seq) - 1 else self.new()
                        self.edges[at].append((blo, bhi, to))
                        at = to
        elif kind == "bol":
            self.eps_bol[a].append(b)
        elif kind == "eol":
            self.eps_eol[a].append(b)
        elif kind == "cat":
            at = a
            for child in node[1]:
                s, e = self.build(child)
                self.eps[at].append(s)
                at = e
            self.eps[at].append(b)
        elif kind == "alt":
            for child in node[1]:
                s, e = self.build(child)
                self.eps[a].append(s)
                self.eps[e].append(b)
        else:
            _, child, m, n = node
            at = a
            for _ in range(m):
                s, e = self.build(child)
                self.eps[at].append(s)
                at = e
            if n is None:
                s, e = self.build(child)
                self.eps[at] += [s, b]
                self.eps[e] += [s, b]
            else:
                for _ in range(n - m):                        # (x(x(x)?)?)?: every optional copy may also leave
                    s, e = self.build(child)
                    self.eps[at] += [s, b]
                    at = e
                self.eps[at].append(b)
        return a, b

    def closure(self, states, bol: bool, eol: bool) -> frozenset:
        seen, stack = set(states), list(states)
        while stack:
            s = stack.pop()
            for t in self.eps[s] + (self.eps_bol[s] if bol else []) + (self.eps_eol[s] if eol else []):
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _subset_construction(nfa: _NFA, start: int, accept: int):
    """-> (trans int32 [n, C0], flags uint8 [n], class_of uint8-able [256]) over the byte classes the NFA's edges induce; state 0 is the start."""
    cuts = {0, 256}
    for edges in nfa.edges:
        for lo, hi, _ in edges:
            cuts.add(lo)
            cuts.add(hi + 1)
    bounds = sorted(cuts)
    class_of = np.zeros(256, dtype=np.int32)
    for c in range(len(bounds) - 1):
        class_of[bounds[c]:bounds[c + 1]] = c
    n_cls = len(bounds) - 1
    plain: Dict[int, frozenset] = {}

    def closed(s: int) -> frozenset:
        if s not in plain:
            plain[s] = nfa.closure([s], False, False)
        return plain[s]

    MATCH = -1                                                # resolved to a state of its own at the end
    rows: List[List[int]] = []
    flags: List[int] = []
    ids: Dict[frozenset, int] = {}
    moves: Dict[frozenset, int] = {}
    todo: List[Tuple[int, frozenset]] = []

    def add(subset: frozenset, at_end: frozenset) -> int:
        rows.append([0] * n_cls)
        flags.append(ACCEPT_AT_END if accept in at_end else 0)
        todo.append((len(rows) - 1, subset))
        if len(rows) > MAX_RAW_STATES:
            raise ValueError(f"regex: more than {MAX_RAW_STATES} DFA states before minimisation (at most {MAX_STATES} are scanned) "
                             f"in {_show(nfa.pattern)}")
        return len(rows) - 1

    first = nfa.closure([start], True, False)
    if accept in first:                                       # matches the empty string: every row
        return np.zeros((1, 1), dtype=np.int32), np.array([MATCHED | ACCEPT_AT_END], dtype=np.uint8), np.zeros(256, dtype=np.int32)
    add(first, nfa.closure([start], True, True))              # (the start is a state of its own: only its closure follows `^`)
    while todo:
        sid, subset = todo.pop()
        per_class: List[set] = [set() for _ in range(n_cls)]
        for s in subset:
            for lo, hi, t in nfa.edges[s]:
                for c in range(class_of[lo], class_of[hi] + 1):
                    per_class[c].add(t)
        for c, targets in enumerate(per_class):
            key = frozenset(targets)
            if key not in moves:
                nxt = frozenset().union(*(closed(t) for t in key)) if key else frozenset()
                if accept in nxt:
                    moves[key] = MATCH
                else:
                    if nxt not in ids:
                        ids[nxt] = add(nxt, nfa.closure(nxt, False, True))
                    moves[key] = ids[nxt]
            rows[sid][c] = moves[key]
    trans = np.array(rows, dtype=np.int32)
    if (trans == MATCH).any():
        trans[trans == MATCH] = len(rows)
        trans = np.vstack([trans, np.full((1, n_cls), len(rows), dtype=np.int32)])
        flags.append(MATCHED | ACCEPT_AT_END)
    return trans, np.array(flags, dtype=np.uint8), class_of


def _minimise(trans: np.ndarray, flags: np.ndarray):
    """Moore's partition refinement; -> (trans, flags) with the start state still 0 and DEAD set where no accepting state is reachable."""
    n = trans.shape[0]
    block = np.unique(flags, return_inverse=True)[1].reshape(-1)
    while True:
        sig = np.concatenate([block[:, None], block[trans]], axis=1)
        new = np.unique(sig, axis=0, return_inverse=True)[1].reshape(-1)
        if new.max() == block.max():
            break
        block = new
    order: List[int] = []                                     # blocks in order of first appearance from the start: state 0 stays the start
    seen = set()
    for s in range(n):
        if block[s] not in seen:
            seen.add(block[s])
            order.append(s)
    remap = {int(block[s]): i for i, s in enumerate(order)}
    new_id = np.array([remap[int(b)] for b in block], dtype=np.int32)
    mt = new_id[trans[order]]
    mf = flags[order].copy()
    live = (mf & (MATCHED | ACCEPT_AT_END)) != 0              # backwards reachability of an accepting state
    while True:
        grown = live | live[mt].any(axis=1)
        if (grown == live).all():
            break
        live = grown
    mf[~live] |= DEAD
    return mt, mf


def compile_regex(pattern: str) -> RegexDFA:
    """Compile `pattern` (the dialect of the module docstring: \\d \\w \\s are ASCII and (?i) folds ASCII letters only, unlike the Rust crate)
    to a minimal byte-level DFA of at most 256 states over at most 256 byte classes.  ValueError names what is refused or which limit
    the pattern exceeds, with its count; there is no host path for such a pattern."""
    if not isinstance(pattern, str):
        raise ValueError(f"regex: a pattern must be a string, got {pattern!r}")
    if not pattern:
        raise ValueError("regex: the empty pattern is refused (it would match every row)")
    nbytes = len(pattern.encode("utf-8", "surrogatepass"))
    if nbytes > MAX_PATTERN_BYTES:
        raise ValueError(f"regex: a pattern of {nbytes} bytes as UTF-8, at most {MAX_PATTERN_BYTES} are compiled: {_show(pattern)}")
    ast = _Parser(pattern).parse()
    nfa = _NFA(pattern)
    start, accept = nfa.new(), nfa.new()
    s, e = nfa.build(ast)
    nfa.edges[start].append((0, 255, start))                  # the unanchored search
    nfa.eps[start].append(s)
    nfa.eps[e].append(accept)
    trans, flags, class_of = _subset_construction(nfa, start, accept)
    trans, flags = _minimise(trans, flags)
    cols, col_of = np.unique(trans, axis=1, return_inverse=True)      # bytes no state tells apart share a class
    class_of = col_of.reshape(-1)[class_of]
    n_states, n_classes = cols.shape
    if n_states > MAX_STATES:
        raise ValueError(f"regex: {n_states} DFA states after minimisation, at most {MAX_STATES} are scanned: {_show(pattern)}")
    if n_classes > MAX_CLASSES:
        raise ValueError(f"regex: {n_classes} byte classes, at most {MAX_CLASSES} are scanned: {_show(pattern)}")
    return RegexDFA(pattern, int(n_states), int(n_classes), class_of.astype(np.uint8), flags.astype(np.uint8),
                    np.ascontiguousarray(cols, dtype=np.uint8))


def match_host(dfa: RegexDFA, data: bytes) -> bool:
    """Does `data` contain a match?  The table interpreter: the definition `arx_text_regex` is tested against."""
    state, flags, trans, class_of = 0, dfa.flags, dfa.trans, dfa.class_of
    for b in data:
        if flags[state] & (MATCHED | DEAD):
            break
        state = trans[state, class_of[b]]
    return bool(flags[state] & (MATCHED | ACCEPT_AT_END))


def pack_tables(dfas: Sequence[RegexDFA]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (uint8 [sum of table bytes], int32 [len(dfas) + 1]) for `arx_text_regex`.  One table: uint16 n_states, uint16 n_classes
    (little-endian), class_of[256], flags[n_states], trans[n_states][n_classes]."""
    if not (1 <= len(dfas) <= MAX_TABLES):
        raise ValueError(f"regex: {len(dfas)} regexes in one scan, 1..{MAX_TABLES} are supported")
    parts, off = [], [0]
    for d in dfas:
        assert 1 <= d.n_states <= MAX_STATES and 1 <= d.n_classes <= MAX_CLASSES
        assert d.class_of.shape == (256,) and d.flags.shape == (d.n_states,) and d.trans.shape == (d.n_states, d.n_classes)
        assert int(d.trans.max()) < d.n_states and int(d.class_of.max()) < d.n_classes
        stop = np.nonzero(d.flags & (MATCHED | DEAD))[0]      # absorbing: the kernel looks at the flags once per 16 bytes, not per byte
        assert (d.trans[stop] == stop[:, None]).all()
        head = np.array([d.n_states, d.n_classes], dtype="<u2").view(np.uint8)
        parts += [head, d.class_of.astype(np.uint8), d.flags.astype(np.uint8), d.trans.astype(np.uint8).reshape(-1)]
        off.append(off[-1] + HEADER_BYTES + 256 + d.n_states + d.n_states * d.n_classes)
    return np.concatenate(parts), np.array(off, dtype=np.int32)
