"""Chroma `where_document` filters (`$contains` / `$not_contains` on the chunk TEXT), scanned on the GPU and folded into the row
bitmap the filtered search takes (`arx_text_contains` -> `arx_topk_search_filtered`, include/arx.h).

    tree = compile_where_document({"$and": [{"$contains": "Lipschitz"}, {"$not_contains": "lemma"}]})
    store = DocumentStore(texts, device="cuda:0")            # the shard's texts as one UTF-8 blob in HBM
    words, n_allowed = store.allow(tree)                     # int64 [ceil(n / 64)] on the device, bit r & 63 of word r >> 6 = row r

Operators: `{"$contains": s}` (the text contains `s` as a contiguous substring, case-sensitive: Python's `s in text`), `{"$not_contains": s}`
(its negation), `{"$and": [...]}` / `{"$or": [...]}` with nesting; exactly one operator per dict, `s` a non-empty str.  On the device both
sides are UTF-8 bytes (`errors="surrogatepass"`, so a lone surrogate neither raises nor changes the answer); a byte substring of well-formed
UTF-8 is a code-point substring because UTF-8 is self-synchronising.  Limits (ValueError before anything is launched; there is no host
path): a pattern of more than 256 bytes once encoded, more than 32 distinct patterns in one filter.

Opt-in (`compile_where_document(f, regex=True)`; without it they stay refused as unknown operators): `{"$regex": p}` (the text contains
a match of `p`: unanchored, `bool(re.search(...))`) and `{"$not_regex": p}` (its negation).  The dialect, its two deviations from the
Rust `regex` crate (ASCII \\d \\w \\s, ASCII-only `(?i)`) and its limits are `regex_dfa.compile_regex`'s; a pattern it refuses is a
ValueError here, before anything is launched.  At most 8 distinct regexes in one filter, counted apart from the 32 substrings; one
`arx_text_regex` launch scans them all.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_PATTERN_BYTES = 256
MAX_PATTERNS = 32
MAX_REGEXES = 8
_LEAF = ("$contains", "$not_contains")
_REGEX_LEAF = ("$regex", "$not_regex")
_DFA_CACHE_SIZE = 256
_dfa_cache: Dict[str, object] = {}
_NODE = ("$and", "$or")


def encode_text(s: str) -> bytes:
    return s.encode("utf-8", "surrogatepass")


def compiled_regex(pattern: str):
    """`regex_dfa.compile_regex(pattern)`, kept per pattern string in a bounded dict (the oldest entry leaves first)."""
    dfa = _dfa_cache.get(pattern)
    if dfa is None:
        from .regex_dfa import compile_regex
        dfa = compile_regex(pattern)
        if len(_dfa_cache) >= _DFA_CACHE_SIZE:
            del _dfa_cache[next(iter(_dfa_cache))]
        _dfa_cache[pattern] = dfa
    return dfa


def _compile(f, regex: bool = False) -> Tuple:
    if not isinstance(f, dict) or not f:
        raise ValueError(f"where_document: expected a non-empty dict, got {f!r}")
    if len(f) != 1:
        raise ValueError(f"where_document: exactly one operator per dict, got {sorted(map(str, f))!r}")
    (op, val), = f.items()
    if op in _LEAF:
        if not isinstance(val, str):
            raise ValueError(f"where_document: operand of {op} must be a string, got {val!r}")
        if not val:
            raise ValueError(f"where_document: operand of {op} must be a non-empty string")
        nbytes = len(encode_text(val))
        if nbytes > MAX_PATTERN_BYTES:
            raise ValueError(f"where_document: operand of {op} is {nbytes} bytes as UTF-8, at most {MAX_PATTERN_BYTES} are scanned: {val[:24]!r}...")
        return (op[1:], val)
    if regex and op in _REGEX_LEAF:
        if not isinstance(val, str):
            raise ValueError(f"where_document: operand of {op} must be a string, got {val!r}")
        try:
            compiled_regex(val)                              # compiled at once: a bad pattern fails before any GPU work
        except ValueError as e:
            raise ValueError(f"where_document: operand of {op}: {e}") from None
        return (op[1:], val)
    if op in _NODE:
        if not isinstance(val, (list, tuple)) or not val:
            raise ValueError(f"where_document: {op} needs a non-empty list of filters, got {val!r}")
        return (op[1:], tuple(_compile(v, regex) for v in val))
    raise ValueError(f"where_document: unknown operator {op!r}")


def _leaves_of(tree: Tuple, kinds: Tuple[str, str]) -> List[str]:
    out: Dict[str, None] = {}

    def walk(node):
        if node[0] in ("and", "or"):
            for c in node[1]:
                walk(c)
        elif node[0] in kinds:
            out.setdefault(node[1])
    walk(tree)
    return list(out)


def patterns_of(tree: Tuple) -> List[str]:
    """The distinct strings of the tree's `contains` / `not_contains` leaves, in first-seen order."""
    return _leaves_of(tree, ("contains", "not_contains"))


def regexes_of(tree: Tuple) -> List[str]:
    """The distinct patterns of the tree's `regex` / `not_regex` leaves, in first-seen order."""
    return _leaves_of(tree, ("regex", "not_regex"))


def compile_where_document(f: Dict, regex: bool = False) -> Tuple:
    """Validate a Chroma `where_document` filter and return its tree: ("and" | "or", children), ("contains" | "not_contains", str).
    ValueError names the offending part.
    `regex=True` also accepts `$regex` / `$not_regex` leaves, as ("regex" | "not_regex", pattern), each pattern compiled here
    (`regex_dfa.compile_regex`: its dialect, deviations and limits); without it they are unknown operators, as ever."""
    tree = _compile(f, regex)
    n = len(patterns_of(tree))
    if n > MAX_PATTERNS:
        raise ValueError(f"where_document: {n} distinct patterns in one filter, at most {MAX_PATTERNS} are scanned per call")
    n = len(regexes_of(tree))
    if n > MAX_REGEXES:
        raise ValueError(f"where_document: {n} distinct regexes in one filter, at most {MAX_REGEXES} are scanned per call")
    return tree


def evaluate_host(tree: Tuple, texts: Sequence[str]) -> np.ndarray:
    """bool [n]: the pure-Python definition (`s in text` on the strs; `regex_dfa.match_host` on the text's bytes for a regex leaf).  For
    tests and documentation; the product path never calls it."""
    kind = tree[0]
    if kind in ("and", "or"):
        out = evaluate_host(tree[1][0], texts)
        for child in tree[1][1:]:
            m = evaluate_host(child, texts)
            out = (out & m) if kind == "and" else (out | m)
        return out
    s = tree[1]
    if kind in ("regex", "not_regex"):
        from .regex_dfa import match_host
        dfa = compiled_regex(s)
        hit = np.fromiter((match_host(dfa, encode_text(t)) for t in texts), dtype=bool, count=len(texts))
        return hit if kind == "regex" else ~hit
    hit = np.fromiter((s in t for t in texts), dtype=bool, count=len(texts))
    return hit if kind == "contains" else ~hit


def pack_documents(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (uint8 [B], int64 [n + 1]): the texts as UTF-8, concatenated without separators, and each row's start (row r is
    blob[off[r]:off[r + 1]]; off[0] == 0, off[n] == B)."""
    enc = [encode_text(t) for t in texts]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc)), out=off[1:])
    return np.frombuffer(b"".join(enc), dtype=np.uint8), off


def pack_patterns(patterns: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (uint8 [sum of lengths], int32 [P + 1]) for `arx_text_contains`; refuses what the kernel's contract excludes."""
    if not (1 <= len(patterns) <= MAX_PATTERNS):
        raise ValueError(f"where_document: {len(patterns)} patterns in one scan, 1..{MAX_PATTERNS} are supported")
    enc = []
    for s in patterns:
        if not isinstance(s, str) or not s:
            raise ValueError(f"where_document: a pattern must be a non-empty string, got {s!r}")
        e = encode_text(s)
        if len(e) > MAX_PATTERN_BYTES:
            raise ValueError(f"where_document: a pattern of {len(e)} bytes as UTF-8, at most {MAX_PATTERN_BYTES} are scanned: {s[:24]!r}...")
        enc.append(e)
    off = np.zeros(len(enc) + 1, dtype=np.int32)
    np.cumsum(np.fromiter((len(e) for e in enc), dtype=np.int32, count=len(enc)), out=off[1:])
    return np.frombuffer(b"".join(enc), dtype=np.uint8), off


class DocumentStore:
    """The texts of one shard as a UTF-8 blob in HBM, with the substring scan over it."""

    def __init__(self, texts: Sequence[str], device="cuda:0", slab_rows: int = 1 << 16, capacity_bytes: int = 0):
        """`capacity_bytes` (0 = nothing changes): the blob is allocated with room for that many bytes, so that `append` need not
        reallocate it until they are used up."""
        import torch
        from . import _lib
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.n_rows = n = len(texts)
        self.n_words = (n + 63) // 64
        off = np.zeros(n + 1, dtype=np.int64)
        pieces = []
        for s0 in range(0, n, slab_rows):                     # slabs: the host never holds a second copy of all the texts
            s1 = min(n, s0 + slab_rows)
            blob, o = pack_documents(texts[s0:s1])
            off[s0 + 1:s1 + 1] = off[s0] + o[1:]
            pieces.append(torch.from_numpy(blob.copy()).to(self.device))
        self.n_bytes = int(off[n])
        self.blob = torch.zeros(max(16, self.n_bytes, int(capacity_bytes)), dtype=torch.uint8, device=self.device)    # (a valid pointer for an all-empty shard too)
        at = 0
        for i in range(len(pieces)):
            p, pieces[i] = pieces[i], None
            self.blob[at:at + p.numel()] = p
            at += p.numel()
        self.row_off = torch.from_numpy(off).to(self.device)
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def append(self, texts: Sequence[str]) -> None:
        """More rows at the end.  The blob grows by reallocation (to at least twice its size) once its capacity is used up: nothing
        else holds it.  The scans read `row_off[n_rows]` bytes of it, whatever its size."""
        import torch
        if not len(texts):
            return
        blob, o = pack_documents(list(texts))
        need = self.n_bytes + int(o[-1])
        if need > self.blob.numel():
            grown = torch.zeros(max(need, 2 * self.blob.numel()), dtype=torch.uint8, device=self.device)
            grown[:self.n_bytes] = self.blob[:self.n_bytes]
            self.blob = grown
        if len(blob):
            self.blob[self.n_bytes:need] = torch.from_numpy(blob.copy()).to(self.device)
        more = torch.from_numpy(self.n_bytes + o[1:].astype(np.int64)).to(self.device)
        self.row_off = torch.cat([self.row_off, more])
        self.n_rows, self.n_bytes = self.n_rows + len(texts), need
        self.n_words = (self.n_rows + 63) // 64

    def compact(self, keep, word_rank, count: int) -> None:
        """Drop the rows whose bit of `keep` (device int64 / uint64 [ceil(n / 64)]) is clear, on the device (`arx_compact_text`).
        `word_rank`, `count`: the plan of `keep` (`arx_compact_plan`).  The blob keeps its capacity."""
        import torch
        from . import _lib
        assert keep.is_cuda and keep.is_contiguous() and keep.shape == (self.n_words,) and word_rank.shape == (self.n_words + 1,)
        new_blob = torch.zeros_like(self.blob)
        new_off = torch.empty(int(count) + 1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.arx_compact_text(self.blob.data_ptr(), self.row_off.data_ptr(), self.n_rows, keep.data_ptr(), word_rank.data_ptr(),
                                           new_blob.data_ptr(), new_off.data_ptr(), self._stream())
        _lib.check(rc, "arx_compact_text")
        self.blob, self.row_off = new_blob, new_off
        self.n_rows, self.n_bytes = int(count), int(new_off[-1].item())
        self.n_words = (self.n_rows + 63) // 64

    def contains(self, patterns: Sequence[str], out=None):
        """int64 [P, ceil(n / 64)] on the device: bit r & 63 of word [p, r >> 6] = `patterns[p] in texts[r]`; bits at or beyond n are 0.
        One `arx_text_contains` launch for all the patterns, on the current stream, no synchronisation."""
        import torch
        from . import _lib
        pb, po = pack_patterns(patterns)
        if out is None:
            out = torch.empty((len(patterns), self.n_words), dtype=torch.int64, device=self.device)
        assert out.shape == (len(patterns), self.n_words) and out.dtype == torch.int64 and out.is_contiguous() and out.device == self.blob.device
        if self.n_rows == 0:
            return out
        with torch.cuda.device(self.device):
            pbd, pod = torch.from_numpy(pb.copy()).to(self.device), torch.from_numpy(po).to(self.device)
            rc = self.lib.arx_text_contains(self.blob.data_ptr(), self.row_off.data_ptr(), self.n_rows, pbd.data_ptr(), pod.data_ptr(),
                                            len(patterns), out.data_ptr(), self._stream())
        _lib.check(rc, "arx_text_contains")
        return out

    def regex(self, patterns: Sequence[str], out=None, waves_per_block: int = 0):
        """int64 [P, ceil(n / 64)] on the device: bit r & 63 of word [p, r >> 6] = `texts[r]` contains a match of the regular expression
        `patterns[p]` (`regex_dfa.compile_regex`; 1..8 of them); bits at or beyond n are 0.  One `arx_text_regex` launch for all of
        them, on the current stream, no synchronisation.  `waves_per_block`: the launch shape (`arx_text_regex_tuned`), same bits."""
        import torch
        from . import _lib
        from .regex_dfa import pack_tables
        tb, to = pack_tables([compiled_regex(p) for p in patterns])
        if out is None:
            out = torch.empty((len(patterns), self.n_words), dtype=torch.int64, device=self.device)
        assert out.shape == (len(patterns), self.n_words) and out.dtype == torch.int64 and out.is_contiguous() and out.device == self.blob.device
        if self.n_rows == 0:
            return out
        with torch.cuda.device(self.device):
            tbd, tod = torch.from_numpy(tb).to(self.device), torch.from_numpy(to).to(self.device)
            rc = self.lib.arx_text_regex_tuned(self.blob.data_ptr(), self.row_off.data_ptr(), self.n_rows, tbd.data_ptr(), tod.data_ptr(),
                                               len(patterns), out.data_ptr(), waves_per_block, self._stream())
        _lib.check(rc, "arx_text_regex")
        return out

    def count(self, words) -> int:
        """Set bits of `words` (int64 [ceil(n / 64)], device) that name rows below n (`arx_bitmap_count`).  Waits for the result."""
        import torch
        from . import _lib
        assert words.is_cuda and words.dtype == torch.int64 and words.is_contiguous() and words.shape == (self.n_words,)
        if self.n_rows == 0:
            return 0
        with torch.cuda.device(self.device):
            _lib.check(self.lib.arx_bitmap_count(words.data_ptr(), self.n_rows, self._count.data_ptr(), self._stream()), "arx_bitmap_count")
        return int(self._count.item())

    def fold(self, tree: Tuple):
        """int64 [ceil(n / 64)] on the device: the tree folded over the pattern bitmaps with bitwise ops.  `$not_contains` is `~`, which also
        sets the last word's bits beyond n: the search ignores them and `count` does not count them.  One `arx_text_contains` launch for
        the tree's substrings and one `arx_text_regex` launch for its regexes (`$not_regex` is `~` likewise)."""
        pats, regs = patterns_of(tree), regexes_of(tree)
        row = {}
        if pats:
            bits = self.contains(pats)
            row.update((("contains", s), bits[i]) for i, s in enumerate(pats))
        if regs:
            bits = self.regex(regs)
            row.update((("regex", s), bits[i]) for i, s in enumerate(regs))

        def go(node):
            if node[0] in ("and", "or"):
                acc = go(node[1][0])
                for c in node[1][1:]:
                    acc = (acc & go(c)) if node[0] == "and" else (acc | go(c))
                return acc
            if node[0] in ("contains", "regex"):
                return row[node]
            return ~row[(node[0][4:], node[1])]
        return go(tree).contiguous()

    def allow(self, tree: Tuple):
        """-> (words int64 [ceil(n / 64)] on the device, n_allowed): what `ShardIndex.search(allow=..., n_allowed=...)` takes."""
        words = self.fold(tree)
        return words, self.count(words)
