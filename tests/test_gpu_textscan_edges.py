"""The text scans (`text_contains_kernel`, `text_regex_kernel`; csrc/textscan.hip) where their tile geometry and their guards for device
data can go wrong: blobs at every address mod 16 between guard bytes, needles at the edges of a tile and of its halo, rows that end
where the wave's previous row left bytes in LDS, the capacity of the pattern store, pattern lengths and regex tables outside the
contract of include/arx.h, and hand-made tables.  The cases are tests/textscan_cases.py's (tests/test_textscan_cases_host.py shows
on the CPU that each family fails for the fault it is there to catch).  Both entry points are called through the C ABI on a view
`buf[16 + shift:]` of a 16-byte aligned allocation; the output is prefilled with ones and lies between guard words.  Every
comparison is on bits: Python's `in` for the substring scan, `regex_dfa.match_host` / `evaluate_host` for the regex scan."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arxiv_rag_amd.regex_dfa import ACCEPT_AT_END, DEAD, MATCHED, RegexDFA, compile_regex, match_host, pack_tables
from arxiv_rag_amd.where import pack_bitmap
from arxiv_rag_amd.where_document import evaluate_host
from tests import textscan_cases as TC

pytestmark = pytest.mark.gpu

GUARD_WORDS, GUARD_WORD = 8, 0x5A5A5A5A5A5A5A5A
REGEX_WAVES = (0, 1, 16)


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def _pack(bits):
    """[pattern][row] bools -> uint64 [P, ceil(n / 64)]."""
    return np.stack([pack_bitmap(np.asarray(b, dtype=bool)) for b in bits])


class Blob:
    """Rows on the device at address = 16 * k + shift, between `before` and `after`."""

    def __init__(self, rows, shift, before=b"", after=b""):
        mem, at = TC.place(b"".join(rows), shift, before, after)
        self.buf = torch.from_numpy(np.frombuffer(mem, dtype=np.uint8).copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0, "the allocation is expected to be 16-byte aligned"
        self.view = self.buf[at:]
        assert self.view.data_ptr() % 16 == shift
        self.off = torch.from_numpy(np.asarray(TC.offsets(rows), dtype=np.int64)).cuda()
        self.n_rows, self.words = len(rows), (len(rows) + 63) // 64


def _scan(hip, blob, n_out, call, what):
    """Run `call(out_ptr, stream)` on an output of n_out x words int64 prefilled with ones between guard words -> uint64 [n_out, words]."""
    size = n_out * blob.words
    buf = torch.full((2 * GUARD_WORDS + size,), GUARD_WORD, dtype=torch.int64, device="cuda")
    out = buf[GUARD_WORDS:GUARD_WORDS + size]
    out.fill_(-1)
    hip.check(call(out.data_ptr(), torch.cuda.current_stream().cuda_stream), what)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD_WORDS] == GUARD_WORD).all() and (host[GUARD_WORDS + size:] == GUARD_WORD).all(), f"{what}: a word outside the output was written"
    return host[GUARD_WORDS:GUARD_WORDS + size].view(np.uint64).reshape(n_out, blob.words)


def _contains_raw(hip, blob, pat_blob, pat_off, what):
    """arx_text_contains with the pattern store as given (uint8, int32 [P + 1]: not validated on the way)."""
    d_pb = torch.from_numpy(np.ascontiguousarray(pat_blob, dtype=np.uint8).copy()).cuda()
    d_po = torch.from_numpy(np.ascontiguousarray(pat_off, dtype=np.int32).copy()).cuda()
    n_pat = len(pat_off) - 1
    lib = hip.load()
    return _scan(hip, blob, n_pat, lambda out, st: lib.arx_text_contains(blob.view.data_ptr(), blob.off.data_ptr(), blob.n_rows, d_pb.data_ptr(),
                                                                          d_po.data_ptr(), n_pat, out, st), what)


def _regex_raw(hip, blob, d_tables, d_off, n_re, waves, what):
    lib = hip.load()
    return _scan(hip, blob, n_re, lambda out, st: lib.arx_text_regex_tuned(blob.view.data_ptr(), blob.off.data_ptr(), blob.n_rows, d_tables.data_ptr(),
                                                                           d_off.data_ptr(), n_re, out, waves, st), what)


def _same(got, want, what, rows, names, info=None, ref="python"):
    """The message of tests/test_gpu_where_document.py::_check, with the cell of the first differing row."""
    if np.array_equal(got, want):
        return
    p, w = np.argwhere(got != want)[0]
    diff = int(got[p, w] ^ want[p, w])
    r = int(w) * 64 + (diff & -diff).bit_length() - 1
    size = f"{len(rows[r])} B" if r < len(rows) else "beyond n_rows"
    cell = f", {info[r]}" if info and r in info else ""
    raise AssertionError(f"{what}: pattern {p} ({names[p][:40]!r}, {len(names[p])} B) row {r} ({size}{cell}): device "
                         f"{bool(got[p, w] >> np.uint64(r % 64) & np.uint64(1))}, {ref} {bool(want[p, w] >> np.uint64(r % 64) & np.uint64(1))}; "
                         f"{int((got != want).sum())} words differ")


def _run_contains_cases(hip, cases):
    for c in cases:
        blob = Blob(c["rows"], c["shift"], c["before"], c["after"])
        pats = c["patterns"]
        pat_off = np.cumsum([0] + [len(p) for p in pats])
        got = _contains_raw(hip, blob, np.frombuffer(b"".join(pats), dtype=np.uint8), pat_off, c["what"])
        _same(got, _pack(TC.expect(c["rows"], pats)), c["what"], c["rows"], pats, c["info"])


# ---- the substring scan: every family of tests/textscan_cases.py ------------------------------------------------------------------------
def test_contains_at_every_shift_between_guard_bytes(hip):
    """The HEAD ... TAIL corpus at shifts 0..15 and total lengths 0, 1, 8, 15 mod 16; GUARD | HEAD and TAIL | AFTER match no row."""
    cases = TC.ends_cases()
    assert {c["shift"] for c in cases} == set(range(16)) and {sum(map(len, c["rows"])) % 16 for c in cases} == {0, 1, 8, 15}
    for c in cases:
        want = TC.expect(c["rows"], c["patterns"])
        assert [sum(1 << r for r, b in enumerate(w) if b) for w in want] == [1, 32, 4, 4, 8, 4, 32, 0, 0, 0, 0, 0, 1, 0, 1, 0], c["what"]
    _run_contains_cases(hip, cases)


def test_contains_at_tile_and_halo_edges(hip):
    """A needle at in-tile positions 1023, 1024 - m, 1025 - m, 1008, 1007 of tiles 0 and 1, the row ending 0, 1, 15, 16, 17 bytes behind
    it or one byte inside it; m in {1, 3, 4, 5, 16, 17, 255, 256}, row starts at 0, 1, 15 mod 16, shifts 0 and 7."""
    _run_contains_cases(hip, TC.sweep_cases())


def test_contains_does_not_compare_what_the_waves_previous_row_left_in_lds(hip):
    _run_contains_cases(hip, TC.stale_cases())


def test_contains_with_a_full_pattern_store(hip):
    """32 x 256 bytes, 1 byte beside 256 bytes (either order), 32 x 1 byte."""
    _run_contains_cases(hip, TC.capacity_cases())


# ---- the regex scan at every shift -------------------------------------------------------------------------------------------------------
def _regex_bits(hip, rows, shift, d_tables, d_off, n_re, waves, what, before=b"", after=b""):
    return _regex_raw(hip, Blob(rows, shift, before, after), d_tables, d_off, n_re, waves, what)


def test_regex_at_every_shift_between_guard_bytes(hip):
    """The ends corpus (anchored guard regexes: ^HEAD behind GUARD, TAIL$ before AFTER) and the constructed rows of
    tests/test_gpu_where_document_regex.py at shifts 0..15, waves_per_block 0, 1 and 16, against `evaluate_host`."""
    corpora = [(f"ends pad {pad}", [r.decode() for r in TC.ends_rows(pad)], TC.ENDS_REGEXES) for pad in TC.ENDS_PADS]
    corpora.append(("constructed", TC.regex_constructed_rows(), TC.REGEX_CONSTRUCTED_PATTERNS))
    for name, texts, patterns in corpora:
        want = np.stack([pack_bitmap(evaluate_host(("regex", p), texts)) for p in patterns])
        if name.startswith("ends"):
            assert [int(w[0]) for w in want] == [1, 32, 0, 0, 0, 0, 32, 4], name
        else:
            assert want[0, 0] == np.uint64((1 << 48) - 1) and all(w.any() for w in want), name
        tb, to = pack_tables([compile_regex(p) for p in patterns])
        d_tb, d_to = torch.from_numpy(tb).cuda(), torch.from_numpy(to).cuda()
        rows = [t.encode("utf-8", "surrogatepass") for t in texts]
        for shift in range(16):
            blob = Blob(rows, shift, TC.GUARD_BEFORE, TC.GUARD_AFTER)
            for waves in REGEX_WAVES:
                what = f"regex {name}, shift {shift}, waves_per_block {waves}"
                _same(_regex_raw(hip, blob, d_tb, d_to, len(patterns), waves, what), want, what, rows, [p.encode() for p in patterns], ref="host")


# ---- device data outside the contract ----------------------------------------------------------------------------------------------------
LONG257 = TC.needle(257, seed=5)                               # occurs in a row: a length of 257 cut to 256, or taken as it is, would match


def _raw_patterns(entries, start=300):
    """entries: bytes (a valid pattern) or an int (a length outside the contract: 0, 257 or negative, i.e. a descending offset).
    -> (uint8 [1024], int32 [P + 1]).  The offsets are cumulative, so after a negative length the next pattern overlaps the previous."""
    blob, off = bytearray(b"\xee" * 1024), [start]
    for e in entries:
        if isinstance(e, bytes):
            blob[off[-1]:off[-1] + len(e)] = e
            off.append(off[-1] + len(e))
        else:
            if e > 0:
                blob[off[-1]:off[-1] + e] = LONG257[:e]
            off.append(off[-1] + e)
    for e, o in zip(entries, off):
        assert not isinstance(e, bytes) or bytes(blob[o:o + len(e)]) == e, "a valid pattern was overwritten: choose overlapping neighbours"
    return np.frombuffer(bytes(blob), dtype=np.uint8), np.asarray(off, dtype=np.int32)


def test_pattern_lengths_outside_the_contract_match_no_row(hip):
    """Lengths 0, 257 and -3 at positions 0, 2 and 4 of five patterns: that bitmap is zero, the valid patterns' equal Python's `in`."""
    valid = [b"HEAD", b"leabc", b"abcde", b"TAIL"]             # ("leabc" | "abcde" overlap in "abc": the neighbours of a length of -3)
    rows = [b"HEAD of it", b"xx leabcde TAIL", b"", LONG257 + b"zz", b"q" + LONG257[:256], b"whole TAIL", b"\xee" * 40, LONG257[:-1]]
    for shift in (0, 5):
        blob = Blob(rows, shift, TC.GUARD_BEFORE, TC.GUARD_AFTER)
        for bad in (0, 257, -3):
            for pos in (0, 2, 4):
                entries = valid[:pos] + [bad] + valid[pos:]
                pb, po = _raw_patterns(entries)
                assert int(po[pos + 1] - po[pos]) == bad and len(entries) == 5
                what = f"pattern length {bad} at position {pos}, shift {shift}"
                got = _contains_raw(hip, blob, pb, po, what)
                pats = [e if isinstance(e, bytes) else b"" for e in entries]
                want = _pack(TC.expect(rows, pats))
                assert not want[pos].any() and all(want[p].any() for p in range(5) if p != pos)
                _same(got, want, what, rows, [e if isinstance(e, bytes) else b"<length %d>" % e for e in entries])


def _table_bytes(dfa):
    return pack_tables([dfa])[0].tobytes()


def _host_bits(dfas, rows):
    """uint64 [len(dfas), words]: `match_host`; None in `dfas` = a table that matches no row."""
    return _pack([[d is not None and match_host(d, r) for r in rows] for d in dfas])


def _regex_pieces(hip, blob, pieces, waves, what):
    """arx_text_regex_tuned on tables laid out as the byte strings `pieces`, table_off = their cumulative lengths."""
    tables = np.frombuffer(b"".join(pieces) + b"\xff" * 16, dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(p) for p in pieces]).astype(np.int32)
    return _regex_raw(hip, blob, torch.from_numpy(tables).cuda(), torch.from_numpy(off).cuda(), len(pieces), waves, what)


def test_regex_tables_outside_the_contract_match_no_row(hip):
    """One table of three with a header of 0 or 257, a slice one byte too short, a slice of 3 bytes: that regex matches no row and the
    other two are unaffected.  A gap of 5 unused bytes behind a table changes nothing."""
    dfas = [compile_regex(p) for p in ("ab", "a$", "^b")]
    good = [_table_bytes(d) for d in dfas]
    rows = [b"ab", b"ba", b"a", b"b", b"", b"xxab", b"b" * 17, b"x" * 15 + b"a", b"abxa", b"q" * 300 + b"a"]
    full = _host_bits(dfas, rows)
    assert all(w.any() for w in full)
    room = TC.MAX_LEN + 1                                      # bytes enough for a header of 257 x 257, so that only the header is wrong
    room = 4 + 256 + room + room * room

    def header(t, ns=None, nc=None):
        h = np.frombuffer(t[:4], dtype="<u2").copy()
        h[0], h[1] = (h[0] if ns is None else ns), (h[1] if nc is None else nc)
        return (h.tobytes() + t[4:]).ljust(room, b"\x00")

    variants = [("n_states 0", lambda t: header(t, ns=0)), ("n_states 257", lambda t: header(t, ns=257)),
                ("n_classes 0", lambda t: header(t, nc=0)), ("n_classes 257", lambda t: header(t, nc=257)),
                ("one byte short", lambda t: t[:-1]), ("three bytes", lambda t: t[:3])]
    for shift in (0, 3):
        blob = Blob(rows, shift, TC.GUARD_BEFORE, TC.GUARD_AFTER)
        for i, (name, damage) in enumerate(variants):
            for k in sorted({i % 3, 2}):                        # (the last table: its slice ends where the tables do)
                pieces = list(good)
                pieces[k] = damage(good[k])
                want = full.copy()
                want[k] = 0
                for waves in REGEX_WAVES:
                    what = f"table {k} of 3 with {name}, shift {shift}, waves_per_block {waves}"
                    _same(_regex_pieces(hip, blob, pieces, waves, what), want, what, rows, [d.pattern.encode() for d in dfas], ref="host")
        for k in (0, 1, 2):
            pieces = list(good)
            pieces[k] = good[k] + b"\xff" * 5
            what = f"5 unused bytes behind table {k}, shift {shift}"
            _same(_regex_pieces(hip, blob, pieces, 0, what), full, what, rows, [d.pattern.encode() for d in dfas], ref="host")


def _raw_table(n_states, n_classes, class_of, flags, trans):
    head = np.array([n_states, n_classes], dtype="<u2").tobytes()
    return head + np.asarray(class_of, np.uint8).tobytes() + np.asarray(flags, np.uint8).tobytes() + np.asarray(trans, np.uint8).tobytes()


def test_classes_and_transitions_out_of_range_are_read_as_0(hip):
    """A compiled table with some classes >= n_classes and some transitions >= n_states (none of them in a MATCHED / DEAD state, which
    stays absorbing), against `match_host` on the table with "read as 0" applied on the host."""
    dfa = compile_regex("ab+c|x[0-9]y")
    ns, nc = dfa.n_states, dfa.n_classes
    assert ns < 200 and nc < 200
    class_of, trans = dfa.class_of.copy(), dfa.trans.copy()
    class_of[ord("b")], class_of[ord("q")], class_of[ord("5")] = nc, 255, nc + 7
    walk = [s for s in range(ns) if not dfa.flags[s] & (MATCHED | DEAD)]
    stop = [s for s in range(ns) if dfa.flags[s] & (MATCHED | DEAD)]
    assert len(walk) >= 3 and stop
    trans[walk[1], dfa.class_of[ord("c")]] = ns                # the first value out of range, and the last
    trans[walk[-1], dfa.class_of[ord("y")]] = 255
    trans[walk[2], :] = np.where(np.arange(nc) % 2 == 0, ns + 1, trans[walk[2], :])
    fixed_cls = np.where(class_of < nc, class_of, 0).astype(np.uint8)
    fixed_tr = np.where(trans < ns, trans, 0).astype(np.uint8)
    assert all((fixed_tr[s] == s).all() for s in stop), "a MATCHED / DEAD state must stay absorbing"
    assert (class_of >= nc).sum() == 3 and (trans >= ns).sum() >= 3
    fixed = RegexDFA("read as 0", ns, nc, fixed_cls, dfa.flags, fixed_tr)
    rows = [b"abc", b"abbbc", b"x5y", b"ac", b"qq abc", b"ab", b"", b"xay", b"x7y", b"a" * 16 + b"bc", b"z" * 33 + b"x9y", b"abcabc", b"c", b"axc",
            b"ab" * 150 + b"c"]
    want, untouched = _host_bits([fixed], rows), _host_bits([dfa], rows)
    assert not np.array_equal(want, untouched) and want.any(), "the damage must change a bit, or the case proves nothing"
    piece = _raw_table(ns, nc, class_of, dfa.flags, trans)
    for shift in (0, 13):
        blob = Blob(rows, shift, TC.GUARD_BEFORE, TC.GUARD_AFTER)
        for waves in REGEX_WAVES:
            what = f"classes and transitions out of range, shift {shift}, waves_per_block {waves}"
            _same(_regex_pieces(hip, blob, [piece], waves, what), want, what, rows, [b"ab+c|x[0-9]y (damaged)"], ref="host")
            both = _regex_pieces(hip, blob, [_table_bytes(dfa), piece, _table_bytes(dfa)], waves, what)
            _same(both, np.concatenate([untouched, want, untouched]), what + " beside the untouched table", rows, [b"untouched", b"damaged", b"untouched"], ref="host")


# ---- hand-made tables --------------------------------------------------------------------------------------------------------------------
COUNTER = bytes((37 * i + 11) % 255 + 1 for i in range(255))   # the 255 bytes table 5 counts (0 is not among them)


def _hand_tables():
    one = np.zeros(256, np.uint8)
    t1 = RegexDFA("one state, MATCHED", 1, 1, one, np.array([MATCHED], np.uint8), np.zeros((1, 1), np.uint8))
    t2 = RegexDFA("one state, DEAD", 1, 1, one, np.array([DEAD], np.uint8), np.zeros((1, 1), np.uint8))
    t3 = RegexDFA("one state, ACCEPT_AT_END", 1, 1, one, np.array([ACCEPT_AT_END], np.uint8), np.zeros((1, 1), np.uint8))
    is_a = np.zeros(256, np.uint8)
    is_a[ord("a")] = 1
    t4 = RegexDFA("last byte is a", 2, 2, is_a, np.array([0, ACCEPT_AT_END], np.uint8), np.array([[0, 1], [0, 1]], np.uint8))
    # state i = "the last i bytes were COUNTER[:i]" (a mismatch falls back to 1 if the byte is COUNTER[0], else to 0); 255 = MATCHED
    trans = np.zeros((256, 256), np.uint8)
    trans[:255, COUNTER[0]] = 1
    for i in range(255):
        trans[i, COUNTER[i]] = i + 1
    trans[255, :] = 255
    flags = np.zeros(256, np.uint8)
    flags[255] = MATCHED
    t5 = RegexDFA("counter of 255 bytes", 256, 256, np.arange(256, dtype=np.uint8), flags, trans)
    return [t1, t2, t3, t4, t5]


def test_hand_made_tables(hip):
    """One-state tables whose start state is MATCHED, DEAD or ACCEPT_AT_END, a two-state two-class table and a 256-state 256-class
    counter, over rows of 0, 1, 15, 16, 17 and 300 bytes, against `match_host`."""
    dfas = _hand_tables()
    rows = []
    for n in TC.HAND_ROW_LENGTHS:
        body = TC.filler(n, seed=n)
        rows += [body, body[:-1] + b"a" if n else b"", body[:-1] + b"b" if n else b""]
    broken = COUNTER[:100] + bytes([COUNTER[100] ^ 1]) + COUNTER[101:]
    rows += [TC.filler(45, 1) + COUNTER, COUNTER + TC.filler(44, 2) + b"a", TC.filler(45, 3) + broken, TC.filler(46, 4) + COUNTER[:254],
             COUNTER[:7] + COUNTER + TC.filler(38, 5), COUNTER[:1] * 45 + COUNTER, COUNTER[1:] + TC.filler(46, 6), COUNTER[:254], COUNTER]
    assert {len(r) for r in rows} >= set(TC.HAND_ROW_LENGTHS) and max(map(len, rows)) == 300 and len(COUNTER) == 255 == len(set(COUNTER))
    want = _host_bits(dfas, rows)
    n = len(rows)
    everyone = pack_bitmap(np.ones(n, bool))
    assert np.array_equal(want[0], everyone) and not want[1].any() and np.array_equal(want[2], everyone)
    assert [r for r in range(n) if match_host(dfas[3], rows[r])] == [r for r in range(n) if rows[r].endswith(b"a")] != []
    assert [r for r in range(n) if match_host(dfas[4], rows[r])] == [r for r in range(n) if COUNTER in rows[r]] and 4 <= int(sum(COUNTER in r for r in rows)) < 9
    tb, to = pack_tables(dfas)
    d_tb, d_to = torch.from_numpy(tb).cuda(), torch.from_numpy(to).cuda()
    for shift in (0, 11):
        blob = Blob(rows, shift, TC.GUARD_BEFORE, TC.GUARD_AFTER)
        for waves in REGEX_WAVES:
            what = f"hand-made tables, shift {shift}, waves_per_block {waves}"
            _same(_regex_raw(hip, blob, d_tb, d_to, len(dfas), waves, what), want, what, rows, [d.pattern.encode() for d in dfas], ref="host")
        for k, d in enumerate(dfas):                            # and each alone: the table is the only one the block stages
            t1, o1 = pack_tables([d])
            what = f"hand-made table {k + 1} alone, shift {shift}"
            got = _regex_raw(hip, blob, torch.from_numpy(t1).cuda(), torch.from_numpy(o1).cuda(), 1, 0, what)
            _same(got, want[k:k + 1], what, rows, [d.pattern.encode()], ref="host")
