"""What the edge tests of the text scans share (tests/test_textscan_cases_host.py, tests/test_gpu_textscan_edges.py; no tests in here):
the case builders for `text_contains_kernel` / `text_regex_kernel` (csrc/textscan.hip) and a byte-level model of the substring
kernel's walk.  No torch, no GPU: plain Python data.

A case is a dict: `rows` (list of bytes, the blob is their concatenation), `patterns` (list of bytes), `shift` (the blob's address
mod 16), `before` / `after` (the guard bytes in memory around the blob), `family`, `what` (for messages) and `info` (row -> the cell
it belongs to, for messages).  The expected bits are always Python's `in` on the bytes (`expect`).

The model (`model_contains`) is a reading aid for the kernel, not production code: tiles of 1024 start positions laid over the blob's
ADDRESS, a per-wave LDS buffer that persists from row r to row r + 4 of a 64-row group, chunks behind a row's end not refetched, the
halo fetch condition, the lo / hi start-position bounds and the early exit.  `fault` breaks one of these on purpose
(`CONTAINS_FAULTS`), so that the host test can prove that a family of cases would notice."""
import random

TILE, CHUNK, WAVES, GROUP = 1024, 16, 4, 64
MAX_LEN, MAX_PATTERNS = 256, 32
HALO = 256                                                    # TS_HALO: 16 chunks behind the tile
MAX_ROW_BYTES, MAX_ROWS = 4096, 300                           # the caps every case keeps

FILLER = b"abcdefghijklmnopqrstuvwxyz"                       # the rows' filler; needles use NEEDLE_ALPHABET, disjoint from it
NEEDLE_ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
NEAR = b"#"                                                   # in neither alphabet: the last byte of every near-miss

CONTAINS_FAULTS = ("no_hi", "halo_short", "halo_always_skipped_at_row_end", "drop_j15", "read_guards", "grid_on_row")


def filler(n, seed):
    rs = random.Random(seed)
    return bytes(rs.choice(FILLER) for _ in range(n))


def needle(m, seed=0):
    """m bytes of NEEDLE_ALPHABET, no two neighbours equal (so a needle is no shifted copy of itself at distance 1)."""
    rs = random.Random(1000 + 7 * m + seed)
    out = bytearray()
    while len(out) < m:
        c = rs.choice(NEEDLE_ALPHABET)
        if not out or out[-1] != c:
            out.append(c)
    return bytes(out)


def near_miss(pat):
    return pat[:-1] + NEAR


def place(blob_bytes, shift, before=b"", after=b""):
    """-> (buffer, offset of the blob in it).  The buffer's start is taken to be 16-byte aligned; the blob starts at 16 + shift; the
    16 + shift bytes before it hold `before`, right-aligned (zeros to its left), the bytes after it hold `after`, then zeros up to a
    multiple of 16 and one chunk more, so that every aligned 16-byte chunk that touches the blob lies inside the buffer."""
    assert 0 <= shift < CHUNK and len(before) <= CHUNK + shift
    head = bytes(CHUNK + shift - len(before)) + before
    n = len(head) + len(blob_bytes) + len(after)
    return head + blob_bytes + after + bytes((-n) % CHUNK + CHUNK), CHUNK + shift


def offsets(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return off


def expect(rows, patterns):
    """[pattern][row] -> bool: Python's `in`; a pattern outside 1..256 bytes matches no row."""
    return [[1 <= len(p) <= MAX_LEN and p in r for r in rows] for p in patterns]


def case(family, rows, patterns, shift=0, before=b"", after=b"", what="", info=None):
    return {"family": family, "rows": list(rows), "patterns": list(patterns), "shift": shift, "before": before, "after": after,
            "what": what or family, "info": info or {}}


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def model_contains(rows, patterns, shift=0, before=b"", after=b"", fault=None):
    """[pattern][row] -> bool as `text_contains_kernel` walks it.  `fault`:
      "no_hi"        the end-of-row bound on a start position is dropped: every lane tests its 16 positions, whatever LDS holds there
      "halo_short"   one halo chunk fewer is fetched
      "halo_always_skipped_at_row_end"   a halo chunk is fetched only if it lies wholly inside the row (`lane_pos + TS_TILE + 16 <= b`),
                     so the chunk that holds the row's last bytes is skipped unless the row ends with it
      "drop_j15"     start position 15 of lane 63 (in-tile position 1023, the one whose window needs the halo) is not tested
      "read_guards"  a kernel that knows nothing of the blob's ends: bytes outside [0, total) are read as they are in memory AND a
                     start position of the first row may lie before the blob, a match of the last row may run beyond it.  (Reading
                     the bytes alone, "guards_as_memory", changes no bit: the lo / hi bounds keep every comparison inside the row.
                     The zero fill of `ts_load_chunk` keeps the loads inside the allocation, not the bits right.)
      "grid_on_row"  the tile grid is laid over the row's offset (`a & ~15`), not over the address, while a full chunk is still ONE
                     aligned 16-byte access: modelled as the access dropping the address's low four bits"""
    assert fault in (None, "guards_as_memory") + CONTAINS_FAULTS, fault
    blob = b"".join(rows)
    total, off, n = len(blob), offsets(rows), len(rows)
    mem, at = place(blob, shift, before, after)
    lens = [len(p) if 1 <= len(p) <= MAX_LEN else 0 for p in patterns]
    max_len = max([1] + lens)
    halo_chunks = ((max_len - 1 if max_len > 4 else 3) + 15) >> 4
    if fault == "halo_short":
        halo_chunks -= 1
    raw = fault in ("read_guards", "guards_as_memory")

    def load(pos, chunks):
        """`chunks` consecutive 16-byte chunks from blob position `pos` (ts_load_chunk)."""
        if fault == "grid_on_row" and pos >= 0 and pos + CHUNK * chunks <= total:
            start = (at + pos) & ~15
            return mem[start:start + CHUNK * chunks]
        if pos >= 0 and pos + CHUNK * chunks <= total:
            return blob[pos:pos + CHUNK * chunks]
        out = bytearray(CHUNK * chunks)
        for i in range(CHUNK * chunks):
            p = pos + i
            if 0 <= p < total:
                out[i] = blob[p]
            elif raw and 0 <= at + p < len(mem):
                out[i] = mem[at + p]
        return bytes(out)

    found = [[False] * n for _ in patterns]
    for g in range(0, n, GROUP):
        tiles = [bytearray(TILE + HALO) for _ in range(WAVES)]   # (what LDS holds when a block starts is undefined; zeros here)
        for r in range(g, min(n, g + GROUP)):
            tile = tiles[(r - g) % WAVES]
            a, b = off[r], off[r + 1]
            rem = [p for p in range(len(patterns)) if lens[p]]
            v = (a & ~15) if fault == "grid_on_row" else ((a + shift) & ~15) - shift      # blob position of the tile's byte 0
            while v < b and rem:
                k = min(TILE // CHUNK, (b - v + CHUNK - 1) // CHUNK)                   # lanes with lane_pos < b
                tile[:CHUNK * k] = load(v, k)
                for h in range(halo_chunks):
                    pos = v + TILE + CHUNK * h
                    if (pos + CHUNK <= b) if fault == "halo_always_skipped_at_row_end" else (pos < b):
                        tile[TILE + CHUNK * h:TILE + CHUNK * (h + 1)] = load(pos, 1)
                for p in list(rem):
                    m = lens[p]
                    lo = max(0, a - v)
                    hi = min(TILE, b - m - v + 1)             # start positions s in [lo, hi) lie in the row with their whole match
                    if fault == "no_hi":
                        hi = TILE
                    if fault == "read_guards":
                        lo = 0 if a == 0 else lo
                        hi = TILE if b == total else hi
                    s = tile.find(patterns[p], lo, max(lo, hi + m - 1))
                    while s >= 0 and fault == "drop_j15" and s == TILE - 1:
                        s = tile.find(patterns[p], s + 1, max(lo, hi + m - 1))
                    if s >= 0:
                        found[p][r] = True
                        rem.remove(p)
                v += TILE
    return found


# ---- shifted blob: the ends corpus -----------------------------------------------------------------------------------------------------
GUARD_BEFORE, GUARD_AFTER = b"GUARD", b"AFTER"
ENDS_PATTERNS = [b"HEAD", b"TAIL", b"LEFT", b"RIGHT", b"whole row", b"LEFTmiddleRIGHT", b"zTAIL", b"whole row ",
                 b"GUARDHEAD", b"DHEAD", b"TAILAFTER", b"TAILA", b"Dz", b"zq"]
ENDS_REGEXES = ["^HEAD", "TAIL$", "GUARDHEAD", "DHEAD", "TAILAFTER", "TAILA", "^z*TAIL$", "LEFT.*RIGHT$"]


def ends_rows(pad):
    """The `HEAD ... TAIL` corpus of tests/test_gpu_where_document.py::test_constructed_cases: 50 + pad bytes."""
    return [b"HEAD" + b"z" * pad, b"q" * 7, b"LEFTmiddleRIGHT", b"whole row", b"", b"z" * 11 + b"TAIL"]


ENDS_PADS = (14, 15, 6, 13)                                   # total length mod 16 = 0, 1, 8, 15


def ends_cases():
    """Every shift 0..15 x total length mod 16 in {0, 1, 8, 15}.  The memory before the blob ends with GUARD and the blob starts with
    HEAD, so a kernel that let a match start outside [0, total) would find GUARDHEAD; likewise TAIL | AFTER behind it."""
    out = []
    for pad in ENDS_PADS:
        rows = ends_rows(pad)
        assert sum(map(len, rows)) % 16 == (0, 1, 8, 15)[ENDS_PADS.index(pad)]
        for shift in range(16):
            out.append(case("ends", rows, ENDS_PATTERNS + [b"D" + b"z" * pad, b"HEAD" + b"z" * pad + b"q"], shift, GUARD_BEFORE, GUARD_AFTER,
                            f"ends, total {sum(map(len, rows))} B, shift {shift}"))
    return out


# ---- tile-edge sweep ------------------------------------------------------------------------------------------------------------------
SWEEP_LENGTHS = (1, 3, 4, 5, 16, 17, 255, 256)
SWEEP_RESIDUES = (0, 1, 15)
SWEEP_SHIFTS = (0, 7)
SWEEP_TILES = (0, 1)
SWEEP_ENDS = (0, 1, 15, 16, 17)


def sweep_starts(m):
    """The in-tile start positions of a needle of m bytes: the tile's last position, the last ones that end inside the tile / first
    that reaches the halo, and the two around the last lane's first position."""
    out = []
    for s in (TILE - 1, TILE - m, TILE - m + 1, 1008, 1007):
        if 0 <= s < TILE and s not in out:
            out.append(s)
    return out


def sweep_case(shift, m, t, a):
    """One launch: for every start position s, end distance e and (whole | cut) a cell of three rows
      pad row    brings the start of the next row to a blob offset = a mod 16
      row 1      filler, then the needle at in-tile position 1024 t + s of ITS tile grid, then e filler bytes; in a cut cell the row
                 ends one byte before the needle does
      row 2      short filler; in a cut cell it begins with the needle's missing last byte.
    Patterns: the needle and its near-miss (the last byte changed)."""
    nd = needle(m)
    rows, info = [], {}
    at = 0
    for s in sweep_starts(m):
        for e in SWEEP_ENDS:
            for cut in (False, True):
                if cut and e != 0:
                    continue                                   # (a cut row ends inside the needle: e has no meaning there)
                pad = (a - at) % 16
                rows.append(filler(pad, seed=len(rows)))
                at += pad
                origin = ((at + shift) & ~15) - shift         # the tile origin of row 1, exactly as the kernel computes it
                start = origin + TILE * t + s - at            # offset of the needle in row 1
                assert start >= 0 and (origin + TILE * t + s) - (((at + shift) & ~15) - shift) == TILE * t + s
                body = filler(start, seed=1 + len(rows))
                if cut:
                    row1, row2 = body + nd[:-1], nd[-1:] + filler(5, seed=2 + len(rows))
                else:
                    row1, row2 = body + nd + filler(e, seed=3 + len(rows)), filler(5, seed=2 + len(rows))
                info[len(rows)] = f"s={s} e={e}{' cut' if cut else ''}"
                info[len(rows) + 1] = f"row after s={s} e={e}{' cut' if cut else ''}"
                rows += [row1, row2]
                at += len(row1) + len(row2)
    return case("sweep", rows, [nd, near_miss(nd)], shift, GUARD_BEFORE, GUARD_AFTER, f"sweep shift={shift} m={m} tile={t} a={a}", info) | {
        "m": m, "tile": t, "a": a}


def sweep_cases():
    """e in {1, 15, 16, 17} with a cut makes no sense, so a start position has 5 whole cells and one cut cell."""
    return [sweep_case(shift, m, t, a) for shift in SWEEP_SHIFTS for m in SWEEP_LENGTHS for t in SWEEP_TILES for a in SWEEP_RESIDUES]


# ---- stale LDS inside one wave ---------------------------------------------------------------------------------------------------------
STALE_LENGTHS = (2, 4, 5, 40, 256)
STALE_ENDS = (16, 500, 1008, 1024 + 16, 1024 + 160, 1024 + 256)   # where row r + 4 ends: in the tile, and in the halo of its first tile
STALE_SHIFTS = (0, 9)
STALE_ROW = 3 * TILE + 16                                     # row r: three tiles and one chunk (>= 1024 + 272 + 64, a multiple of 16)


def stale_case(shift, m, c, end):
    """Rows 0 and 4 share a wave and its LDS tile.  Row 0 (3088 bytes) holds needle[c:] at offset `end` mod 1024 of every one of its
    tiles, so whichever of its tiles a chunk of LDS was last written from, the bytes at in-tile offset `end` onwards are needle[c:].
    Row 4 is `end` bytes long and ends with needle[:c]: a comparison that ran past its end into what row 0 left would complete the
    needle.  Rows 1..3 are 16, 32 and 48 bytes of filler (row 4 starts at a multiple of 16, like row 0: equal in-tile offsets at any
    shift); row 5 starts with needle[c:], so the blob does hold the needle across the boundary of rows 4 and 5.
    Patterns: the needle (no row), needle[c:] (rows 0 and 5: the bytes were there) and needle[:c] (row 4)."""
    nd = needle(m, seed=1)
    head, tail = nd[:c], nd[c:]
    row0 = bytearray(filler(STALE_ROW, seed=m * 1000 + c))
    for k in range(4):
        at = end % TILE + TILE * k
        piece = tail[:max(0, STALE_ROW - at)]
        row0[at:at + len(piece)] = piece
    row4 = filler(end - c, seed=end + c) + head
    rows = [bytes(row0), filler(16, 1), filler(32, 2), filler(48, 3), row4, tail + filler(20, 4)]
    assert len(row4) == end and all(len(r) % 16 == 0 for r in rows[:4])
    return case("stale", rows, [nd, tail, head], shift, GUARD_BEFORE, GUARD_AFTER, f"stale shift={shift} m={m} cut={c} end={end}") | {
        "m": m, "cut": c, "end": end}


def stale_cases():
    out = []
    for shift in STALE_SHIFTS:
        for m in STALE_LENGTHS:
            for c in sorted({1, m // 2, m - 1}):
                for end in STALE_ENDS:
                    if c <= end:
                        out.append(stale_case(shift, m, c, end))
    return out


# ---- capacity --------------------------------------------------------------------------------------------------------------------------
def capacity_cases():
    out = []
    for shift in (0, 7):
        # 32 patterns of 256 bytes (the 8 KiB of s_pat): the odd ones are near-misses; row i holds patterns 2 (i % 16) and 2 ((7 i) % 16),
        # the first of them ending with the row
        full = [needle(256, seed=10 + p) for p in range(32)]
        pats = [full[p] if p % 2 == 0 else near_miss(full[p - 1]) for p in range(32)]
        rows = [filler(900 + 37 * i, seed=i) + pats[2 * ((7 * i) % 16)] + filler(3 * i, seed=50 + i) + pats[2 * (i % 16)] for i in range(20)]
        rows += [b"", pats[30], pats[30][1:], pats[30][:-1]]
        out.append(case("capacity", rows, pats, shift, GUARD_BEFORE, GUARD_AFTER, f"32 patterns of 256 B, shift {shift}"))
        # one 1-byte pattern beside one 256-byte pattern: the halo is the long one's, the window path serves the short one
        long = needle(256, seed=99)
        rows = [filler(1023, 1) + b"Q", filler(1023, 2) + b"Q" + filler(40, 3), filler(800, 4) + long, filler(769, 5) + long + b"Q",
                filler(2047, 6) + b"Q", filler(300, 7), b"Q", b"", filler(1000, 8) + long[:-1], long]
        out.append(case("capacity", rows, [b"Q", long], shift, GUARD_BEFORE, GUARD_AFTER, f"1 B beside 256 B, shift {shift}"))
        out.append(case("capacity", rows, [long, b"Q"], shift, GUARD_BEFORE, GUARD_AFTER, f"256 B beside 1 B, shift {shift}"))
        # 32 one-byte patterns
        ones = [bytes([c]) for c in NEEDLE_ALPHABET[:32]]
        rows = [filler(1000 + i, seed=i) + ones[i] + (ones[(5 * i) % 32] if i % 3 else b"") for i in range(32)] + [b"", ones[31], bytes(NEEDLE_ALPHABET)]
        out.append(case("capacity", rows, ones, shift, GUARD_BEFORE, GUARD_AFTER, f"32 patterns of 1 B, shift {shift}"))
    return out


def contains_cases():
    return ends_cases() + sweep_cases() + stale_cases() + capacity_cases()


# ---- rows for the regex scan ----------------------------------------------------------------------------------------------------------
REGEX_CONSTRUCTED_PATTERNS = ["abcd", "^x*😀$", "[^a-z]$", "ab", "^b", "a$", "(?i)QZ\\d$", "^(ab)+Qz9$"]


def regex_constructed_rows():
    """The rows of tests/test_gpu_where_document_regex.py::test_constructed_rows as strs, its 70 000-byte row cut to 4 003 bytes (the
    row cap of these cases)."""
    texts = ["x" * k + "abcd" + "y" * (k % 4) for k in range(48)] + ["x" * k + "😀" for k in range(20)] + ["x" * k + "é" + "z" * (k % 3) for k in range(20)]
    texts += ["xa", "bx", "a", "b", "", "", "a", "", "b", "ab", "xxab", "abxx", "b" * 16, "a" * 16, "b" * 17, "x" * 15 + "a", "b"]
    texts += ["q", "ab" * 2000 + "Qz9", "", "z", "Qz9", "Qz9 "]
    return texts


HAND_ROW_LENGTHS = (0, 1, 15, 16, 17, 300)
