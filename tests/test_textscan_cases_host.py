"""The cases of tests/textscan_cases.py can fail: the byte-level model of `text_contains_kernel` equals Python's `in` on every one of
them, and each fault of `CONTAINS_FAULTS` changes at least one expected bit of the family that is there to catch it.  No GPU."""
import pytest

from tests import textscan_cases as TC


@pytest.fixture(scope="module")
def families():
    return {"ends": TC.ends_cases(), "sweep": TC.sweep_cases(), "stale": TC.stale_cases(), "capacity": TC.capacity_cases()}


def _model(c, fault=None):
    return TC.model_contains(c["rows"], c["patterns"], c["shift"], c["before"], c["after"], fault)


def _changed(cases, fault):
    """The cases of `cases` in which the faulted model differs from Python's `in`."""
    return [c for c in cases if _model(c, fault) != TC.expect(c["rows"], c["patterns"])]


def test_place_puts_the_blob_at_16_plus_shift_between_its_guards():
    for shift in range(16):
        buf, at = TC.place(b"HEADxTAIL", shift, b"GUARD", b"AFTER")
        assert at == 16 + shift and buf[at:at + 9] == b"HEADxTAIL" and buf[at - 5:at] == b"GUARD" and buf[at + 9:at + 14] == b"AFTER"
        assert len(buf) % 16 == 0 and len(buf) >= ((at + 9 + 15) & ~15) + 16 and not any(buf[:at - 5])
    with pytest.raises(AssertionError):
        TC.place(b"x", 0, b"a" * 17)


def test_the_unfaulted_model_equals_python_in_on_every_case(families):
    n = 0
    for cases in families.values():
        for c in cases:
            assert _model(c) == TC.expect(c["rows"], c["patterns"]), c["what"]
            n += 1
    assert n == len(TC.contains_cases()) == 64 + 96 + len(families["stale"]) + 8


def test_the_size_caps_hold(families):
    for cases in families.values():
        for c in cases:
            assert 1 <= len(c["rows"]) <= TC.MAX_ROWS, (c["what"], len(c["rows"]))
            assert max(map(len, c["rows"])) <= TC.MAX_ROW_BYTES, (c["what"], max(map(len, c["rows"])))
            assert 1 <= len(c["patterns"]) <= TC.MAX_PATTERNS and all(1 <= len(p) <= TC.MAX_LEN for p in c["patterns"])
    assert max(len(t.encode()) for t in TC.regex_constructed_rows()) <= TC.MAX_ROW_BYTES and len(TC.regex_constructed_rows()) <= TC.MAX_ROWS


def test_every_sweep_holds_matching_and_non_matching_cells(families):
    for c in families["sweep"]:
        want = TC.expect(c["rows"], c["patterns"])
        cells = [r for r, what in c["info"].items() if what.startswith("s=")]
        assert any(want[0][r] for r in cells) and any(not want[0][r] for r in cells), c["what"]
        assert not any(want[1]), (c["what"], "the near-miss matches nothing")
        # a whole cell matches in its row 1 and a cut cell does not; the needle occurs nowhere else (m = 1: the cut-off byte IS the needle)
        for r in cells:
            assert want[0][r] == ("cut" not in c["info"][r]), (c["what"], c["info"][r])
            assert not want[0][r - 1] and (c["m"] == 1 or not want[0][r + 1])
        assert {c["info"][r].split()[0] for r in cells} == {f"s={s}" for s in TC.sweep_starts(c["m"])}
    assert {(c["shift"], c["m"], c["tile"], c["a"]) for c in families["sweep"]} == {
        (sh, m, t, a) for sh in TC.SWEEP_SHIFTS for m in TC.SWEEP_LENGTHS for t in TC.SWEEP_TILES for a in TC.SWEEP_RESIDUES}


def test_the_sweep_puts_the_needle_where_it_says(families):
    """The in-tile start position is recomputed from the blob alone, with the kernel's arithmetic."""
    for c in families["sweep"]:
        off, nd = TC.offsets(c["rows"]), c["patterns"][0]
        for r, what in c["info"].items():
            if not what.startswith("s=") or "cut" in what:
                continue
            s, e = int(what.split()[0][2:]), int(what.split()[1][2:])
            a = off[r]
            assert a % 16 == c["a"]
            origin = ((a + c["shift"]) & ~15) - c["shift"]
            pos = a + c["rows"][r].index(nd)
            assert pos - origin == TC.TILE * c["tile"] + s and off[r + 1] - (pos + c["m"]) == e, (c["what"], what)


def test_every_stale_case_leaves_the_tail_of_the_needle_behind_the_shorter_row(families):
    assert {(c["shift"], c["m"], c["end"]) for c in families["stale"]} >= {(sh, m, e) for sh in TC.STALE_SHIFTS for m in TC.STALE_LENGTHS
                                                                           for e in TC.STALE_ENDS if e >= m - 1}
    for c in families["stale"]:
        want = TC.expect(c["rows"], c["patterns"])
        assert not any(want[0]), c["what"]
        assert want[1][0] and want[1][5] and want[2][4], (c["what"], "the control patterns prove that the bytes are there")
        assert len(c["rows"][0]) >= 1024 + 272 + 64 and len(c["rows"][0]) % 16 == 0 and len(c["rows"][4]) == c["end"]


# fault -> (family that must notice, the cases of it that must, a name for the message)
MUST_CHANGE = {
    "no_hi": ("stale", lambda c: True, "stale LDS"),
    "halo_short": ("sweep", lambda c: c["m"] >= 255, "sweep at m >= 255"),
    "halo_always_skipped_at_row_end": ("sweep", lambda c: True, "sweep"),
    "drop_j15": ("sweep", lambda c: True, "sweep at s = 1023"),
    "read_guards": ("ends", lambda c: True, "shifted blob"),
    "grid_on_row": ("ends", lambda c: True, "shifted blob"),
}


@pytest.mark.parametrize("fault", TC.CONTAINS_FAULTS)
def test_each_fault_changes_a_bit_of_the_family_that_is_there_to_catch_it(families, fault):
    family, keep, name = MUST_CHANGE[fault]
    cases = [c for c in families[family] if keep(c)]
    changed = _changed(cases, fault)
    assert changed, f"{fault} changes no bit of the {name} cases: they prove nothing about it"
    if fault == "no_hi":
        # not one lucky case: the bound is crossed at both shifts, for every needle length and where row r + 4 ends in the tile and in the halo
        assert {c["shift"] for c in changed} == set(TC.STALE_SHIFTS) and {c["m"] for c in changed} == set(TC.STALE_LENGTHS)
        assert {c["end"] for c in changed} == set(TC.STALE_ENDS)
    if fault == "halo_short":
        assert {(c["shift"], c["m"], c["tile"], c["a"]) for c in changed} == {(c["shift"], c["m"], c["tile"], c["a"]) for c in cases}
    if fault == "drop_j15":
        for c in changed:                                       # only the cells at s = 1023 change, and in every sweep one does
            got, want = _model(c, fault), TC.expect(c["rows"], c["patterns"])
            rows = [r for r in range(len(c["rows"])) if got[0][r] != want[0][r]]
            assert rows and all(c["info"][r].startswith("s=1023 ") for r in rows), c["what"]
        assert len(changed) == len(cases)
    if fault == "grid_on_row":
        assert {c["shift"] for c in changed} == set(range(1, 16)), "every shift but 0 moves the grid against the blob"
    if fault == "read_guards":                                  # the head of the blob at every shift but 0, its tail wherever it ends inside a chunk
        head = {c["shift"] for c in changed if any(_model(c, fault)[c["patterns"].index(p)][0] for p in (b"GUARDHEAD", b"DHEAD"))}
        tail = {c["shift"] for c in changed if any(_model(c, fault)[c["patterns"].index(p)][5] for p in (b"TAILAFTER", b"TAILA"))}
        assert head == set(range(1, 16)) and tail == set(range(16))


def test_reading_the_guard_bytes_alone_changes_no_bit(families):
    """Why "read_guards" is a compound fault: with the lo / hi bounds in place no comparison leaves the row, so what a chunk holds
    outside [0, total) cannot reach a bit."""
    for cases in families.values():
        assert not _changed(cases, "guards_as_memory")
