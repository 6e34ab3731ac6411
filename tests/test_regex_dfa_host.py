"""The host half of `$regex` / `$not_regex`: `regex_dfa.compile_regex` against Python's `re` (hand table and a seeded random sweep), its
refusals and limits, `pack_tables`, and the opt-in switch of `compile_where_document`, `evaluate_host`, the collection and the CLI.
No GPU."""
import re

import numpy as np
import pytest

from arxiv_rag_amd import regex_dfa as R
from arxiv_rag_amd.regex_dfa import compile_regex, match_host, pack_tables
from arxiv_rag_amd.where_document import MAX_REGEXES, compile_where_document, encode_text, evaluate_host, patterns_of, regexes_of


def translate(p):
    """-> (pattern for `re`, flags): `^` -> `\\A`, `$` -> `\\Z` outside classes, the leading flag group moved into `flags`."""
    flags = re.ASCII
    for f in ("(?is)", "(?si)", "(?i)", "(?s)"):
        if p.startswith(f):
            p = p[len(f):]
            flags |= (re.I if "i" in f else 0) | (re.S if "s" in f else 0)
            break
    out, i, in_class = [], 0, False
    while i < len(p):
        c = p[i]
        if c == "\\":
            out.append(p[i:i + 2])
            i += 2
            continue
        if in_class:
            in_class = c != "]"
        elif c == "[":
            in_class = True
            if p[i + 1:i + 2] == "^":
                out.append("[")
                c, i = "^", i + 1
        elif c == "^":
            c = "\\A"
        elif c == "$":
            c = "\\Z"
        out.append(c)
        i += 1
    return "".join(out), flags


def agree(pattern, text):
    tp, flags = translate(pattern)
    return match_host(compile_regex(pattern), text.encode()) == bool(re.search(tp, text, flags))


HAND_PATTERNS = [
    "abc", "é", "中", "😀", "a😀b", "é+x", "[à-ü]x", "[中-文]", "[^a]", "[^é]", "[^a-z中]", "[abc]", "[a-c]x", "[a\\-c]", "[-a]", "[a-]", "[\\d\\s]x",
    ".", "a.c", "(?s)a.c", "(?s).", "(?is)A.C", "(?si)a.c", "a\\.c", "\\x41", "\\n", "\\t", "a\\/b", "\\$", "\\^a",
    "\\d{4}\\.\\d{4,5}", "[A-Z][a-z]+ et al\\.", "(?i)transformer", "(?i)[^a]b", "(?i)[x-z]+!", "\\w+@\\w+", "\\W", "\\S\\s", "\\D\\d",
    "^a", "a$", "^a$", "^$", "$", "^", "(^a|b)c", "a(b|$)", "a$b", "$^", "a*$^b*", "^(a|b)+$",
    "a{3}", "a{2,}", "a{1,2}b", "x{2,}?y", "a{0}b", "(ab){2}", "(a|b)*a(a|b){5}", "(?:ab|cd)+e", "a|b|c", "ab|", "(|a)b", "()", "a*", "a*?", "a+?b", "a??b",
    "a?", "(a*)*b",
]
HAND_TEXTS = ["", "a", "b", "abc", "xabc", "abcx", "a\nc", "a\rc", "\n", "é", "ééx", "xé", "中", "文", "😀", "a😀b", "aéc", "a中c", "a😀c", "üx", "AbC", "A\nC",
              "arXiv:2101.00001v2", "2101.0001", "Smith et al. 2020", "Smith et al", "TransFormer", "xb", "Ab", "ab", "ba", "bc", "ac", "xxy", "a b", "z-", "A",
              "aaaaab", "baaaaaa", "abab", "cde", "ab@cd", "Z!", "a.c", "a/b", "$", "^a", "1a", "\t"]


def test_hand_table_agrees_with_python_re():
    bad = [(p, t) for p in HAND_PATTERNS for t in HAND_TEXTS if not agree(p, t)]
    assert not bad, bad[:10]
    # a match at the first and at the last byte of a long text, and nowhere
    for text, want in (("é" + "x" * 300, True), ("x" * 300 + "é", True), ("x" * 300, False)):
        assert match_host(compile_regex("é"), text.encode()) is want
    # every text matches an empty-match pattern, the empty text included
    for p in ("a*", "()", "a|", "$", "^", "(?i)"):
        assert all(match_host(compile_regex(p), t.encode()) for t in HAND_TEXTS), p
    assert compile_regex("a*").n_states == 1


ATOMS = ("a", "b", ".", "[ab]", "[^a]", "\\d", "é")
TEXT_ALPHABET = ("a", "b", "1", "\n", "é", "中")


def generate(rs, depth):
    """A pattern from the grammar atom | concatenation | alternation | quantified group, `depth` levels of nesting at the most."""
    kind = rs.randint(4) if depth > 0 else 0
    if kind == 0:
        return ATOMS[rs.randint(len(ATOMS))]
    if kind == 1:
        return "".join(generate(rs, depth - 1) for _ in range(rs.randint(2, 4)))
    if kind == 2:
        return "(" + "|".join(generate(rs, depth - 1) for _ in range(rs.randint(2, 4))) + ")"
    quant = ("*", "+", "?", "{2}", "{1,3}", "{2,}", "*?")[rs.randint(7)]
    return "(?:" + generate(rs, depth - 1) + ")" + quant


def test_random_sweep_agrees_with_python_re():
    rs = np.random.RandomState(20240607)
    checked = skipped = n_patterns = 0
    for _ in range(600):
        p = generate(rs, 3)
        if rs.randint(4) == 0:
            p = ("^" + p, p + "$", "(?s)" + p, "(?i)" + p)[rs.randint(4)]
        n_patterns += 1
        try:
            dfa = compile_regex(p)
        except ValueError as e:                                # only the state limits may refuse a generated pattern
            assert "DFA states" in str(e), (p, str(e))
            skipped += 1
            continue
        tp, flags = translate(p)
        rx = re.compile(tp, flags)
        for _ in range(6):
            t = "".join(TEXT_ALPHABET[j] for j in rs.randint(len(TEXT_ALPHABET), size=rs.randint(0, 13)))
            assert match_host(dfa, t.encode()) == bool(rx.search(t)), (p, t)
            checked += 1
    assert skipped <= 0.05 * n_patterns, (skipped, n_patterns)
    assert checked >= 3000


REFUSED = [
    ("", "empty pattern"), ("a" * 257, "257 bytes"), ("é" * 129, "258 bytes"), ("(a)\\1", "backreference"), ("(?=a)b", "look-around"), ("(?!a)b", "look-around"),
    ("(?<=a)b", "look-around"), ("(?<!a)b", "look-around"), ("\\bword", "\\\\b"), ("a\\B", "\\\\B"), ("\\Aa", "\\\\A"), ("a\\z", "\\\\z"), ("a\\Z", "\\\\Z"),
    ("\\p{L}", "Unicode class"), ("\\P{L}", "Unicode class"), ("[[:alpha:]]", "alpha"), ("(?P<n>a)", "named group"), ("(?<n>a)", "named group"),
    ("(?m)^a", "flag"), ("(?x)a", "flag"), ("a(?i)b", "flag"), ("(?i:a)", "flag"), ("\\xff", "above 7F"), ("\\x80", "above 7F"), ("a{256}", "above 255"),
    ("a{1,256}", "above 255"), ("(a", "unbalanced"), ("a)", "unbalanced"), ("[a", "unbalanced"), ("a]", "unbalanced"), ("a}", "unbalanced"), ("*a", "dangling"),
    ("a|+", "dangling"), ("(?:*)", "dangling"), ("a\\", "dangling backslash"), ("a{", "'\\{'"), ("a{,3}", "'\\{'"), ("a{x}", "'\\{'"), ("a**", "doubled"),
    ("a{2}{3}", "doubled"), ("a{2,1}", "max below min"), ("[z-a]", "reversed"), ("[]", "empty class"), ("[a[b]]", "inside a class"), ("[a&&b]", "&&"),
    ("^*", "anchor"), ("\\q", "unknown escape"), ("[a-\\d]", "end of a range"), ("\\xg1", "\\\\x"),
]


@pytest.mark.parametrize("pattern,names", REFUSED)
def test_refusals_name_the_construct_and_the_pattern(pattern, names):
    with pytest.raises(ValueError, match=names) as e:
        compile_regex(pattern)
    assert pattern == "" or repr(pattern)[1:20] in str(e.value)
    with pytest.raises(ValueError, match="must be a string"):
        compile_regex(7)


def test_state_limits():
    assert compile_regex("(a|b)*a(a|b){5}").n_states <= 256
    with pytest.raises(ValueError, match="4096 DFA states.*\\(a\\|b\\)\\*a"):
        compile_regex("(a|b)*a(a|b){12}")
    # 2^7 remembered bytes and the final byte: one state too many after minimisation; one repetition fewer, twice, is exactly the limit
    with pytest.raises(ValueError, match="257 DFA states after minimisation, at most 256.*a\\[ab\\]"):
        compile_regex("a[ab]{7}c")
    assert compile_regex("a[ab]{6}c|d[de]{6}f").n_states == 256
    with pytest.raises(ValueError, match="DFA states"):
        compile_regex(".{255}x")


def test_pack_tables_layout_and_ranges():
    dfas = [compile_regex(p) for p in ("a*", "a", "\\d{4}\\.\\d{4,5}", "(?i)transformer", "[^é]$", "a[ab]{6}c|d[de]{6}f", "^$", ".")]
    tables, off = pack_tables(dfas)
    assert tables.dtype == np.uint8 and off.dtype == np.int32 and off[0] == 0 and off[-1] == tables.shape[0] and len(off) == 9
    for d, a, b in zip(dfas, off[:-1], off[1:]):
        t = tables[a:b]
        ns, nc = int(t[0]) | int(t[1]) << 8, int(t[2]) | int(t[3]) << 8
        assert (ns, nc) == (d.n_states, d.n_classes) and 1 <= ns <= 256 and 1 <= nc <= 256 and b - a == 4 + 256 + ns + ns * nc
        class_of, flags, trans = t[4:260], t[260:260 + ns], t[260 + ns:].reshape(ns, nc)
        assert int(class_of.max()) < nc and int(trans.max()) < ns and int(flags.max()) < 8
        assert np.array_equal(class_of, d.class_of) and np.array_equal(flags, d.flags) and np.array_equal(trans, d.trans)
        stop = np.nonzero(flags & (R.MATCHED | R.DEAD))[0]
        assert (trans[stop] == stop[:, None]).all()            # absorbing: stopping there changes no answer
        assert not (flags & R.DEAD).astype(bool)[(flags & (R.MATCHED | R.ACCEPT_AT_END)) != 0].any()
    assert dfas[0].n_states == 1 and dfas[0].flags[0] & R.MATCHED
    assert dfas[5].n_states == 256
    assert compile_regex("^a").flags.tolist().count(R.DEAD) == 1  # an anchored pattern that failed can stop
    for n in (0, 9):
        with pytest.raises(ValueError, match="1..8"):
            pack_tables(dfas[:1] * n)


def test_compile_where_document_switch():
    for f in ({"$regex": "a"}, {"$not_regex": "a"}, {"$and": [{"$contains": "x"}, {"$regex": "a"}]}):
        with pytest.raises(ValueError, match="unknown operator '\\$(not_)?regex'"):
            compile_where_document(f)
        with pytest.raises(ValueError, match="unknown operator '\\$(not_)?regex'"):
            compile_where_document(f, regex=False)
    assert compile_where_document({"$regex": "a"}, regex=True) == ("regex", "a")
    assert compile_where_document({"$not_regex": "a|b"}, regex=True) == ("not_regex", "a|b")
    plain = {"$and": [{"$contains": "x"}, {"$not_contains": "y"}]}
    assert compile_where_document(plain, regex=True) == compile_where_document(plain)
    tree = compile_where_document({"$or": [{"$regex": "a+"}, {"$and": [{"$contains": "x"}, {"$not_regex": "a+"}, {"$not_regex": "\\d"}]}]}, regex=True)
    assert regexes_of(tree) == ["a+", "\\d"] and patterns_of(tree) == ["x"]
    # a bad pattern fails here, before any GPU work, with the construct named
    for bad, names in (("(a", "unbalanced"), ("\\bword", "\\\\b"), ("", "empty pattern"), ("a[ab]{7}c", "257 DFA states")):
        with pytest.raises(ValueError, match="where_document: operand of \\$regex: regex: .*" + names):
            compile_where_document({"$regex": bad}, regex=True)
    with pytest.raises(ValueError, match="must be a string"):
        compile_where_document({"$regex": 3}, regex=True)
    # eight distinct regexes beside 32 substrings; the ninth is refused
    assert MAX_REGEXES == 8
    eight = [{"$regex": f"a{{{j + 1}}}"} for j in range(8)]
    compile_where_document({"$or": eight + eight + [{"$contains": f"s{j}"} for j in range(32)]}, regex=True)
    with pytest.raises(ValueError, match="9 distinct regexes in one filter, at most 8"):
        compile_where_document({"$or": eight + [{"$not_regex": "b"}]}, regex=True)


def test_evaluate_host_over_mixed_trees():
    texts = ["", "alpha 12", "Beta", "beta 2101.00001", "gamma\ndelta", "é 7", "ALPHA", "alpha beta"]
    leaves = {
        "c": ({"$contains": "alpha"}, lambda t: "alpha" in t), "nc": ({"$not_contains": "beta"}, lambda t: "beta" not in t),
        "r": ({"$regex": "(?i)^alpha|\\d{4}\\."}, lambda t: bool(re.search(r"\Aalpha|\d{4}\.", t, re.I | re.A))),
        "nr": ({"$not_regex": "\\d$"}, lambda t: not re.search(r"\d\Z", t, re.A)),
    }
    for name, (f, py) in leaves.items():
        assert evaluate_host(compile_where_document(f, regex=True), texts).tolist() == [py(t) for t in texts], name
    c, nc, r, nr = (leaves[k] for k in ("c", "nc", "r", "nr"))
    trees = [({"$and": [c[0], nr[0]]}, lambda t: c[1](t) and nr[1](t)),
             ({"$or": [r[0], nc[0]]}, lambda t: r[1](t) or nc[1](t)),
             ({"$and": [{"$or": [c[0], r[0]]}, {"$or": [nc[0], nr[0]]}]}, lambda t: (c[1](t) or r[1](t)) and (nc[1](t) or nr[1](t))),
             ({"$or": [{"$and": [c[0], nc[0], r[0], nr[0]]}, {"$not_regex": "."}]}, lambda t: (c[1](t) and nc[1](t) and r[1](t) and nr[1](t)) or t == "")]
    for f, py in trees:
        got = evaluate_host(compile_where_document(f, regex=True), texts)
        assert got.dtype == bool and got.tolist() == [py(t) for t in texts], f
    # a lone surrogate is scanned as its bytes: `.` does not match the ill-formed sequence, a literal beside it still does
    assert evaluate_host(("regex", "^.$"), ["\ud800", "a"]).tolist() == [False, True]
    assert evaluate_host(("regex", "a"), ["\ud800a"]).tolist() == [True] and len(encode_text("\ud800")) == 3


def test_collection_and_cli_switch():
    import argparse
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from arxiv_rag_amd.retrieval import RowFilters
    from arxiv_rag_amd.store import HipCollection
    with pytest.raises(ValueError, match="document_regex=True needs documents=True"):
        HipCollection(np.zeros((4, 8), np.float32), [{}] * 4, document_regex=True)
    assert RowFilters((), "cpu", 0, 0).document_regex is False and RowFilters((), "cpu", 0, 0, document_regex=True).document_regex is True
    args = GEN.build_parser().parse_args(["in", "--where-document", '{"$regex": "a+"}', "--where-document-regex"])
    assert args.where_document_regex is True and GEN.build_parser().parse_args(["in"]).where_document_regex is False
    assert GEN.check_where_document_args(args) is None and args.where_document_filter == {"$regex": "a+"}
    off = argparse.Namespace(**{**vars(args), "where_document_regex": False})
    assert "unknown operator '$regex'" in GEN.check_where_document_args(off)
    bad = argparse.Namespace(**{**vars(args), "where_document": '{"$regex": "(a"}'})
    assert "unbalanced" in GEN.check_where_document_args(bad)
    alone = argparse.Namespace(**{**vars(args), "where_document": None})
    assert "--where-document-regex needs --where-document" in GEN.check_where_document_args(alone)
