"""Facet counts on the device (-m gpu): `arx_facet_count` against `facets.bin_counts_host` counter for counter, between canary words;
contention and skew; launch-shape independence through `arx_facet_count_tuned`; bad device data; the host-side limits;
`HipCollection.facets` and the CLI against `facets.oracle`.  Every comparison is exact integer equality."""
import ctypes
import json
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from arxiv_rag_amd import facets as F
from arxiv_rag_amd.where import compile_where, evaluate, pack_bitmap

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 4097, 70001)
BIN_COUNTS = (1, 2, 8190, 8191, 20000)                       # 8190 + 2 counters is the last size the default LDS histogram takes
CANARY, PAD = 0x5A5A5A5A, 8
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from arxiv_rag_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


class Key:
    """One key of a call: host arrays (for `bin_counts_host`) and their device copies."""

    def __init__(self, mode, want, n_bins, kind, val, cuts=None):
        self.mode, self.want, self.n_bins = mode, want, n_bins
        self.kind, self.val = np.ascontiguousarray(kind, np.uint8), np.ascontiguousarray(val, np.float64)
        self.cuts = None if cuts is None else np.ascontiguousarray(cuts, np.float64)
        self.d_kind, self.d_val = torch.from_numpy(self.kind).to(DEV), torch.from_numpy(self.val).to(DEV)
        self.d_cuts = None if cuts is None else torch.from_numpy(self.cuts).to(DEV)

    def want_counts(self, mask):
        return F.bin_counts_host(self.mode, self.want, self.n_bins, self.cuts, self.kind, self.val, mask)


def code_key(n, n_bins, seed, want=2):
    """A CODE column: mostly valid codes, some rows of another kind, a few codes that have no bin."""
    rs = np.random.RandomState(seed)
    kind = np.where(rs.rand(n) < 0.9, want, rs.randint(0, 4, n)).astype(np.uint8)
    val = rs.randint(0, n_bins, n).astype(np.float64)
    val[rs.rand(n) < 0.02] = n_bins
    return Key(F.CODE, want, n_bins, kind, val)


def exact_key(n, n_bins, seed):
    rs = np.random.RandomState(seed)
    cuts = np.unique(np.concatenate([[-np.inf, 0.0], np.abs(rs.randn(n_bins * 2)) + 1e-9]))[:n_bins]     # -inf, 0.0, then positives
    kind = np.where(rs.rand(n) < 0.9, 1, rs.randint(0, 4, n)).astype(np.uint8)
    val = cuts[rs.randint(0, n_bins, n)].copy()
    val[val == 0.0] = -0.0                                     # -0.0 finds 0.0
    miss = rs.rand(n) < 0.05
    val[miss] = rs.choice([np.nan, 1e9, 0.123456789], size=int(miss.sum()))
    return Key(F.EXACT, 1, n_bins, kind, val, cuts)


def interval_key(n, n_bins, seed):
    rs = np.random.RandomState(seed)
    edges = np.linspace(-1.0, 1.0, n_bins + 1)
    kind = np.where(rs.rand(n) < 0.9, 1, rs.randint(0, 4, n)).astype(np.uint8)
    val = rs.uniform(-1.2, 1.2, n)
    on_edge = rs.rand(n) < 0.3
    val[on_edge] = edges[rs.randint(0, n_bins + 1, int(on_edge.sum()))]          # values exactly on every edge, the last one included
    val[rs.rand(n) < 0.02] = np.nan
    return Key(F.INTERVAL, 1, n_bins, kind, val, edges)


def bitmaps_for(n, seed=0):
    """bool [5, n]: all zero, all ones, random 1 %, a contiguous range that starts and ends mid-word, random half."""
    rs = np.random.RandomState(seed)
    contiguous = np.zeros(n, bool)
    contiguous[min(n - 1, 7 + n // 5):max(1, n - n // 3 - 3)] = True
    return np.stack([np.zeros(n, bool), np.ones(n, bool), rs.rand(n) < 0.01, contiguous, rs.rand(n) < 0.5])


def pack(masks, n):
    """bool [F, n] -> uint64 [F, W], the bits of the last word at or beyond n all SET (the kernel must not count them)."""
    words = np.stack([pack_bitmap(m) for m in masks]).astype(np.uint64)
    if n % 64:
        words[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return words


def run(keys, n, masks=None, stride_zero=False, tuned=None, n_filters=None, gap=0):
    """One call over `keys` -> int64 [F, out_stride] from the host, the canaries on both sides of `out` checked.  `masks`: None (allow is
    NULL) or bool [F, n] (stride_zero: one mask, shared by `n_filters` filters).  `out` holds garbage before the call."""
    offs, stride = [], gap
    for k in keys:
        offs.append(stride)
        stride += k.n_bins + 2 + gap
    nf = n_filters if n_filters is not None else (1 if masks is None else len(masks))
    buf = torch.full((PAD + nf * stride + PAD,), CANARY, dtype=torch.int32, device=DEV)
    out = buf[PAD:PAD + nf * stride]
    out.fill_(-7)
    allow = None if masks is None else torch.from_numpy(pack(masks, n).view(np.int64)).to(DEV)
    F.launch([(k.d_kind, k.d_val, k.d_cuts, k.mode, k.want, k.n_bins, off) for k, off in zip(keys, offs)], n, allow,
             0 if (allow is None or stride_zero) else (n + 63) // 64, nf, out, stride, tuned=tuned)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all(), "a canary word beside out was overwritten"
    return host[PAD:-PAD].reshape(nf, stride).astype(np.int64), offs


def check(keys, n, masks=None, stride_zero=False, tuned=None, n_filters=None, gap=0):
    got, offs = run(keys, n, masks, stride_zero, tuned, n_filters, gap)
    nf = got.shape[0]
    for f in range(nf):
        m = None if masks is None else masks[0 if stride_zero else f]
        allowed = n if m is None else int(m.sum())
        for k, off in zip(keys, offs):
            mine = got[f, off:off + k.n_bins + 2]
            want = k.want_counts(m)
            assert np.array_equal(mine, want), (n, k.mode, k.n_bins, f, np.nonzero(mine != want)[0][:5], mine[mine != want][:5], want[mine != want][:5])
            assert int(mine.sum()) == allowed                      # every key's counters sum to the bitmap's popcount below n
    if gap:
        covered = np.zeros(got.shape[1], bool)
        for k, off in zip(keys, offs):
            covered[off:off + k.n_bins + 2] = True
        assert (got[:, ~covered] == 0).all()                       # the call zeroes the whole slice
    return got


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_kernel_against_count_host(hip, n):
    masks = bitmaps_for(n, seed=n)
    for nb in BIN_COUNTS:
        key = code_key(n, nb, seed=nb + n)
        check([key], n)                                            # allow == NULL
        check([key], n, masks)                                     # 5 filters, a real stride
        check([key], n, masks[4:5], stride_zero=True, n_filters=2) # 2 filters sharing one bitmap
        check([key], n, masks[2:4])                                # 2 filters, a real stride
    rs = np.random.RandomState(n)
    many = rs.rand(64, n) < rs.rand(64, 1)
    check([exact_key(n, 300, seed=n)], n, many)                    # 64 filters, a real stride
    check([interval_key(n, 40, seed=n)], n, many[:1], stride_zero=True, n_filters=64)      # 64 filters, stride 0
    check([interval_key(n, 1, seed=n + 1)], n, many[:3])


@pytest.mark.parametrize("n", (65, 70001))
def test_sixteen_keys_of_mixed_modes_in_one_call(hip, n):
    keys = []
    for j, nb in enumerate((1, 2, 7, 300, 8190, 8191, 20000, 64, 3, 2, 1000, 8190, 12, 9000, 5, 2)):
        make = (code_key, exact_key, interval_key)[j % 3]
        keys.append(make(n, nb, seed=17 * j + n) if make is not code_key else code_key(n, nb, seed=17 * j + n, want=(2, 3)[j % 2]))
    masks = bitmaps_for(n, seed=5)
    check(keys, n, masks[2:4], gap=3)
    check(keys, n)
    check(keys[:5], n, masks[3:4], stride_zero=True, n_filters=64)


def test_contention_and_skew(hip):
    n, rs = 70001, np.random.RandomState(11)
    masks = bitmaps_for(n, seed=3)[1:]
    kind = np.full(n, 2, np.uint8)
    for nb in (1, 50, 20000):                                      # every row in one bin: LDS and direct
        check([Key(F.CODE, 2, nb, kind, np.full(n, nb - 1, np.float64))], n, masks)
    zipf = np.minimum(rs.zipf(1.3, n) - 1, 19999).astype(np.float64)
    check([Key(F.CODE, 2, 20000, kind, zipf), Key(F.CODE, 2, 8190, kind, np.minimum(zipf, 8189))], n, masks)
    for run_len in (1, 64, 200):                                   # the wave-combined add (whole words agree) and its fallbacks
        codes = (np.arange(n) // run_len).astype(np.float64)
        check([Key(F.CODE, 2, 20000, kind, codes % 20000), Key(F.CODE, 2, 50, kind, codes % 50)], n, masks)
        check([Key(F.CODE, 2, 20000, kind, codes % 20000)], n)
    check([Key(F.CODE, 2, 20000, kind, zipf)], n, masks, tuned=(256, 7, 32768))       # an 80 KB LDS histogram
    three = (np.arange(n) % 3).astype(np.float64)                  # three bins per word: two combined rounds, then single adds
    check([Key(F.CODE, 2, 3, kind, three), Key(F.CODE, 2, 9000, kind, three)], n, masks)


@pytest.mark.parametrize("mode", ("code", "exact", "interval"))
def test_launch_shape_independence(hip, mode):
    n = 70001
    key = {"code": lambda: code_key(n, 100, 1), "exact": lambda: exact_key(n, 9000, 2), "interval": lambda: interval_key(n, 30, 3)}[mode]()
    masks = bitmaps_for(n, seed=8)[2:]
    base, _ = run([key], n, masks)
    assert np.array_equal(base[0, :key.n_bins + 2], key.want_counts(masks[0]))
    for threads in (64, 256, 1024):
        for blocks in (1, 7, 512):
            for lds in (0, 64, 8192, 32768):
                got, _ = run([key], n, masks, tuned=(threads, blocks, lds))
                assert np.array_equal(got, base), (threads, blocks, lds)


def test_bad_codes_land_in_unbinned(hip):
    for nb in (4, 20000):
        bad = np.array([-1.0, nb, 2.5, 1e300, np.nan, -np.inf, np.inf, -1e-300, 2.0 ** 31, 2.0 ** 63, -0.0, nb - 1])
        val = np.tile(bad, 11)
        n = len(val)
        got = check([Key(F.CODE, 2, nb, np.full(n, 2, np.uint8), val)], n)
        assert got[0, 0] == 11 and got[0, nb - 1] == 11 and got[0, nb] == 0 and got[0, nb + 1] == 10 * 11
    n = 1000                                                       # unsorted cuts: wrong counts are allowed, a wild access is not
    rs = np.random.RandomState(0)
    cuts = rs.randn(501)
    for mode, nb in ((F.EXACT, 501), (F.INTERVAL, 500)):
        got, _ = run([Key(mode, 1, nb, np.ones(n, np.uint8), rs.randn(n) * 2, cuts)], n)
        assert int(got.sum()) == n and (got >= 0).all()


def test_host_side_limits_name_the_field(hip):
    lib = hip.load()
    n = 100
    k = code_key(n, 5, 0)
    out = torch.full((64 * 16,), CANARY, dtype=torch.int32, device=DEV)

    def call(keys, n_rows=n, allow=None, allow_stride=0, nf=1, out_ptr=out.data_ptr(), out_stride=16, tuned=None, n_keys=None, keys_null=False):
        arr = (hip.FacetKeyC * max(1, len(keys)))()
        for a, d in zip(arr, keys):
            a.kind, a.val, a.cuts = d.get("kind", k.d_kind.data_ptr()), d.get("val", k.d_val.data_ptr()), d.get("cuts")
            a.mode, a.want_kind, a.n_bins, a.out_off = d.get("mode", 0), d.get("want", 2), d.get("nb", 5), d.get("off", 0)
        head = (None if keys_null else arr, len(keys) if n_keys is None else n_keys, n_rows, allow, allow_stride, nf, out_ptr, out_stride)
        rc = lib.arx_facet_count(*head, None) if tuned is None else lib.arx_facet_count_tuned(*head, *tuned, None)
        return rc, lib.arx_last_error()

    assert call([{}])[0] == 0
    for kw, part in ((dict(keys=[{}], n_keys=0), b"n_keys=0"), (dict(keys=[{}] * 17), b"n_keys=17"), (dict(keys=[{}], nf=0), b"n_filters=0"),
                     (dict(keys=[{}], nf=65), b"n_filters=65"), (dict(keys=[{"nb": 0}]), b"keys[0].n_bins=0"),
                     (dict(keys=[{"nb": (1 << 20) + 1}], out_stride=1 << 21), b"keys[0].n_bins=1048577"),
                     (dict(keys=[{}], n_rows=1 << 31), b"n_rows=2147483648"), (dict(keys=[{}], n_rows=-1), b"n_rows=-1"),
                     (dict(keys=[{"mode": 3}]), b"keys[0].mode=3"), (dict(keys=[{"mode": -1}]), b"keys[0].mode=-1"),
                     (dict(keys=[{"want": 0}]), b"keys[0].want_kind=0"), (dict(keys=[{"want": 4}]), b"keys[0].want_kind=4"),
                     (dict(keys=[{}, {"off": 6}]), b"keys[1].out_off=6 overlaps"), (dict(keys=[{"off": 3}, {"off": 0}]), b"keys[1].out_off=0"),
                     (dict(keys=[{"off": 10}]), b"keys[0].out_off=10"), (dict(keys=[{"off": -1}]), b"keys[0].out_off=-1"),
                     (dict(keys=[{}], nf=64, out_stride=(1 << 21) + 1), b"out_stride=2097153"), (dict(keys=[{}], out_stride=0), b"out_stride=0"),
                     (dict(keys=[{}], allow_stride=-1), b"allow_stride=-1"), (dict(keys=[{}], out_ptr=None), b"out"),
                     (dict(keys=[{}], keys_null=True), b"keys"), (dict(keys=[{"kind": None}]), b"keys[0].kind"),
                     (dict(keys=[{"val": None}]), b"keys[0].val"), (dict(keys=[{"mode": 1}]), b"keys[0].cuts"),
                     (dict(keys=[{"mode": 2}]), b"keys[0].cuts"),
                     (dict(keys=[{}], tuned=(100, 1, 0)), b"block_threads=100"), (dict(keys=[{}], tuned=(2048, 1, 0)), b"block_threads=2048"),
                     (dict(keys=[{}], tuned=(0, 1, 0)), b"block_threads=0"), (dict(keys=[{}], tuned=(256, 0, 0)), b"blocks_x=0"),
                     (dict(keys=[{}], tuned=(256, 1, -1)), b"lds_bins=-1"), (dict(keys=[{}], tuned=(256, 1, 32769)), b"lds_bins=32769")):
        keys = kw.pop("keys")
        rc, msg = call(keys, **kw)
        assert rc < 0 and part in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[16:] == CANARY).all() and host[:7].sum() == n     # only the one good call wrote, and only its slice
    with pytest.raises(hip.ArxError, match=r"n_bins=0"):
        F.launch([(k.d_kind, k.d_val, None, 0, 2, 0, 0)], n, None, 0, 1, out, 16)


# ---- HipCollection.facets against the oracle ------------------------------------------------------------------------------------------
N_ROWS, DIM = 5000, 64
WORDS = ["transformer", "graph", "lemma", "Lipschitz", "kernel", "résumé", "attention", "proof", "bound", "sparse", "dense", "token"]
KEYS = ["section", "paper_id", "year", "peer_reviewed", {"key": "quality_score", "edges": [0.8, 0.85, 0.9, 0.95, 1.0]},
        {"key": "quality_score", "kind": "number"}, "no_such_key", {"key": "section", "kind": "number"}]
_WORLD = {}


def corpus():
    if not _WORLD:
        rs = np.random.RandomState(4)
        meta = []
        for r in range(N_ROWS):
            m = {"chunk_id": f"c{r}", "paper_id": f"{r // 9:04d}.{r // 90:03d}", "text": " ".join(rs.choice(WORDS, size=rs.randint(2, 9))),
                 "section": ["Introduction", "Methods", "Results", "Résumé", "Appendix"][min(4, int(rs.zipf(1.7)) - 1)],
                 "quality_score": float(rs.choice([0.8, 0.85, 0.9, 0.95, 1.0, 0.7999, 1.0001, float("nan")])) if rs.rand() < 0.3
                 else float(np.round(rs.uniform(0.75, 1.0), 3))}
            if rs.rand() < 0.8:
                m["year"] = int(rs.randint(1995, 2024))
            if rs.rand() < 0.5:
                m["peer_reviewed"] = bool(rs.rand() < 0.3)
            if rs.rand() < 0.03:
                m["section"] = 7                                # another kind under a string key
            meta.append(m)
        emb = rs.randn(N_ROWS, DIM).astype(np.float32)
        emb /= np.linalg.norm(emb, axis=1, keepdims=True)
        emb[1000:1040] = emb[10:50]                              # exact duplicates for dedup_threshold
        _WORLD.update(meta=meta, emb=emb)
    return _WORLD["emb"], _WORLD["meta"]


def collection(**kw):
    from arxiv_rag_amd.store import HipCollection
    key = json.dumps(kw, sort_keys=True)
    if key not in _WORLD:
        emb, meta = corpus()
        _WORLD[key] = HipCollection(emb, meta, **kw)
    return _WORLD[key]


def host_mask(meta, where=None, contains=None, regex=None, keep=None):
    m = np.ones(len(meta), bool) if where is None else evaluate(compile_where(where), meta)
    if contains is not None:
        m = m & np.array([contains in (md.get("text") or "") for md in meta])
    if regex is not None:
        m = m & np.array([re.search(regex, md.get("text") or "") is not None for md in meta])
    return m if keep is None else m & keep


WHERE = {"$and": [{"quality_score": {"$gte": 0.9}}, {"section": {"$in": ["Methods", "Results", "Résumé"]}}]}


@pytest.mark.parametrize("top", (1, 10, None))
def test_collection_facets_against_the_oracle(hip, top):
    emb, meta = corpus()
    n = len(meta)
    plain, dev = collection(documents=True, document_regex=True), collection(documents=True, document_regex=True, where_on_device=True)
    cases = [(dict(), None), (dict(where=WHERE), host_mask(meta, WHERE)),
             (dict(where_document={"$contains": "transformer"}), host_mask(meta, contains="transformer")),
             (dict(where_document={"$regex": "gra(ph|de) lemma"}), host_mask(meta, regex="gra(ph|de) lemma")),
             (dict(where=WHERE, where_document={"$contains": "Lipschitz"}), host_mask(meta, WHERE, contains="Lipschitz")),
             (dict(where={"section": "no such section"}), np.zeros(n, bool))]
    for kw, mask in cases:
        want = F.oracle(meta, 0, n, KEYS, None if mask is None else [mask], top=top)[0]
        for coll in (plain, dev):
            got = coll.facets(KEYS, top=top, **kw)
            assert got == want, (kw, [(a, b) for a, b in zip(got, want) if a != b][:1])
    want = F.oracle(meta, 0, n, KEYS, None, top=top)[0]
    assert want[6] == {"key": "no_such_key", "values": [], "counts": [], "distinct": 0, "missing": n, "unbinned": 0, "total": n}
    assert want[4]["unbinned"] > 0 and all(c > 0 for c in want[4]["counts"]) and len(want[4]["values"]) == 4
    assert plain.facets("section", top=top) == want[:1]             # one spec alone is a list of one
    only_missing = plain.facets(["no_such_key"], where=WHERE)       # no key enters the kernel: the total is the bitmap's count
    assert only_missing[0]["total"] == only_missing[0]["missing"] == int(host_mask(meta, WHERE).sum())


def test_collection_facets_with_a_list_of_seventy_filters(hip):
    emb, meta = corpus()
    n = len(meta)
    wheres = [{"year": {"$gte": 1950 + j}} for j in range(70)]        # 68 distinct (where, where_document) pairs: two calls
    wheres[3], wheres[10], wheres[20] = wheres[2], None, None         # a repeated pair is evaluated once; no filter at all
    docs = [{"$contains": WORDS[j % len(WORDS)]} if j % 5 == 0 else None for j in range(70)]
    masks = [host_mask(meta, w, contains=None if d is None else d["$contains"]) for w, d in zip(wheres, docs)]
    want = F.oracle(meta, 0, n, KEYS[:5], masks, top=10)
    for coll in (collection(documents=True, document_regex=True), collection(documents=True, document_regex=True, where_on_device=True)):
        got = coll.facets(KEYS[:5], where=wheres, where_document=docs)
        assert len(got) == 70 and got == want


def test_collection_facets_with_dedup_threshold(hip):
    emb, meta = corpus()
    coll = collection(dedup_threshold=0.99)
    keep = coll._keep_mask
    assert keep is not None and 0 < int((~keep).sum()) <= 60
    for kw, mask in ((dict(), keep), (dict(where=WHERE), host_mask(meta, WHERE, keep=keep))):
        assert coll.facets(KEYS, top=None, **kw) == F.oracle(meta, 0, len(meta), KEYS, [mask], top=None)[0]


def test_collection_facets_after_delete_compact_and_add(hip):
    from arxiv_rag_amd.store import HipCollection
    emb, meta = corpus()
    n0 = 3000
    coll = HipCollection(emb[:n0], meta[:n0], capacity=N_ROWS, where_on_device=True)
    keys = KEYS[:6]
    assert coll.facets(keys, top=None) == F.oracle(meta, 0, n0, keys, None, top=None)[0]
    gone = coll.delete(ids=[f"c{r}" for r in range(100, 164)]) + coll.delete(where={"section": "Methods"})
    alive = ~(host_mask(meta[:n0], {"section": "Methods"}) | np.isin(np.arange(n0), np.arange(100, 164)))
    assert gone == int((~alive).sum()) > 64
    for kw, mask in ((dict(), alive), (dict(where={"year": {"$lt": 2010}}), host_mask(meta[:n0], {"year": {"$lt": 2010}}, keep=alive))):
        got = coll.facets(keys, top=None, **kw)
        assert got == F.oracle(meta, 0, n0, keys, [mask], top=None)[0]          # deleted rows are never counted
    before = coll.facets(keys, top=None)
    assert "Methods" not in before[0]["values"]
    coll.compact()
    survivors = [md for md, a in zip(meta[:n0], alive) if a]
    assert coll.facets(keys, top=None) == before == F.oracle(survivors, 0, len(survivors), keys, None, top=None)[0]
    coll.add(emb[n0:n0 + 500], meta[n0:n0 + 500])
    now = survivors + meta[n0:n0 + 500]
    after = coll.facets(keys, top=None)
    assert after == F.oracle(now, 0, len(now), keys, None, top=None)[0] and "Methods" in after[0]["values"]
    assert after[0]["total"] == len(now) == coll.count()


def test_collection_facets_refusals(hip):
    from arxiv_rag_amd.store import HipCollection
    emb, meta = corpus()
    coll = collection(documents=True, document_regex=True)
    for bad, part in (({"key": "section", "kind": "date"}, "kind='date'"), ({"key": "q", "edges": [1, 1]}, "ascend strictly"), (3, "key name")):
        with pytest.raises(ValueError, match=part):
            coll.facets(["section", bad])
    with pytest.raises(ValueError, match="top=0"):
        coll.facets(["section"], top=0)
    with pytest.raises(ValueError, match="documents=True"):
        collection().facets(["section"], where_document={"$contains": "x"})
    with pytest.raises(ValueError, match="world == 1"):
        HipCollection(emb[:128], meta[:128], rank=0, world=2).facets(["section"])


def test_cli_facets_end_to_end(hip, tmp_path, monkeypatch):
    """--facets writes a facets.json equal to the oracle's over the rows the run kept; without the flag no such file appears."""
    from arxiv_rag_amd import generate_embeddings_parallel as GEN
    from tests.helpers import make_chunk_tree
    from tests.test_gpu_cli import _minilm_model_dir
    cfg, sd, mdir, words = _minilm_model_dir(tmp_path)
    make_chunk_tree(tmp_path / "in", n_files=30, chunks_per_file=10, seed=2, words=words)
    (tmp_path / "queries.txt").write_text(" ".join(words[:6]) + "\n" + " ".join(words[6:12]) + "\n")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = [str(tmp_path / "in"), "--model", "all-MiniLM-L6-v2", "--model-dir", str(tmp_path / "models"), "--batch-size", "32",
              "--min-quality", "0.9", "--skip-chroma", "--queries", str(tmp_path / "queries.txt")]
    where = {"section": {"$in": ["Methods", "Results"]}}
    out = tmp_path / "embeddings_saved"
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--where", json.dumps(where)]) == 0
    assert not (out / "facets.json").exists()
    plain_results = (out / "search_results.json").read_bytes()
    GEN._model, GEN._model_name = None, None
    assert GEN.main(common + ["--where", json.dumps(where), "--facets", "section,paper_id", "--facets-top", "5"]) == 0
    assert (out / "search_results.json").read_bytes() == plain_results
    meta = json.loads((out / "metadata.json").read_text())
    rows = [{k: m.get(k) for k in ("paper_id", "section", "quality_score")} for m in meta]
    got = json.loads((out / "facets.json").read_text())
    want = F.oracle(rows, 0, len(rows), ["section", "paper_id"], [host_mask(rows, where)], top=5)[0]
    assert got == {"keys": ["section", "paper_id"], "top": 5, "facets": want}
    assert want[0]["values"] and set(want[0]["values"]) <= {"Methods", "Results"} and len(want[1]["values"]) == 5
