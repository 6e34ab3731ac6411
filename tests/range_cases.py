"""What the score-threshold search's GPU tests share (tests/test_gpu_range_search.py): the masks, the reference list of a query built
by peeling the repository's own filtered search, the thresholds derived from it, and the checks of an answer against that list and
against float64."""
import numpy as np

from tests.helpers import pass_b_budget

MASKS = ("none", "ones", "half", "percent", "zeros", "one_row", "stray")


def make_mask(kind, n, seed):
    """-> the bitmap's words as numpy uint64 [ceil(n / 64)] (None for "none").  "stray": a random half with every bit beyond n set."""
    if kind == "none":
        return None
    n_words = (n + 63) // 64
    rs = np.random.RandomState(seed)
    if kind == "ones":
        on = np.ones(n, bool)
    elif kind in ("half", "stray"):
        on = rs.rand(n) < 0.5
    elif kind == "percent":
        on = rs.rand(n) < 0.01
    elif kind == "zeros":
        on = np.zeros(n, bool)
    else:
        on = np.zeros(n, bool)
        on[rs.randint(n)] = True
    bits = np.zeros(n_words * 64, bool)
    bits[:n] = on
    if kind == "stray":
        bits[n:] = True
    return np.packbits(bits.reshape(n_words, 64), axis=1, bitorder="little").view(np.uint64).reshape(n_words)


def visible_rows(words, n):
    """bool [n]: the rows a bitmap lets a query see (None: all)."""
    if words is None:
        return np.ones(n, bool)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def to_device(words):
    import torch
    return None if words is None else torch.from_numpy(words.view(np.int64).copy()).cuda()


def peel(idx, q1, words, n, need, base):
    """The best `need` visible rows of ONE query (fp16 [1, D] on the device) by the search's own order and score bits: search(q, 32,
    allow=bitmap), clear the returned rows from the bitmap, repeat until `need` rows are seen or the bitmap runs dry.
    -> (scores f32 [m], local rows int64 [m]), m <= need."""
    import torch
    n_words = (n + 63) // 64
    bits = np.full(n_words, ~np.uint64(0), np.uint64) if words is None else words.copy()
    scores, rows = [], []
    while len(rows) < need:
        s, i = idx.search(q1, 32, allow=torch.from_numpy(bits.view(np.int64)).cuda())
        s, i = s[0].cpu().numpy(), i[0].cpu().numpy()
        got = i >= 0
        if not got.any():
            break
        r = i[got] - base
        scores.extend(s[got].tolist()); rows.extend(r.tolist())
        for rr in r:                                                            # (one by one: several of the rows may share a word)
            bits[rr >> 6] &= ~(np.uint64(1) << np.uint64(rr & 63))
        if got.sum() < 32:
            break
    return np.asarray(scores[:need], np.float32), np.asarray(rows[:need], np.int64)


KINDS = ("own_mid", "above_mid", "own_last", "above_last", "-inf", "nan", "+inf")


def threshold_of(kind, ref_scores, M):
    """A threshold of one kind for a query whose reference list (the best <= M + 1 rows) has the scores `ref_scores`: the bits of its
    own j-th best score (the row is included: >=) or the next float above them (the row and its bit-equal ties are excluded), with j
    in the middle of the list or at its M-th row (near-ties then straddle the cut)."""
    if kind == "-inf" or (len(ref_scores) == 0 and kind not in ("nan", "+inf")):
        return np.float32(-np.inf)
    if kind == "nan":
        return np.float32(np.nan)
    if kind == "+inf":
        return np.float32(np.inf)
    j = (min(len(ref_scores), M) - 1) // 2 if kind.endswith("mid") else min(len(ref_scores), M) - 1
    v = np.float32(ref_scores[j])
    return v if kind.startswith("own") else np.nextafter(v, np.float32(np.inf), dtype=np.float32)


def expected(ref_scores, ref_rows, ms, M, base):
    """The range answer the reference list implies: its prefix cut at the threshold and at M, padded; count = qualifying among the
    M + 1.  -> (scores f32 [M], ids int64 [M], count)."""
    qual = int((ref_scores >= ms).sum()) if len(ref_scores) else 0             # (NaN: none; the list is sorted, so these are a prefix)
    assert qual == 0 or (ref_scores[:qual] >= ms).all()
    m = min(qual, M)
    s = np.full(M, -np.inf, np.float32); i = np.full(M, -1, np.int64)
    s[:m], i[:m] = ref_scores[:m], ref_rows[:m] + base
    return s, i, min(qual, M + 1)


def check_range_fp64(c, q, e, words, ms, M, s, i, counts, base, what):
    """(s, i, counts) = search_range(q, ms, M) over the fp16 rows `c` with the bitmap `words` (numpy, None = every row); e = q.c in
    float64 (device).  Per query, with B = B(D) |q| |c| the bound of check_topk_fp64:
      - the list is min(count, M) rows followed by (-inf, -1) padding; ids distinct, visible, inside the shard; every returned score is
        >= the threshold in f32, scores non-increasing and bit-equal scores in ascending id order; count <= M + 1;
      - every returned row is within B of its fp64 score;
      - not truncated: no unreturned visible row has an fp64 score above min_score + B;
      - truncated: no unreturned visible row has an fp64 score above the smallest returned score + 2 B (B at the largest row norm)."""
    import torch
    n, D = c.shape
    nq = q.shape[0]
    assert s.shape == (nq, M) and i.shape == (nq, M) and counts.shape == (nq,), what
    B = pass_b_budget(D) * (1 + 1e-3)
    qn = q.double().norm(dim=1)
    cn = c.double().norm(dim=1)
    vis = torch.from_numpy(visible_rows(words, n)).cuda()
    ms_t = torch.from_numpy(np.asarray(ms, np.float32)).cuda()
    cnt = counts.long()
    assert ((cnt >= 0) & (cnt <= M + 1)).all(), (what, "count out of range")
    m = cnt.clamp(max=M)
    col = torch.arange(M, device="cuda")[None, :]
    held = col < m[:, None]
    assert ((i >= 0) == held).all() and (s[~held] == float("-inf")).all() and (i[~held] == -1).all(), (what, "padding / count")
    assert (m <= int(vis.sum())).all(), what
    none = ~(ms_t < float("inf"))
    assert (cnt[none] == 0).all(), (what, "+inf / NaN threshold")
    ids = (i - base).clamp(min=0)
    assert (ids[held] < n).all() and vis[ids[held]].all(), (what, "ids out of range or masked")
    srt = torch.where(held, ids, -1 - col.expand_as(ids)).sort(dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), (what, "duplicate ids")
    assert (s >= ms_t[:, None])[held].all(), (what, "a returned row below the threshold")
    both = held[:, 1:]
    assert (s[:, :-1] >= s[:, 1:])[both].all(), (what, "order")
    eq = (s[:, :-1] == s[:, 1:]) & both
    assert (ids[:, :-1][eq] < ids[:, 1:][eq]).all(), (what, "tie order")
    ej = e.gather(1, ids)
    bj = B * qn[:, None] * cn[ids]
    assert ((s.double() - ej).abs() <= bj)[held].all(), (what, "score outside B(D)")
    # the rows left out: visible and not returned
    ret = torch.zeros((nq, n + 1), dtype=torch.bool, device="cuda")
    ret.scatter_(1, torch.where(held, ids, n), True)
    left = e.clone()
    left[ret[:, :n] | ~vis[None, :]] = float("-inf")
    full = cnt <= M
    live = full & ~none
    worst = (left - B * qn[:, None] * cn[None, :]).max(dim=1).values
    assert (worst[live] <= ms_t.double()[live]).all(), (what, "complete list: a row left out is above min_score + B")
    trunc = ~full
    if trunc.any():
        slack = left[trunc].max(dim=1).values - (s[trunc, M - 1].double() + 2 * B * qn[trunc] * cn.max())
        assert (slack <= 0).all(), (what, "truncated list: a row left out is above the smallest returned score + 2 B", slack.max().item())
