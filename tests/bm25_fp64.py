"""float64 reference of the keyword side of hybrid search, written independently of arxiv_rag_amd/keyword.py: plain dictionaries of
lists, no CSR, no vectorisation.  Definition (hybrid search): Lucene BM25 with k1 = 1.2, b = 0.75,
idf(t) = ln(1 + (N - df + 0.5) / (df + 0.5)), w(t, d) = idf * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl)); a query is its
distinct terms; top-n by (score desc, row asc) over rows holding a query term; relative-score fusion of two lists."""
import math

import numpy as np

K1, B = 1.2, 0.75
U24 = 2.0 ** -24


def statistics(docs, vocab_size):
    """docs: list of term-id lists -> (N, df list [V], total_len)."""
    df = [0] * vocab_size
    total = 0
    for d in docs:
        total += len(d)
        for t in set(d):
            df[t] += 1
    return len(docs), df, total


def idf(N, df_t):
    return math.log(1.0 + (N - df_t + 0.5) / (df_t + 0.5))


def postings(docs):
    """-> {term: [(row, tf), ...] rows ascending}."""
    post = {}
    for r, d in enumerate(docs):
        tf = {}
        for t in d:
            tf[t] = tf.get(t, 0) + 1
        for t, c in tf.items():
            post.setdefault(t, []).append((r, c))
    return post


def impact(N, df_t, avgdl, tf, dl):
    return idf(N, df_t) * tf * (K1 + 1.0) / (tf + K1 * (1.0 - B + B * dl / avgdl))


def impacts(docs, vocab_size, stats=None, fault=None):
    """-> {term: {row: float64 impact}} with the statistics `stats` (N, df, total_len; default: of `docs`).
    fault: None | "no_tf" (tf taken as 1) | "dl_neighbour" (dl of the next row, cyclically)."""
    N, df, total = stats if stats is not None else statistics(docs, vocab_size)
    avgdl = total / N
    out = {}
    for t, pl in postings(docs).items():
        row = {}
        for r, tf in pl:
            dl = len(docs[(r + 1) % len(docs)]) if fault == "dl_neighbour" else len(docs[r])
            row[r] = impact(N, df[t], avgdl, 1 if fault == "no_tf" else tf, dl)
        out[t] = row
    return out


def stored_f32(imp):
    """the impacts as the index stores them: rounded once to f32 (returned as float64 values)."""
    return {t: {r: float(np.float32(w)) for r, w in row.items()} for t, row in imp.items()}


def scores(imp, terms, n_rows):
    """float64 score of every row for the query's distinct terms: (scores [n_rows], has_term bool [n_rows])."""
    s = np.zeros(n_rows, np.float64)
    has = np.zeros(n_rows, bool)
    for t in sorted(set(terms)):
        for r, w in imp.get(t, {}).items():
            s[r] += w
            has[r] = True
    return s, has


def topn(s, has, n, idx_base=0):
    """-> (scores float64 [n], ids int64 [n]) by (score desc, row asc) over the candidate rows; unused slots (-inf, -1)."""
    cand = sorted((r for r in range(len(s)) if has[r]), key=lambda r: (-s[r], r))[:n]
    out_s = np.full(n, -np.inf); out_i = np.full(n, -1, np.int64)
    for j, r in enumerate(cand):
        out_s[j], out_i[j] = s[r], r + idx_base
    return out_s, out_i


def fuse(dense, keyword, alpha, k):
    """dense / keyword: lists of (score, row) -> [(fused, row)] of the best k by (fused desc, row asc)."""
    def norm(lst):
        if not lst:
            return {}
        lo, hi = min(s for s, _ in lst), max(s for s, _ in lst)
        return {r: (1.0 if hi == lo else (float(s) - float(lo)) / (float(hi) - float(lo))) for s, r in lst}
    nd, nk = norm(dense), norm(keyword)
    fused = [(alpha * nd.get(r, 0.0) + (1.0 - alpha) * nk.get(r, 0.0), r) for r in set(nd) | set(nk)]
    fused.sort(key=lambda fr: (-fr[0], fr[1]))
    return fused[:k]


def query_terms(pieces, exclude=()):
    """distinct ids, the first 64 in order of appearance, ascending."""
    out = []
    for t in pieces:
        if t not in out and t not in exclude:
            out.append(t)
        if len(out) == 64:
            break
    return sorted(out)


def zipf_corpus(n_docs, vocab_size, mean_len, seed, empty_every=0):
    """Seeded corpus of term-id lists with Zipf-distributed terms (repeats included); every `empty_every`-th document is empty."""
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, vocab_size + 1) ** 1.1
    p /= p.sum()
    perm = rs.permutation(vocab_size)
    docs = []
    for d in range(n_docs):
        if empty_every and d % empty_every == empty_every - 1:
            docs.append([])
            continue
        ln = max(1, int(rs.poisson(mean_len)))
        docs.append(perm[rs.choice(vocab_size, size=ln, p=p)].tolist())
    return docs
