"""float64 reference of topic clustering (INTEGRATION.md "Topics"), written independently of arxiv_rag_amd/topics.py: boolean masks and
plain float64 sums, no member lists, no runs.  Spherical k-means: a row goes to the centroid with the largest dot product (ties to the
lower centroid), a centroid becomes the normalised sum of its members, an empty cluster keeps its centroid; the centroids the assign
sees are rounded to fp16, as the device's are."""
import math

import numpy as np

U = 2.0 ** -24                                                 # unit roundoff of f32


def cluster_sums(X, labels, n_clusters):
    """(S float64 [C, dim], A float64 [C, dim]): the sum of every cluster's rows and the sum of their absolute values."""
    X64 = np.asarray(X, dtype=np.float64)
    S = np.zeros((n_clusters, X64.shape[1]))
    A = np.zeros_like(S)
    for c in range(n_clusters):
        m = np.asarray(labels) == c
        S[c], A[c] = X64[m].sum(axis=0), np.abs(X64[m]).sum(axis=0)
    return S, A


def gamma(k):
    return k * U / (1.0 - k * U)


def sum_bound(m):
    """gamma_k of the two-level sequential f32 sum of m terms in runs of 256: k = 256 + ceil(m / 256) (each term passes through at
    most 255 adds inside its run and ceil(m / 256) adds over the partials)."""
    return gamma(256 + math.ceil(m / 256))


def normalise(S):
    """float64 rows S / |S| (rows of norm 0 are returned as they are)."""
    S = np.asarray(S, dtype=np.float64)
    n = np.sqrt((S * S).sum(axis=1))
    return S / np.where(n > 0, n, 1.0)[:, None]


def assign(X, centroids_f16):
    """(labels, best score, best minus second-best score) in float64; ties to the lower centroid."""
    sc = np.asarray(X, dtype=np.float64) @ np.asarray(centroids_f16, dtype=np.float64).T
    labels = np.argmax(sc, axis=1)
    best = sc[np.arange(len(sc)), labels]
    if sc.shape[1] > 1:
        rest = sc.copy()
        rest[np.arange(len(sc)), labels] = -np.inf
        margin = best - rest.max(axis=1)
    else:
        margin = np.full(len(sc), np.inf)
    return labels, best, margin


def lloyd(X, init, iters):
    """float64 Lloyd from `init` (f32 [C, dim]); the centroids are rounded to fp16 before every assign.  -> a list with one entry per
    assign, {labels, sizes, objective, margin (min over rows), centroids (float64, before the rounding)}; it stops as the device loop
    does: after `iters` assigns or once an assign changes no label."""
    X = np.asarray(X)
    C = init.shape[0]
    cent = np.asarray(init, dtype=np.float64)
    prev = np.full(X.shape[0], -1)
    out = []
    for it in range(iters):
        labels, best, margin = assign(X, cent.astype(np.float16))
        sizes = np.bincount(labels, minlength=C)
        out.append({"labels": labels, "sizes": sizes, "objective": float(best.mean()), "margin": float(margin.min()), "centroids": cent})
        if (labels != prev).sum() == 0 or it == iters - 1:
            break
        S, _ = cluster_sums(X, labels, C)
        norm = np.sqrt((S * S).sum(axis=1))
        keep = (sizes == 0) | ~(norm > 0)
        cent = np.where(keep[:, None], cent, S / np.where(keep, 1.0, norm)[:, None])
        prev = labels
    return out


def planted(n, dim, n_centres, noise, seed):
    """Unit fp16 rows around `n_centres` random orthonormal centres: centre + gaussian noise of relative norm `noise`, normalised.
    -> (X fp16 [n, dim], planted label of every row, centres float64)."""
    rs = np.random.RandomState(seed)
    centres, _ = np.linalg.qr(rs.randn(dim, n_centres))
    centres = centres.T
    which = rs.randint(0, n_centres, n)
    g = rs.randn(n, dim)
    g *= noise / np.linalg.norm(g, axis=1, keepdims=True)
    x = centres[which] + g
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16), which, centres
