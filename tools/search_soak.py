#!/usr/bin/env python3
"""Race / edge screen of the search path (the counterpart of tools/gemm_soak.py): random shard sizes (1 row ... a few hundred thousand, ragged
against every tile size), dimensions, query-batch sizes (1 ... 1 100: narrow tiles, the persistent pass, two internal passes), k, first pass
(fp16 / int8), row norms (unit / 0.01 ... 8), a component shared by all rows (anisotropic embeddings), planted near-ties and duplicated rows, idx_base; every answer validated ON THE DEVICE against
float64 scores of EVERY row with the certificate's own rounding budgets (tests/helpers.py check_topk_fp64: returned scores within the
pass-B budget of those rows' scores; nothing left out beats the k-th by more than the budgets allow; equal scores in ascending id order), run twice (bit-repeatable), and — batches of <= 1 024 queries — against `search_many` (2 lanes).
usage: search_soak.py [seconds] [seed]"""
import json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from arxiv_rag_amd import _lib
from arxiv_rag_amd.index import ShardIndex
from tests.helpers import check_topk_fp64

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
LOG = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
g = torch.Generator(device="cuda"); g.manual_seed(seed)
gc = torch.Generator(); gc.manual_seed(seed)


def ri(lo, hi):
    return int(torch.randint(lo, hi + 1, (1,), generator=gc).item())


def validate(c, q, s, i, k, base, what):
    # float64 scores of every row, checked with the certificate's own budgets (tests/helpers.py check_topk_fp64: the pass-B error of each
    # returned score, completeness, order, ids, padding), so the tolerance grows with D as the library's does
    check_topk_fp64(c, q, s, i, k, idx_base=base, sample_rows=0, what=what)


t0 = time.time(); cases = 0; stats = {"fp16": 0, "int8": 0, "many": 0, "flagged": 0}
while time.time() - t0 < secs:
    d = [64, 128, 192, 256, 320, 384, 768, 1024, 1536, 4096][ri(0, 9)]
    shape = ri(0, 9)
    n = ri(1, 70) if shape == 0 else (ri(64 * 3, 64 * 40) if shape < 4 else ri(20_000, 300_000 if d <= 256 else (120_000 if d <= 1024 else 30_000)))
    if shape == 9:
        n = 256 * ri(4, 300) + [0, 1, 63, 64, 255][ri(0, 4)]
    big = ri(0, 39) == 0                                             # now and then a shard beyond 1 M rows: the select kernel's lists feed the tails
    if big:
        d = [64, 128][ri(0, 1)]; n = ri(1_000_000, 2_600_000)
    nq = [1, ri(2, 64), ri(65, 128), ri(129, 256), ri(257, 1100)][min(4, ri(0, 5))]
    if big:
        nq = min(nq, 300)                                            # (the validator's score matrix is nq x n floats)
    k = [1, 5, 10, 10, 10, 11, 16, 31, 32][ri(0, 8)]
    base = [0, 7, 1 << 33][ri(0, 2)]
    c = torch.nn.functional.normalize(torch.randn((n, d), generator=g, device="cuda"), dim=1)
    q = torch.nn.functional.normalize(torch.randn((nq, d), generator=g, device="cuda"), dim=1)
    if ri(0, 3) == 0:                                                # a common component (anisotropic embeddings; the int8 index is centred on the shard's mean)
        u = torch.nn.functional.normalize(torch.randn((1, d), generator=g, device="cuda"), dim=1) * [0.2, 0.6, 1.5, -0.8][ri(0, 3)]
        c = torch.nn.functional.normalize(c + u, dim=1)
        q = torch.nn.functional.normalize(q + (u if ri(0, 1) else 0.3 * u), dim=1)
    scale = 1.0
    if ri(0, 3) == 0:                                                # rows far from unit norm
        nr = torch.exp(torch.empty(n, device="cuda").uniform_(-4.6, 2.08, generator=g)); c = c * nr[:, None]; scale = float(nr.max().item())
    flavour = ri(0, 5)
    if flavour == 0 and n > 200:                                     # near-ties planted across many groups for query 0
        rows = torch.randperm(n, generator=g, device="cuda")[:min(n, 60)]
        c[rows] = (q[0] * 0.9 + 1e-4 * torch.randn((len(rows), d), generator=g, device="cuda")) * (scale if scale != 1.0 else 1.0)
    elif flavour == 1 and n > 10:                                    # exact duplicates
        rows = torch.randperm(n, generator=g, device="cuda")[:min(n, 300)]; c[rows] = c[rows[0]].clone()
    elif flavour == 2 and n > 64:                                    # a run of neighbours inside one group
        c[64:64 + min(40, n - 64)] = q[min(1, nq - 1)] * 0.8 + 0.02 * torch.randn((min(40, n - 64), d), generator=g, device="cuda")
    c16, q16 = c.to(torch.float16).contiguous(), q.to(torch.float16).contiguous()
    if LOG is not None:                                                # the case about to run, on disk before any kernel of it is launched
        LOG.write(json.dumps(dict(case=cases, n=n, d=d, nq=nq, k=k, base=base, flavour=flavour, scale=round(scale, 3))) + "\n"); LOG.flush()
    for pre in (None, "int8"):
        if pre == "int8" and (d % 128 != 0 or d > 1024 or n >= (1 << 32)):
            continue
        idx = ShardIndex(c16, idx_base=base, prefilter=pre, centre_query=[None, None, True, False][ri(0, 3)])      # (int8: the query centred as well, or not, or the index's own choice)
        s, i = idx.search(q16, k)
        what = dict(n=n, d=d, nq=nq, k=k, pre=pre, base=base, flavour=flavour, scale=round(scale, 3), seed=seed, case=cases)
        validate(c16, q16, s, i, k, base, what)
        s2, i2 = idx.search(q16, k)
        assert torch.equal(i, i2) and torch.equal(s, s2), (what, "not repeatable")
        stats["flagged"] += idx.certificate_stats()[0] if pre is None else 0
        if nq <= 1024 and nq >= 4:
            cut = [0, nq // 3, 2 * nq // 3, nq]
            got = idx.search_many([q16[cut[j]:cut[j + 1]] for j in range(3) if cut[j + 1] > cut[j]], k)
            assert torch.equal(torch.cat([x[1] for x in got]), i) and torch.equal(torch.cat([x[0] for x in got]), s), (what, "search_many")
            stats["many"] += 1
        stats["fp16" if pre is None else "int8"] += 1
    cases += 1
    if cases % 50 == 0:
        print(json.dumps({"cases": cases, "seconds": round(time.time() - t0, 1), **stats}), flush=True)
torch.cuda.synchronize()
print(json.dumps({"done": True, "cases": cases, "seconds": round(time.time() - t0, 1), **stats, "seed": seed}))
