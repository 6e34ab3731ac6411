"""The edges that the candidate scans' one host driver decides (csrc/key_lists.h `key_scan`), for both families against their numpy
restatements (-m gpu): an empty shard (no scan is launched; the merge of no parts writes -1 and 0), one row and 65 rows at the smallest
and the default rows_per_block, a second slice of queries over 65 parts, and what each library call answers to no queries at all (the
one place the families differ on purpose).  dim 64 throughout (PQ: dsub 8, M = 8): the driver's arithmetic does not see the code width.
The library is called directly, with every output filled beforehand, so that what a call leaves unwritten shows."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import _lib
from arxiv_rag_amd import binary as B
from arxiv_rag_amd import pq as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIM, DSUB, M = 64, 8, 8
N, NQ = 4160, 257                                               # 65 parts of 64 rows; a slice of 256 queries and one of 1
FILL = 7                                                        # no row, distance, sum or count of these cases is 7 where it matters
FAMILIES = ("binary", "pq")

_DATA = {}


def data(family):
    """The family's code array and query-side data (every bit pattern is a legal value), on both sides, and the host answer at R = 256:
    the lists of a smaller R are its prefixes."""
    if family not in _DATA:
        rs = np.random.RandomState(len(family))
        if family == "binary":
            codes = rs.randint(0, 1 << 62, size=(N, 1)).astype(np.uint64) << np.uint64(2) | rs.randint(0, 4, size=(N, 1)).astype(np.uint64)
            qdata = rs.randint(0, 1 << 62, size=(NQ, 1)).astype(np.uint64) << np.uint64(2) | rs.randint(0, 4, size=(NQ, 1)).astype(np.uint64)
            dcodes, dq = torch.from_numpy(codes.view(np.int64)).to(DEV), torch.from_numpy(qdata.view(np.int64)).to(DEV)
        else:
            codes = rs.randint(0, 256, size=(N, M)).astype(np.uint8)
            qdata = rs.randint(0, 256, size=(NQ, M, P.N_CODES)).astype(np.uint8)
            dcodes, dq = torch.from_numpy(codes).to(DEV), torch.from_numpy(qdata).to(DEV)
        _DATA[family] = dict(codes=codes, qdata=qdata, dcodes=dcodes, dq=dq, host={})
    return _DATA[family]


def host(family, n, nq, R):
    d = data(family)
    if n not in d["host"]:
        f = B.candidates_host if family == "binary" else P.candidates_host
        d["host"][n] = f(d["codes"][:n], d["qdata"], 256)
    cand, hi, count = d["host"][n]
    return cand[:nq, :R], hi[:nq, :R], np.minimum(count[:nq], R)


def call(family, n, nq, R, rpb, with_hi=True, n_out=None):
    """(rc, message, cand, hi or None, count): `arx_<family>_candidates_tuned` over the first n rows and nq queries."""
    lib, d = _lib.load(), data(family)
    n_out = nq if n_out is None else n_out
    cand = torch.full((n_out, R), FILL, dtype=torch.int32, device=DEV)
    hi = torch.full((n_out, R), FILL, dtype=torch.int32, device=DEV) if with_hi else None
    count = torch.full((n_out,), FILL, dtype=torch.int64, device=DEV)
    size = (lib.arx_binary_workspace_bytes(n, max(nq, 1), DIM, R) if family == "binary"
            else lib.arx_pq_workspace_bytes(n, max(nq, 1), DIM, DSUB, R))
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    codes_p = d["dcodes"].data_ptr() if n else None
    tail = (nq, None, R, cand.data_ptr(), hi.data_ptr() if with_hi else None, count.data_ptr(), ws.data_ptr(), ws.numel(), rpb, None)
    if family == "binary":
        rc = lib.arx_binary_candidates_tuned(codes_p, n, DIM, d["dq"].data_ptr(), *tail)
    else:
        rc = lib.arx_pq_candidates_tuned(codes_p, n, DIM, DSUB, d["dq"].data_ptr(), *tail)
    msg = lib.arx_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg, cand.cpu().numpy(), hi.cpu().numpy() if with_hi else None, count.cpu().numpy()


@pytest.mark.parametrize("family", FAMILIES)
def test_an_empty_shard_gives_no_candidates(family):
    for nq in (1, 9):
        for R in (1, 256):
            for with_hi in (True, False):
                for rpb in (0, 64):
                    rc, msg, cand, hi, count = call(family, 0, nq, R, rpb, with_hi)
                    assert rc == 0, msg
                    assert (cand == -1).all() and (count == 0).all() and (hi is None or (hi == -1).all()), (nq, R, with_hi, rpb)


@pytest.mark.parametrize("n", (1, 65))
@pytest.mark.parametrize("family", FAMILIES)
def test_one_row_and_one_row_past_a_wave(family, n):
    for rpb in (64, 0):
        for R in (1, 256):
            for with_hi in (True, False):
                rc, msg, cand, hi, count = call(family, n, 9, R, rpb, with_hi)
                wc, wh, wn = host(family, n, 9, R)
                assert rc == 0, msg
                assert np.array_equal(cand, wc) and np.array_equal(count, wn) and (hi is None or np.array_equal(hi, wh)), (rpb, R, with_hi)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_second_slice_of_queries_over_65_parts(family):
    """257 queries at rows_per_block = 64: 65 parts x 256 queries = 16 640 lists, inside the 2^15 the workspace holds, so rows_per_block
    stays 64 in both slices; the second slice is one query with its own offsets into the query-side data and the outputs."""
    for R in (10, 256):
        rc, msg, cand, hi, count = call(family, N, NQ, R, 64)
        wc, wh, wn = host(family, N, NQ, R)
        assert rc == 0, msg
        assert np.array_equal(cand, wc) and np.array_equal(hi, wh) and np.array_equal(count, wn), R


def test_no_queries_binary_refuses_and_pq_writes_nothing():
    rc, msg, cand, hi, count = call("binary", N, 0, 10, 0, n_out=1)
    assert rc != 0 and "n_queries" in msg and "empty query set" in msg
    assert (cand == FILL).all() and (hi == FILL).all() and (count == FILL).all()
    rc, msg, cand, hi, count = call("pq", N, 0, 10, 0, n_out=1)
    assert rc == 0, msg
    assert (cand == FILL).all() and (hi == FILL).all() and (count == FILL).all()
