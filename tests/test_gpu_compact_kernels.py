"""arx_compact_plan / arx_compact_rows / arx_compact_text (csrc/compact.hip) against numpy: every row count at which the block scans
change shape, every keep pattern, every row size that takes another copy path.  The output buffers are pre-filled with a sentinel:
what the kernels must write equals numpy's, and every byte beyond keeps the sentinel.  No test feeds out-of-range offsets to the
device; the clamping of arx_compact_text is checked by reading csrc/compact.hip."""
import numpy as np
import pytest
import torch

from arxiv_rag_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ROWS = (1, 63, 64, 65, 257, 4099, 70001)                     # 70 001 rows = 1 094 words: the plan's block scan crosses 5 blocks, the text's 274
SENTINEL = 0xA5


def keep_patterns(n, rs):
    """name -> (mask bool [n], words uint64 [ceil(n / 64)])."""
    from arxiv_rag_amd.where import pack_bitmap
    masks = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
             "alternating": np.arange(n) % 2 == 0, "random": rs.rand(n) < 0.5,
             "zero_words": ((np.arange(n) // 64) % 3 == 0) & (rs.rand(n) < 0.7), "garbage_tail": rs.rand(n) < 0.5}
    out = {}
    for name, m in masks.items():
        words = pack_bitmap(m).copy()
        if name == "garbage_tail" and n % 64:
            words[-1] |= np.uint64(rs.randint(1, 1 << 62)) << np.uint64(n % 64)      # bits at or beyond n_rows: ignored
        out[name] = (m, words)
    return out


def guard(fill):
    return int.from_bytes(bytes([fill]) * 8, "little", signed=True)


def plan(words_d, n, fill=SENTINEL):
    lib = _lib.load()
    n_words = (n + 63) // 64
    rank = torch.full((n_words + 1 + 8,), guard(fill), dtype=torch.int64, device=DEV)     # 8 guard entries behind
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    _lib.check(lib.arx_compact_plan(words_d.data_ptr(), n, rank.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "arx_compact_plan")
    return rank, count


def upload_words(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).to(DEV) if len(words) else torch.zeros(1, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("n", N_ROWS)
def test_plan_equals_numpy_cumsum(n):
    rs = np.random.RandomState(n)
    for name, (mask, words) in keep_patterns(n, rs).items():
        per_word = np.add.reduceat(mask.astype(np.int64), np.arange(0, n, 64))
        want = np.concatenate([[0], np.cumsum(per_word)])
        for fill in (SENTINEL, 0x00):                           # the result does not depend on what the buffers held
            rank, count = plan(upload_words(words), n, fill)
            got = rank.cpu().numpy()
            assert np.array_equal(got[:len(want)], want), (n, name)
            assert (got[len(want):] == guard(fill)).all(), (n, name)
            assert count.tolist() == [int(mask.sum()), -7], (n, name)


def test_plan_of_no_rows():
    rank, count = plan(torch.zeros(1, dtype=torch.int64, device=DEV), 0)
    assert rank[0].item() == 0 and count.tolist() == [0, -7] and rank[1].item() != 0


@pytest.mark.parametrize("row_bytes,src_shift", [(1, 0), (4, 0), (8, 0), (6, 0), (128, 0), (1536, 0), (1536, 2)])
def test_rows_equal_numpy_and_nothing_else_is_written(row_bytes, src_shift):
    """`src_shift=2`: src starts 2 bytes behind a 16-byte boundary, which forces the byte path on rows that would take 16-byte units."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for n in N_ROWS:
        rs = np.random.RandomState(n + row_bytes)
        src = rs.randint(0, 256, size=(n, row_bytes), dtype=np.uint8)
        src[src == SENTINEL] = 0                                 # a copied byte is never mistaken for an untouched one
        holder = torch.zeros(n * row_bytes + 16, dtype=torch.uint8, device=DEV)
        src_d = holder[src_shift:src_shift + n * row_bytes]
        src_d.copy_(torch.from_numpy(src.reshape(-1)).to(DEV))
        assert src_d.data_ptr() % 16 == src_shift
        for name, (mask, words) in keep_patterns(n, rs).items():
            words_d = upload_words(words)
            rank, count = plan(words_d, n)
            want = src[mask]
            outs = []
            for fill in (SENTINEL, 0x5A) if name == "random" else (SENTINEL,):
                dst = torch.full((n * row_bytes + 64,), fill, dtype=torch.uint8, device=DEV)
                _lib.check(lib.arx_compact_rows(src_d.data_ptr(), dst.data_ptr(), row_bytes, n, words_d.data_ptr(), rank.data_ptr(), st),
                           "arx_compact_rows")
                got = dst.cpu().numpy()
                assert np.array_equal(got[:want.size].reshape(-1, row_bytes), want), (n, name, row_bytes)
                assert (got[want.size:] == fill).all(), (n, name, row_bytes)
                outs.append(got[:want.size])
            assert all(np.array_equal(outs[0], o) for o in outs)
            assert count[0].item() == len(want)


def text_rows(n, rs):
    """Rows of 0, 1, 15, 16, 17 and about 2 000 bytes, mixed: row starts fall on every residue mod 16."""
    lens = rs.choice([0, 1, 15, 16, 17, 2000], size=n, p=[0.2, 0.15, 0.15, 0.15, 0.15, 0.2])
    lens = np.where(lens == 2000, lens + rs.randint(-40, 40, size=n), lens).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    blob = rs.randint(0, 256, size=int(off[-1]), dtype=np.uint8)
    blob[blob == SENTINEL] = 1
    return blob, off


def run_text(blob, off, n, mask, words, blob_shift=0, fill=SENTINEL):
    lib = _lib.load()
    total, count = int(off[-1]), int(mask.sum())
    holder = torch.zeros(max(total, 16) + 32, dtype=torch.uint8, device=DEV)
    blob_d = holder[blob_shift:blob_shift + max(total, 16)]
    if total:
        blob_d[:total] = torch.from_numpy(blob).to(DEV)
    off_d = torch.from_numpy(off).to(DEV)
    words_d = upload_words(words)
    rank, cnt = plan(words_d, n)
    assert cnt[0].item() == count
    new_blob = torch.full((max(total, 16) + 64,), fill, dtype=torch.uint8, device=DEV)
    new_off = torch.full((count + 1 + 8,), -3 if fill == SENTINEL else 0, dtype=torch.int64, device=DEV)
    _lib.check(lib.arx_compact_text(blob_d.data_ptr(), off_d.data_ptr(), n, words_d.data_ptr(), rank.data_ptr(), new_blob.data_ptr(),
                                    new_off.data_ptr(), torch.cuda.current_stream().cuda_stream), "arx_compact_text")
    return new_blob.cpu().numpy(), new_off.cpu().numpy()


def check_text(blob, off, n, mask, words, what, **kw):
    lens = np.diff(off)
    want_off = np.concatenate([[0], np.cumsum(lens[mask])]).astype(np.int64)
    want_blob = blob[np.repeat(mask, lens)]
    outs = []
    for fill in (SENTINEL, 0x00) if kw.pop("twice", False) else (SENTINEL,):
        got_blob, got_off = run_text(blob, off, n, mask, words, fill=fill, **kw)
        assert np.array_equal(got_off[:len(want_off)], want_off), what
        assert (got_off[len(want_off):] == (-3 if fill == SENTINEL else 0)).all(), what
        assert np.array_equal(got_blob[:len(want_blob)], want_blob), what
        assert (got_blob[len(want_blob):] == fill).all(), what
        outs.append(got_blob[:len(want_blob)])
    assert all(np.array_equal(outs[0], o) for o in outs)


@pytest.mark.parametrize("n", N_ROWS)
def test_text_equals_the_host(n):
    rs = np.random.RandomState(1000 + n)
    blob, off = text_rows(n, rs)
    for name, (mask, words) in keep_patterns(n, rs).items():
        check_text(blob, off, n, mask, words, (n, name), twice=name == "random")
    mask, words = keep_patterns(n, rs)["random"]
    check_text(blob, off, n, mask, words, (n, "blob 3 bytes behind a 16-byte boundary"), blob_shift=3)


@pytest.mark.parametrize("n", (1, 65, 4099))
def test_text_of_empty_rows_only(n):
    rs = np.random.RandomState(n)
    off = np.zeros(n + 1, np.int64)
    for name, (mask, words) in keep_patterns(n, rs).items():
        check_text(np.zeros(0, np.uint8), off, n, mask, words, (n, name))
