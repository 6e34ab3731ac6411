"""The workspace sizes of the five searches that the scan driver serves (csrc/masked_topk.h), pinned to recorded values (CPU): the common
prefix plus each search's own buffers must add up to what `arx_topk_filtered_workspace_bytes`, `arx_topk_filtered_multi_workspace_bytes`,
`arx_topk_prefix_workspace_bytes`, `arx_range_workspace_bytes` and `arx_topk_grouped_workspace_bytes` returned before the searches shared
one driver and one layout, and the shapes each refuses stay refused.  The numbers are this library's own output, recorded from the build
before the change; callers size allocations they keep by them."""
import pytest

ROWS = (1, 64, 65, 1000, (1 << 20) + 1)
NQ = (1, 64, 65, 1024, 1025)
DIMS = (64, 768)                                             # dim is checked, it does not enter the size

# RECORDED[search][k | (n_filters, k) | max_results | (n_groups, chunks_per_group)][i_rows][i_nq]: the argument at its minimum and maximum
RECORDED = {
    "filtered": {
        1: ((1792, 2048, 3072, 21248, 21248),
                 (2048, 2304, 3328, 21504, 21504),
                 (2560, 2816, 4096, 25856, 25856),
                 (13568, 16128, 20992, 127488, 127488),
                 (12716800, 12813568, 17009920, 77210368, 77210368)),
        32: ((1792, 25856, 26880, 402176, 402176),
                 (2048, 26112, 27136, 402432, 402432),
                 (2560, 26624, 27904, 406784, 406784),
                 (14592, 111360, 117248, 1651200, 1651200),
                 (12764416, 15860992, 20104960, 125969152, 125969152)),
    },
    "filtered_multi": {
        (1, 1): ((2816, 3072, 4352, 26112, 26112),
                 (2816, 3072, 4352, 26112, 26112),
                 (3584, 3840, 5376, 30720, 30720),
                 (14336, 16896, 22016, 132096, 132096),
                 (12586752, 12683520, 16880128, 77084160, 77084160)),
        (64, 32): ((2816, 26880, 28160, 407040, 407040),
                 (2816, 26880, 28160, 407040, 407040),
                 (3584, 27648, 29184, 411648, 411648),
                 (15360, 112128, 118272, 1655808, 1655808),
                 (12634368, 15730944, 19975168, 125842944, 125842944)),
    },
    "prefix": {
        1: ((2048, 2304, 3840, 29184, 29184),
                 (2048, 2304, 3840, 29184, 29184),
                 (2304, 2560, 4352, 33280, 33280),
                 (5888, 8448, 13824, 127488, 127488),
                 (4197376, 4294144, 8491008, 68698624, 68698624)),
        32: ((2048, 26112, 27648, 410112, 410112),
                 (2048, 26112, 27648, 410112, 410112),
                 (2304, 26368, 28160, 414208, 414208),
                 (6912, 103680, 110080, 1651200, 1651200),
                 (4244992, 7341568, 11586048, 117457408, 117457408)),
    },
    "range": {
        1: ((1536, 1792, 2816, 20992, 20992),
                 (1536, 1792, 2816, 20992, 20992),
                 (1792, 2048, 3328, 25088, 25088),
                 (5376, 7936, 12800, 119296, 119296),
                 (4327936, 4424704, 8621056, 68821504, 68821504)),
        1024: ((9472, 525568, 534528, 8401408, 8401408),
                 (9472, 525568, 534528, 8401408, 8401408),
                 (9728, 525824, 535040, 8405504, 8405504),
                 (37888, 2103040, 2140416, 33640960, 33640960),
                 (4359424, 6424576, 10652416, 100819456, 100819456)),
    },
    "grouped": {
        (1, 1): ((2048, 2560, 4096, 33280, 33280),
                 (2048, 2560, 4096, 33280, 33280),
                 (2304, 2816, 4608, 37376, 37376),
                 (5888, 8704, 14080, 131584, 131584),
                 (4328448, 4425472, 8622336, 68833792, 68833792)),
        (32, 8): ((2048, 50176, 51712, 795136, 795136),
                 (2048, 50176, 51712, 795136, 795136),
                 (2304, 50432, 52224, 799232, 799232),
                 (6912, 127744, 134144, 2036224, 2036224),
                 (4376064, 7496704, 11741184, 117973504, 117973504)),
    },
}


def _functions():
    from arxiv_rag_amd import _lib
    lib = _lib.load()
    return {
        "filtered": lambda n, q, d, a: lib.arx_topk_filtered_workspace_bytes(n, q, d, a),
        "filtered_multi": lambda n, q, d, a: lib.arx_topk_filtered_multi_workspace_bytes(n, q, a[0], d, a[1]),
        "prefix": lambda n, q, d, a: lib.arx_topk_prefix_workspace_bytes(n, q, d, a),
        "range": lambda n, q, d, a: lib.arx_range_workspace_bytes(n, q, d, a),
        "grouped": lambda n, q, d, a: lib.arx_topk_grouped_workspace_bytes(n, q, d, a[0], a[1]),
    }


@pytest.mark.parametrize("search", sorted(RECORDED))
def test_workspace_sizes_are_the_recorded_ones(search):
    f = _functions()[search]
    for arg, by_rows in RECORDED[search].items():
        for n, by_nq in zip(ROWS, by_rows):
            for nq, want in zip(NQ, by_nq):
                for dim in DIMS:
                    assert f(n, nq, dim, arg) == want, (search, arg, n, nq, dim)


def test_sizes_at_the_edges_of_what_each_function_answers():
    """The top-k functions bound neither dim nor n_rows (the search call does); range and grouped answer up to their last shape."""
    f = _functions()
    assert f["filtered"](1000, 64, 8256, 10) == 43776 and f["filtered_multi"](1000, 64, 8256, (1, 10)) == 44544
    assert f["prefix"](1 << 36, 1, 64, 1) == 274877909760
    assert f["range"]((1 << 32) - 1, 1, 64, 1) == 17716742144 and f["range"](1000, 64, 8192, 10) == 26368
    assert f["grouped"]((1 << 36) - 1, 1, 64, (1, 1)) == 283467844096 and f["grouped"](1000, 64, 8192, (10, 3)) == 43264


def test_refused_shapes_stay_refused():
    f = _functions()
    common = ((0, 1, 64), (-1, 1, 64), (1000, 0, 64), (1000, -1, 64), (1000, 64, 0), (1000, 64, -64), (1000, 64, 100), (1000, 64, 32))
    good = {"filtered": 10, "filtered_multi": (4, 10), "prefix": 10, "range": 10, "grouped": (10, 3)}
    for search, arg in good.items():
        assert f[search](1000, 64, 768, arg) > 0
        for n, nq, dim in common:
            assert f[search](n, nq, dim, arg) == -1, (search, n, nq, dim)
    for search in ("filtered", "prefix"):
        for k in (0, -1, 33):
            assert f[search](1000, 64, 768, k) == -1, (search, k)
    for arg in ((4, 0), (4, 33), (0, 10), (65, 10), (-1, 10)):
        assert f["filtered_multi"](1000, 64, 768, arg) == -1, arg
    for n, dim, M in ((1000, 768, 0), (1000, 768, -1), (1000, 768, 1025), (1000, 8256, 10), (1 << 32, 64, 1)):
        assert f["range"](n, 64, dim, M) == -1, (n, dim, M)
    for n, dim, arg in ((1000, 768, (0, 3)), (1000, 768, (33, 3)), (1000, 768, (10, 0)), (1000, 768, (10, 9)), (1000, 8256, (10, 3)),
                        (1 << 36, 64, (1, 1))):
        assert f["grouped"](n, 64, dim, arg) == -1, (n, dim, arg)
