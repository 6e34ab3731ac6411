"""The workspace sizes of the two candidate scans that share one kernel and one driver (csrc/key_lists.h), pinned to recorded values
(CPU): `arx_binary_workspace_bytes` and `arx_pq_workspace_bytes` must answer what they answered before the scans were written once, and
the shapes each refuses stay refused.  The numbers are this library's own output, recorded from the build before the change; callers
size allocations they keep by them."""
ROWS = (0, 1, 64, 65, 1000, (1 << 20) + 1)
NQ = (1, 255, 256, 257, 1025)
DIMS = ((64, 4), (64, 8), (768, 4), (768, 8))                   # (dim, PQ's dsub): both are checked, neither enters the size

# RECORDED[n_candidates][i_rows][i_nq], the same for both functions
RECORDED = {
    1: ((256, 2048, 2048, 2048, 2048),
        (256, 2048, 2048, 2048, 2048),
        (256, 2048, 2048, 2048, 2048),
        (256, 4096, 4096, 4096, 4096),
        (256, 32768, 32768, 32768, 32768),
        (131328, 262144, 262144, 262144, 262144)),
    256: ((2048, 522240, 524288, 524288, 524288),
          (2048, 522240, 524288, 524288, 524288),
          (2048, 522240, 524288, 524288, 524288),
          (4096, 1044480, 1048576, 1048576, 1048576),
          (32768, 8355840, 8388608, 8388608, 8388608),
          (33556480, 67108864, 67108864, 67108864, 67108864)),
}


def _lib():
    from arxiv_rag_amd import _lib
    return _lib.load()


def test_workspace_sizes_are_the_recorded_ones():
    lib = _lib()
    for R, by_rows in RECORDED.items():
        for n, by_nq in zip(ROWS, by_rows):
            for nq, want in zip(NQ, by_nq):
                for dim, dsub in DIMS:
                    assert lib.arx_binary_workspace_bytes(n, nq, dim, R) == want, ("binary", R, n, nq, dim)
                    assert lib.arx_pq_workspace_bytes(n, nq, dim, dsub, R) == want, ("pq", R, n, nq, dim, dsub)


def test_sizes_at_the_last_shapes_each_function_answers():
    lib = _lib()
    assert lib.arx_binary_workspace_bytes((1 << 31) - 1, 1, 64, 1) == 262144 and lib.arx_binary_workspace_bytes(1000, 1, 8192, 1) == 256
    assert lib.arx_pq_workspace_bytes((1 << 31) - 1, 1, 64, 8, 1) == 262144
    assert lib.arx_pq_workspace_bytes(1000, 1, 8192, 32, 1) == 256 and lib.arx_pq_workspace_bytes(1000, 1, 64, 64, 1) == 256


def test_refused_shapes_stay_refused():
    lib = _lib()
    common = ((-1, 1, 64, 1), (1 << 31, 1, 64, 1), (1000, 0, 64, 1), (1000, -1, 64, 1), (1000, 1, 0, 1), (1000, 1, 96, 1), (1000, 1, 8256, 1),
              (1000, 1, 64, 0), (1000, 1, 64, 257))
    for n, nq, dim, R in common:
        assert lib.arx_binary_workspace_bytes(n, nq, dim, R) == -1, (n, nq, dim, R)
        assert lib.arx_pq_workspace_bytes(n, nq, dim, 8, R) == -1, (n, nq, dim, R)
    for dim, dsub in ((8192, 16), (64, 2), (64, 128), (64, 12)):     # M = 512; dsub below 4, above 64, no power of two
        assert lib.arx_pq_workspace_bytes(1000, 1, dim, dsub, 1) == -1, (dim, dsub)
