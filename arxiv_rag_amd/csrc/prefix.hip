// arx_topk_search_prefix: exact top-k with a row limit PER QUERY over an fp16 shard (C ABI in include/arx.h).  Query q may return only
// the local rows r < row_limit[q]; with the queries pointing into the corpus and row_limit[q] = the query's own row this is the
// self-join "nearest earlier row" that near-duplicate detection needs (dedup.py).
//
// The search itself is masked_topk.h's; this file is its prefix policy.  Every query has its own mask, but a mask of a special form, so
// it needs no bitmap at all:
//   pass A        the select is one integer comparison per accumulator element (row < lim[query]); a 256-row tile whose first row is at
//                 or beyond the largest limit of the block's query tile is skipped: for a self-join of consecutive rows that is the
//                 upper triangle
//   the tail      a query reads only the groups that start below its limit (the others hold -inf); a group's visible rows are the low
//                 bits of a word
//   exhaustive    the rows are the prefix [0, lim[q]): the list needs no compaction, position = row
//   path 0        the masked scan with its fallback
#include <math.h>

#include "arx_common.h"
#include "gemm.h"
#include "gemm8.h"
#include "search_consts.h"

namespace {      // the headers also define non-template kernels: internal linkage keeps this object's copies apart from search.hip's
#include "search_pass_a.h"
#include "search_tail.h"
#include "masked_topk.h"

// the batch's limits clamped to [0, n_rows] (lim[q]; 0 for the padding up to a multiple of 64) and their maximum per 64 queries (tmax)
__global__ __launch_bounds__(64) void prefix_limits_kernel(const int64_t* __restrict__ row_limit, int nq, int64_t n_rows,
                                                            int64_t* __restrict__ lim, int64_t* __restrict__ tmax) {
    const int lane = threadIdx.x, q = blockIdx.x * 64 + lane;
    int64_t v = q < nq ? row_limit[q] : 0;
    v = v < 0 ? 0 : (v > n_rows ? n_rows : v);
    lim[q] = v;
    int64_t m = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t x = __shfl_xor(m, o);
        m = x > m ? x : m;
    }
    if (lane == 0) tmax[blockIdx.x] = m;
}

// the rows of group g below `lim` as a mask word (g * 64 < lim for every group the tail lists)
__device__ __forceinline__ uint64_t prefix_bits(int64_t lim, int64_t g) {
    const int64_t rem = lim - g * GROUP_ROWS;
    return rem >= GROUP_ROWS ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
}

// ---- the mask policy (masked_topk.h) -------------------------------------------------------------------------------------------------------
struct PrefixMask {
    const int64_t* row_limit;   // the caller's limits, one per query of the call (host only)
    int64_t* lim;               // workspace: the batch's clamped limits
    int64_t* tmax;              // workspace: their maximum per 64 queries

    // pass A.  The limits are clamped to n_rows, so a position past the shard's end (pass A clamps its row address: a copy of the last
    // row) is never below one.
    struct LaneRows {
        const int64_t* lim; int64_t g0; int lrow;
        struct Below {          // rows of the group below the query's limit, counted from this lane's first
            int rel;
            __device__ __forceinline__ bool operator()(int j, int r) const { return (j * 16 + r) < rel; }
        };
        __device__ __forceinline__ Below of_query(int m, int nq) const {
            const int64_t d = (m < nq ? lim[m] : 0) - g0;
            return {(int)(d < 0 ? 0 : (d > GROUP_ROWS ? GROUP_ROWS : d)) - lrow};
        }
    };
    struct Tile {
        bool empty; const int64_t* lim;
        __device__ __forceinline__ LaneRows lane_rows(int64_t g, int lane) const { return {lim, g * GROUP_ROWS, (lane >> 4) * 4}; }
    };
    template <int BM>
    __device__ __forceinline__ Tile tile(int64_t n0, int, int m0, int nq, int64_t) const {
        const int n_q64 = (nq + 63) >> 6;
        int64_t top = 0;                                       // the largest limit of this block's queries (block-uniform)
#pragma unroll
        for (int j = 0; j < BM / 64; ++j) {
            const int b = (m0 >> 6) + j;
            const int64_t v = b < n_q64 ? tmax[b] : 0;
            top = v > top ? v : top;
        }
        return {n0 >= top, lim};
    }
    // the tail
    struct Query {
        int64_t limit, n_groups;
        __device__ __forceinline__ uint64_t word(int64_t g) const { return prefix_bits(limit, g); }
    };
    __device__ __forceinline__ Query query(int q, int64_t, int64_t) const {
        const int64_t limit = lim[q];
        return {limit, (limit + GROUP_ROWS - 1) / GROUP_ROWS};
    }
    // exhaustive
    __device__ __forceinline__ int64_t list_total(int q) const { return lim[q]; }
    static constexpr bool kListInMemory = false;
    __device__ __forceinline__ int64_t list_row(int, int64_t pos) const { return pos; }

    // host
    static constexpr const char* kWorkspaceFn = "arx_topk_prefix_workspace_bytes";
    bool given() const { return row_limit != nullptr; }
    int check(int64_t) const { return ARX_OK; }
    int choose_path(int32_t) const { return 1; }      // no crossover against the exhaustive path has been measured: the masked scan with its fallback
    static void own_bytes(const MaskedWs& L, int64_t, int64_t b[2]) { b[0] = L.ldg * 8; b[1] = L.ldg / 64 * 8; }
    void bind(char* ws, const MaskedWs& L) { lim = (int64_t*)(ws + L.own[0]); tmax = (int64_t*)(ws + L.own[1]); }
    int prepare_batch(int q0, int nq, int64_t n_rows, hipStream_t st) const {
        prefix_limits_kernel<<<cdiv(nq, 64), 64, 0, st>>>(row_limit + q0, nq, n_rows, lim, tmax);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    int prepare_lists(int, int, int64_t, int64_t, const int*, hipStream_t) const { return ARX_OK; }
};
}      // namespace

extern "C" int64_t arx_topk_prefix_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k) {
    return masked_workspace_bytes<PrefixMask>(n_rows, n_queries, dim, k);
}

extern "C" int32_t arx_topk_search_prefix_tuned(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit,
                                                int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids,
                                                int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                                                int32_t cand_cap, void* stream) {
    return masked_search_impl(PrefixMask{row_limit, nullptr, nullptr}, corpus, n_rows, queries, n_queries, dim, k, out_scores, out_ids, idx_base,
                              max_row_norm, ws, ws_bytes, path, cand_cap, stream);
}

extern "C" int32_t arx_topk_search_prefix(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit, int32_t n_queries,
                                          int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm,
                                          void* ws, int64_t ws_bytes, void* stream) {
    return arx_topk_search_prefix_tuned(corpus, n_rows, queries, row_limit, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm, ws,
                                        ws_bytes, 0, 0, stream);
}

extern "C" int32_t arx_topk_prefix_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    return masked_stats(ws, overflowed_queries, candidate_groups, stream);
}
