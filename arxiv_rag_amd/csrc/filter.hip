// arx_topk_search_filtered: exact top-k over the ALLOWED rows of an fp16 shard (C ABI in include/arx.h; Chroma's `where`).
//
// The filter is a bitmap, one 64-bit word per 64-row group (bit r & 63 of word r >> 6 = row r may be returned; bits at or beyond n_rows
// are ignored), shared by all queries of the call.  The search itself is masked_topk.h's; this file is its bitmap policy:
//   pass A        a wave's select is a bit of its group's word, the same for every query; a 256-row tile whose four words are zero is
//                 skipped
//   the tail      a query reads every group of the shard; a group's visible rows are its word
//   exhaustive    the bitmap compacted to the list of allowed rows (popcount + scan, scatter: bitmap_rows.h), once per call, or
//                 after a masked scan's overflow; the list is the same for every query
//   path 0        the exhaustive path when the caller gave n_allowed and (allowed row, query) pairs are few, else the masked scan
#include <math.h>

#include "arx_common.h"
#include "gemm.h"
#include "gemm8.h"
#include "search_consts.h"

namespace {      // the headers also define non-template kernels: internal linkage keeps this object's copies apart from search.hip's
#include "search_pass_a.h"
#include "search_tail.h"
#include "masked_topk.h"
#include "bitmap_rows.h"

// path = 0 with n_allowed known: the exhaustive path below this many (allowed row, query) pairs.  Measured (profiles/filter_bench.json:
// 1 M x 768 unit rows, k = 10, ms per batch, exhaustive against masked scan): 64 queries — 0.239 / 0.321 at 0.67 M pairs, 0.287 / 0.334 at
// 1.05 M, 1.146 / 0.347 at 6.7 M; 1 query (the exhaustive grid is then 128 blocks) — 0.176 / 0.347 at 0.10 M, 0.173 / 0.184 at 0.13 M,
// 0.424 / 0.353 at 0.52 M.  Hence 2^20 pairs from 64 queries on, 2^18 below.
#define FILT_EXHAUSTIVE_MAX_PAIRS_WIDE (1ll << 20)
#define FILT_EXHAUSTIVE_MAX_PAIRS (1ll << 18)
#define FILT_WIDE_NQ 64

// ---- the mask policy (masked_topk.h) -------------------------------------------------------------------------------------------------------
struct BitmapMask : BitmapRows {      // pass A and `allow`, the caller's bitmap: bitmap_rows.h
    int64_t n_allowed;          // the caller's count of its set bits, -1 = unknown (host only)
    int64_t* off;               // workspace: [n_groups + 1] offsets of the words' rows in `rows`
    int64_t* rows;              // workspace: the allowed rows in ascending order
    const int64_t* n_list;      // = off + n_groups: the number of allowed rows

    // the tail
    struct Query {
        const uint64_t* allow; int64_t n_rows, n_groups;
        __device__ __forceinline__ uint64_t word(int64_t g) const { return allow[g] & valid_bits(n_rows, g); }
    };
    __device__ __forceinline__ Query query(int, int64_t n_rows, int64_t n_groups) const { return {allow, n_rows, n_groups}; }
    // exhaustive
    __device__ __forceinline__ int64_t list_total(int) const { return *n_list; }
    static constexpr bool kListInMemory = true;
    __device__ __forceinline__ int64_t list_row(int, int64_t pos) const { return rows[pos]; }

    // host
    static constexpr const char* kWorkspaceFn = "arx_topk_filtered_workspace_bytes";
    bool given() const { return allow != nullptr; }
    int check(int64_t n_rows) const {
        ARX_REQUIRE(n_allowed >= -1 && n_allowed <= n_rows, "n_allowed=%lld", (long long)n_allowed);
        return ARX_OK;
    }
    int choose_path(int32_t n_queries) const {
        return (n_allowed >= 0 && n_allowed * (int64_t)n_queries < (n_queries >= FILT_WIDE_NQ ? FILT_EXHAUSTIVE_MAX_PAIRS_WIDE : FILT_EXHAUSTIVE_MAX_PAIRS))
                   ? 2 : 1;
    }
    static void own_bytes(const MaskedWs& L, int64_t n_rows, int64_t b[2]) { b[0] = (L.n_groups + 1) * 8; b[1] = n_rows * 8; }
    void bind(char* ws, const MaskedWs& L) { off = (int64_t*)(ws + L.own[0]); rows = (int64_t*)(ws + L.own[1]); n_list = off + L.n_groups; }
    int prepare_batch(int, int, int64_t, hipStream_t) const { return ARX_OK; }
    int prepare_lists(int q0, int path, int64_t n_rows, int64_t n_groups, const int* gate, hipStream_t st) const {
        if (q0 == 0 || path == 1) {                            // (the list does not depend on the batch; after an overflow it is built then)
            filter_scan_kernel<<<1, 1024, 0, st>>>(allow, n_groups, n_rows, off, gate);
            ARX_HIP_CHECK(hipGetLastError());
            filter_scatter_kernel<<<cdiv(n_groups, 4), 256, 0, st>>>(allow, n_groups, n_rows, off, rows, gate);
            ARX_HIP_CHECK(hipGetLastError());
        }
        return ARX_OK;
    }
};
}      // namespace

extern "C" int64_t arx_topk_filtered_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k) {
    return masked_workspace_bytes<BitmapMask>(n_rows, n_queries, dim, k);
}

extern "C" int32_t arx_topk_search_filtered_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                                  int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids,
                                                  int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                                                  int32_t cand_cap, void* stream) {
    return masked_search_impl(BitmapMask{{allow}, n_allowed, nullptr, nullptr, nullptr}, corpus, n_rows, queries, n_queries, dim, k, out_scores, out_ids,
                              idx_base, max_row_norm, ws, ws_bytes, path, cand_cap, stream);
}

extern "C" int32_t arx_topk_search_filtered(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                            int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                                            float max_row_norm, void* ws, int64_t ws_bytes, void* stream) {
    return arx_topk_search_filtered_tuned(corpus, n_rows, allow, n_allowed, queries, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm,
                                          ws, ws_bytes, 0, 0, stream);
}

extern "C" int32_t arx_topk_filtered_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    return masked_stats(ws, overflowed_queries, candidate_groups, stream);
}
