// arx_topk_search_filtered_multi: filtered exact top-k with a DIFFERENT filter per query in one call (C ABI in include/arx.h): a set of up
// to 64 row bitmaps (allow[f], the bit convention of arx_topk_search_filtered) and one filter index per query (filter_of[q], device data).
// Query q sees the rows of allow[filter_of[q]]; an index outside [0, n_filters) means it sees none and answers all (-inf, -1).
//
// The search itself is masked_topk.h's; this file is its filter-set policy, between filter.hip (one bitmap per call) and prefix.hip (one
// limit per query):
//   per batch     filter_set_batch_kernel: the indices clamped (fq[q], -1 = sees nothing: out of range, or padding) and, per 64 queries, the
//                 set of filters they use as a 64-bit word (used[b]) and whether one of them sees nothing (inv[b]).  From here on no
//                 kernel reads filter_of, so nothing the caller put there can become an address.
//   pass A        a 256-row tile is skipped when no filter that the block's query tile uses has a bit in its four words (the OR over the
//                 used filters: lane f of every wave reads filter f's four words, one __any — the same in every wave, so block-uniform).
//                 A query tile whose queries all use one filter takes BitmapMask's route: four uniform loads, one select word for all
//                 its queries.  A mixed tile loads one word per (query, group) in the epilogue, beside the select, after the MFMA loop.
//   the tail      a query reads every group; a group's visible rows are its own filter's word.  A query that sees nothing reads none.
//   exhaustive    the row list of query q is that of its filter, and it is COMPUTED, not stored (kListInMemory = false): per filter the
//                 exclusive popcount offsets of its words (filter_scan_kernel, one block per filter), and list_row(q, pos) = binary search
//                 for the word that holds position pos, then select-the-n-th-set-bit inside it.  n_filters lists of n_rows int64 would be
//                 512 MB at 64 filters x 1 M rows; the offsets are 8 MB.
//   path 0        the host cannot see filter_of, so it bounds the (visible row, query) pairs by max_f n_allowed[f] * n_queries: the
//                 exhaustive path when every n_allowed[f] is given and that bound is below 2^18 — the smaller of BitmapMask's two measured
//                 crossovers, because a list position costs a ~log2(n_rows / 64)-step search here where it is one load there, and no
//                 crossover of its own has been measured — else the masked scan with its fallback.
// Workspace (masked_layout): stats 64 B | gmax n_groups * ldg * 4 | own[0] = used ldg/64 * 8 + fq ldg * 4 + inv ldg/64 * 4 |
// own[1] = offsets 64 * (n_groups + 1) * 8 | redo qb * 4 | part_s, part_i parts * qb * k * (4 + 8), each rounded up to 256 B, with
// qb = min(n_queries, 1 024), ldg = qb rounded up to 64, n_groups = ceil(n_rows / 64), parts = min(ceil(n_rows / 256), 128).  The offsets
// are laid out for 64 filters whatever n_filters is: one workspace serves every filter set over the same shard.
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

#define FSET_MAX_FILTERS 64                      // one bit per filter in used[b]; one lane per filter in the tile test
#define FSET_EXHAUSTIVE_MAX_PAIRS (1ll << 18)

// the batch's filter indices: fq[q] = filter_of[q] if it names a filter, else -1 (also for the padding up to a multiple of 64); per 64
// queries the filters in use (bit f of used[b]) and whether a query of the batch among them sees nothing (inv[b])
__global__ __launch_bounds__(64) void filter_set_batch_kernel(const int32_t* __restrict__ filter_of, int nq, int n_filters,
                                                               int32_t* __restrict__ fq, uint64_t* __restrict__ used,
                                                               int32_t* __restrict__ inv) {
    const int lane = threadIdx.x, q = blockIdx.x * 64 + lane;
    const int f = q < nq ? filter_of[q] : -1;
    const bool ok = f >= 0 && f < n_filters;
    fq[q] = ok ? f : -1;
    uint64_t m = ok ? (1ull << f) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o);
    const int bad = __any(q < nq && !ok);
    if (lane == 0) { used[blockIdx.x] = m; inv[blockIdx.x] = bad; }
}

// the position of the n-th (from 0) set bit of w; w has more than n set bits
__device__ __forceinline__ int select_bit(uint64_t w, int n) {
    int pos = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int c = __popcll(w & ((1ull << s) - 1ull));
        if (n >= c) { n -= c; w >>= s; pos += s; }
    }
    return pos;
}

// ---- the mask policy (masked_topk.h) -------------------------------------------------------------------------------------------------------
struct FilterSetMask {
    const uint64_t* allow;      // the caller's bitmaps [n_filters][n_words]
    int32_t n_filters;
    const int64_t* n_allowed;   // the caller's counts of their set bits, host [n_filters] or null; -1 = unknown (host only)
    const int32_t* filter_of;   // the caller's filter index per query of the call (read by filter_set_batch_kernel only)
    int64_t n_words;            // ceil(n_rows / 64): a bitmap's length
    uint64_t* used;             // workspace: per 64 queries of the batch, the filters they use
    int32_t* fq;                // workspace: the batch's indices, -1 = the query sees nothing
    int32_t* inv;               // workspace: per 64 queries, "one of them sees nothing"
    int64_t* off;               // workspace: [n_filters][n_words + 1] offsets of the words' rows in the filter's row list

    // pass A
    struct Keep {               // a group's word shifted down to this lane's first row
        uint64_t w;
        __device__ __forceinline__ bool operator()(int j, int r) const { return (w >> (uint32_t)(j * 16 + r)) & 1ull; }
    };
    struct LaneRows {
        const uint64_t* col;    // word g of filter 0; filter f's is n_words * f further
        const int32_t* fq; int64_t n_words; uint64_t valid, mine; uint32_t lrow; bool uniform;
        __device__ __forceinline__ Keep of_query(int m, int nq) const {
            if (uniform) return {mine};                        // block-uniform: one filter for every query of the tile
            const int f = m < nq ? fq[m] : -1;
            const uint64_t w = f >= 0 ? (col[(int64_t)f * n_words] & valid) : 0ull;
            return {w >> lrow};
        }
    };
    struct Tile {
        bool empty, uniform; uint64_t mine; const uint64_t* allow; const int32_t* fq; int64_t n_words, n_rows;
        __device__ __forceinline__ LaneRows lane_rows(int64_t g, int lane) const {
            const uint32_t lrow = (uint32_t)(lane >> 4) * 4u;
            return {allow + g, fq, n_words, valid_bits(n_rows, g), mine >> lrow, lrow, uniform};
        }
    };
    template <int BM>
    __device__ __forceinline__ Tile tile(int64_t n0, int wn, int m0, int nq, int64_t n_rows) const {
        const int n_q64 = (nq + 63) >> 6;
        uint64_t u = 0; int bad = 0;                           // the filters this block's queries use (block-uniform)
#pragma unroll
        for (int j = 0; j < BM / 64; ++j) {
            const int b = (m0 >> 6) + j;
            if (b < n_q64) { u |= used[b]; bad |= inv[b]; }
        }
        const int64_t g0 = n0 >> 6;
        Tile t{true, false, 0ull, allow, fq, n_words, n_rows};
        if (u == 0ull) return t;                               // no query of the tile sees any row
        if (!bad && (u & (u - 1ull)) == 0ull) {                // one filter for the whole tile: BitmapMask's four uniform loads
            const uint64_t* a = allow + (int64_t)(__ffsll((unsigned long long)u) - 1) * n_words;
            uint64_t any = 0, mine = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t gj = g0 + j;
                const uint64_t w = gj < n_words ? (a[gj] & valid_bits(n_rows, gj)) : 0ull;
                any |= w;
                mine = j == wn ? w : mine;
            }
            t.empty = any == 0ull; t.uniform = true; t.mine = mine;
            return t;
        }
        const int lane = threadIdx.x & 63;                     // lane f: filter f's four words of the tile (bits of u lie below n_filters)
        bool hit = false;
        if ((u >> lane) & 1ull) {
            const uint64_t* a = allow + (int64_t)lane * n_words;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t gj = g0 + j;
                if (gj < n_words) hit |= (a[gj] & valid_bits(n_rows, gj)) != 0ull;
            }
        }
        t.empty = !__any(hit);                                 // every wave reads the same words: the same answer in all of them
        return t;
    }
    // the tail
    struct Query {
        const uint64_t* allow; int64_t n_rows, n_groups;
        __device__ __forceinline__ uint64_t word(int64_t g) const { return allow[g] & valid_bits(n_rows, g); }
    };
    __device__ __forceinline__ Query query(int q, int64_t n_rows, int64_t n_groups) const {
        const int f = fq[q];
        return {allow + (int64_t)(f < 0 ? 0 : f) * n_words, n_rows, f < 0 ? 0 : n_groups};      // sees nothing: reads no group
    }
    // exhaustive
    __device__ __forceinline__ int64_t list_total(int q) const {
        const int f = fq[q];
        return f < 0 ? 0 : off[(int64_t)f * (n_words + 1) + n_words];
    }
    static constexpr bool kListInMemory = false;
    __device__ __forceinline__ int64_t list_row(int q, int64_t pos) const {      // pos < list_total(q), so fq[q] >= 0
        const int f = fq[q];
        const int64_t* o = off + (int64_t)f * (n_words + 1);
        int64_t lo = 0, hi = n_words;                          // the last word whose offset is <= pos: it holds the position
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (o[mid] <= pos) lo = mid; else hi = mid;
        }
        // (the offsets count the bits below n_rows only and those lie below any garbage bit, so the raw word serves)
        return lo * GROUP_ROWS + select_bit(allow[(int64_t)f * n_words + lo], (int)(pos - o[lo]));
    }

    // host
    static constexpr const char* kWorkspaceFn = "arx_topk_filtered_multi_workspace_bytes";
    bool given() const { return allow != nullptr && filter_of != nullptr; }
    int check(int64_t n_rows) const {
        ARX_REQUIRE(n_filters >= 1 && n_filters <= FSET_MAX_FILTERS, "n_filters=%d out of range 1..%d", n_filters, FSET_MAX_FILTERS);
        if (n_allowed)
            for (int f = 0; f < n_filters; ++f)
                ARX_REQUIRE(n_allowed[f] >= -1 && n_allowed[f] <= n_rows, "n_allowed[%d]=%lld", f, (long long)n_allowed[f]);
        return ARX_OK;
    }
    int choose_path(int32_t n_queries) const {
        if (!n_allowed) return 1;
        int64_t most = 0;
        for (int f = 0; f < n_filters; ++f) {
            if (n_allowed[f] < 0) return 1;
            most = n_allowed[f] > most ? n_allowed[f] : most;
        }
        return most * (int64_t)n_queries < FSET_EXHAUSTIVE_MAX_PAIRS ? 2 : 1;
    }
    static void own_bytes(const MaskedWs& L, int64_t, int64_t b[2]) {
        b[0] = L.ldg / 64 * 8 + L.ldg * 4 + L.ldg / 64 * 4;
        b[1] = (int64_t)FSET_MAX_FILTERS * (L.n_groups + 1) * 8;
    }
    void bind(char* ws, const MaskedWs& L) {
        used = (uint64_t*)(ws + L.own[0]);
        fq = (int32_t*)(used + L.ldg / 64);
        inv = fq + L.ldg;
        off = (int64_t*)(ws + L.own[1]);
    }
    int prepare_batch(int q0, int nq, int64_t, hipStream_t st) const {
        filter_set_batch_kernel<<<cdiv(nq, 64), 64, 0, st>>>(filter_of + q0, nq, n_filters, fq, used, inv);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    int prepare_lists(int q0, int path, int64_t n_rows, int64_t n_groups, const int* gate, hipStream_t st) const {
        if (q0 == 0 || path == 1) {                            // (the offsets do not depend on the batch; after an overflow they are built then)
            filter_scan_kernel<<<n_filters, 1024, 0, st>>>(allow, n_groups, n_rows, off, gate);
            ARX_HIP_CHECK(hipGetLastError());
        }
        return ARX_OK;
    }
};
}      // namespace

extern "C" int64_t arx_topk_filtered_multi_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n_filters, int32_t dim, int32_t k) {
    if (n_filters < 1 || n_filters > FSET_MAX_FILTERS) return -1;
    return masked_workspace_bytes<FilterSetMask>(n_rows, n_queries, dim, k);
}

extern "C" int32_t arx_topk_search_filtered_multi_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int32_t n_filters,
                                                        const int64_t* n_allowed, const int32_t* filter_of, const void* queries,
                                                        int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids,
                                                        int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                                                        int32_t cand_cap, void* stream) {
    FilterSetMask mask{allow, n_filters, n_allowed, filter_of, (n_rows + GROUP_ROWS - 1) / GROUP_ROWS, nullptr, nullptr, nullptr, nullptr};
    return masked_search_impl(mask, corpus, n_rows, queries, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm, ws, ws_bytes, path,
                              cand_cap, stream);
}

extern "C" int32_t arx_topk_search_filtered_multi(const void* corpus, int64_t n_rows, const uint64_t* allow, int32_t n_filters,
                                                  const int64_t* n_allowed, const int32_t* filter_of, const void* queries, int32_t n_queries,
                                                  int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                                                  float max_row_norm, void* ws, int64_t ws_bytes, void* stream) {
    return arx_topk_search_filtered_multi_tuned(corpus, n_rows, allow, n_filters, n_allowed, filter_of, queries, n_queries, dim, k, out_scores,
                                                out_ids, idx_base, max_row_norm, ws, ws_bytes, 0, 0, stream);
}

extern "C" int32_t arx_topk_filtered_multi_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    return masked_stats(ws, overflowed_queries, candidate_groups, stream);
}
