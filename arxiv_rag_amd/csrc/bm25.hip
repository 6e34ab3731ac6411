// BM25 keyword top-n over a CSR-by-term impact index resident in HBM (gfx950).
//
// Index of one shard: term_ptr int64 [V+1], post_row uint32 [P] (shard-local row, ascending within a term), post_w f32 [P] (the
// posting's BM25 impact, > 0, computed in float64 on the host and rounded once).  A query is its <= 64 distinct term ids in ascending
// order; bm25(q, d) = the sum of the impacts of q's terms in d, ADDED IN ASCENDING TERM ORDER IN F32.
//
// One kernel, one cut, one merge serve every export (arx_bm25_search, _tuned, _filtered, _filtered_tuned: n <= 32; arx_bm25_search_wide:
// n <= 1024); the exports differ in the two numbers of Bm25Limits alone.
//
// bm25_search_kernel<FILTERED>: grid (blocks, queries), 512 threads.  A block walks row tiles of the shard (tile b, b + blocks, ...).  The
// f32 accumulators of one tile live in LDS.  Per tile: the two ends of every term's posting sub-range inside the tile are found by up to
// 128 lanes at once (one binary search on post_row per lane), then the terms are applied one after the other with a workgroup barrier
// between them: rows within a term are distinct, so no two lanes touch one accumulator inside a term, and the barrier fixes the order
// across terms.  There is no float atomic anywhere: a row's score depends on the index and the query's term list alone, not on the
// tile size, the block count or the other queries of the launch.  Posting loads are coalesced along a term's list.
//
// Top-n: a candidate is the 64-bit key (f32 score bits << 32) | (0xffffffff - row); scores are > 0, so the unsigned order of the keys is
// (score desc, row asc) and 0 means "none".  The keys are distinct (distinct rows), so "the n largest keys" is one well-defined set and
// order: the output does not depend on the export, and the m-list is a prefix of the n-list.
//   list     BM25_CAP = 4096 keys in LDS (32 KiB).  While a tile is scanned (which also clears it for the next one) the keys above the
//            block's current n-th best are appended (an INTEGER LDS atomic hands out the slots: the list's order varies, its content and
//            therefore the selected top-n do not).  A chunk appends at most 1024 keys, so after a cut to n <= 1024 keys at least
//            (4096 - 1024) / 1024 = 3 chunks pass before the next cut can be needed; once the n-th key has risen most chunks append little.
//   cut      when the list could overflow, bm25_cut keeps its n largest keys, sorted.  One function, one block-uniform choice on n:
//            n > 32   a block-wide bitonic sort (descending, over the next power of two >= its length, 64 at least), as range.hip cuts
//                     its list: log2(m) (log2(m) + 1) / 2 barriers (78 at m = 4096) whatever n.  The compare-exchange steps with a
//                     distance below 32 keys read two 8-byte words per lane at a stride of two: a 2-way LDS bank conflict on 15 of the
//                     78 steps, accepted.
//            n <= 32  min(n, length) rounds of a block-wide maximum over the keys held in registers (8 per thread), one barrier per
//                     round.  Measured at 1 M documents (profiles/bm25_one_kernel.json): the sort alone costs a 64-query batch
//                     1.98 ms at n = 1 and 1.99 ms at n = 10 where selection takes 1.26 ms and 1.48 ms, and selection is still level
//                     with it at n = 32 (2.01 against 2.06 ms).
//   LDS      tile_rows * 4 + sizeof(Bm25SearchSmem) (32 KiB keys + ~1 KiB) [+ 1.5 KiB bitmap words when filtered].  The default tile
//            is BM25_TILE = 10240 rows: 40 + 33 + 1.5 = 74.5 KiB, TWO blocks per 160 KiB CU.  A tuned call may ask for up to
//            BM25_TILE_MAX = 12288 rows (82.5 KiB: one block per CU).
//   partial  with more than one block per query every block writes its n best keys [blocks, nq, n] (0 = none), sorted, to the workspace:
//            blocks = min(tiles, 512, part_keys / n[, max_blocks]), part_keys = 4096 for the n <= 32 exports (a workspace of
//            4096 queries stays 128 MiB) and 65536 for the wide one (64 blocks at n = 1024).
//            workspace = round_up(min(ceil(n_rows / 1024), 512, part_keys / n) * n_queries * n * 8, 256) bytes: sized for the smallest tile.
//   merge    bm25_merge_kernel, one block per query: the blocks * n keys stream through the same 4096-key LDS list, 1024 per round,
//            with the same cut; its result is the exact n largest keys of the union whatever the block count.
// No float atomics, no global atomics; the LDS slot counter is an integer atomic whose order cannot reach the output.
//
// Row filter (bm25_search_kernel<true>): a block serves one query, so a filter per query is a bitmap base pointer per block (allow +
// filter_of[q] * words; an index outside [0, n_filters) leaves the block without a bitmap and its query without rows).  A tile is a
// multiple of 1024 rows and therefore covers whole 64-bit bitmap words: per tile its first tile_rows / 64 threads load them into LDS
// (bounded by ceil(n_rows / 64), the last word masked to n_rows) and a block-wide OR tells whether any row is allowed.  A tile without
// one is skipped before the binary searches and the posting reads; in the scan a key is appended only when its row's bit is set, and
// the accumulator is cleared either way.  Scores and idf are untouched, so an allowed row has the bits the unfiltered search gives it.
// Out of scope: a doc-at-a-time path for very selective SCATTERED filters.  Such a filter still streams the postings of every tile it
// touches; only filters that leave whole tiles empty (contiguous ranges) save bandwidth.
#include "arx_common.h"

namespace {

constexpr int BM25_NT = 512;                 // threads per block
constexpr int BM25_MAXT = 64;                // query terms
constexpr int BM25_CAP = 4096;               // candidate keys in LDS (32 KiB)
constexpr int BM25_CHUNK = 2 * BM25_NT;      // rows scanned between two capacity checks (2 per thread)
constexpr int BM25_TILE = 10240;             // default tile: two blocks per CU (see above)
constexpr int BM25_TILE_MAX = 12288;
constexpr int BM25_SELECT_N = 32;            // lists up to this length are cut by selection, longer ones by the sort (see "cut")

// what tells the n <= 32 exports from the wide one
struct Bm25Limits {
    int n_max;                               // the longest list
    int part_keys;                           // blocks * n <= this: bounds the partial lists of a query
};
constexpr Bm25Limits BM25_NARROW = {32, 4096}, BM25_WIDE = {1024, 65536};

// the ends of every term's postings inside the current tile
struct Bm25Ends {
    long long lo[BM25_MAXT], hi[BM25_MAXT];
};

struct Bm25List {
    unsigned long long keys[BM25_CAP];
    unsigned long long wred[2][BM25_NT / 64];    // the waves' maxima of a selection round (two rounds in flight)
    unsigned long long thr;
    int cnt;
};

struct Bm25SearchSmem {
    Bm25List list;
    Bm25Ends ends;
};

// the filtered kernel's extra LDS, behind Bm25SearchSmem: the bitmap words of the current tile
struct Bm25FilterSmem {
    unsigned long long bits[BM25_TILE_MAX / 64];
};

// first posting p in [a, b) with post_row[p] >= row (b if none); post_row ascending in [a, b)
__device__ __forceinline__ long long lower_bound_row(const uint32_t* __restrict__ post_row, long long a, long long b, uint32_t row) {
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if (post_row[m] < row) a = m + 1; else b = m;
    }
    return a;
}

// acc[0 .. tile_rows) (all zero on entry) += impacts of the query's terms for rows [tile_lo, tile_hi), in term order.
// Ends with a barrier: acc is complete for every thread on return.
__device__ __forceinline__ void bm25_accumulate_tile(const long long* __restrict__ term_ptr, const uint32_t* __restrict__ post_row,
                                                     const float* __restrict__ post_w, int vocab, const int32_t* __restrict__ terms, int nt,
                                                     uint32_t tile_lo, uint32_t tile_hi, int tile_rows, float* acc, Bm25Ends& sm) {
    const int tid = threadIdx.x;
    if (tid < 2 * BM25_MAXT) {
        const int j = tid & (BM25_MAXT - 1);
        if (j < nt) {
            const int t = terms[j];
            long long r = 0;
            if (t >= 0 && t < vocab) {
                const long long a = term_ptr[t], b = term_ptr[t + 1];
                r = lower_bound_row(post_row, a, b, tid < BM25_MAXT ? tile_lo : tile_hi);
            }
            if (tid < BM25_MAXT) sm.lo[j] = r; else sm.hi[j] = r;       // a term outside the vocabulary: lo = hi = 0, no postings
        }
    }
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
        const long long a = sm.lo[j], b = sm.hi[j];
#pragma unroll 4
        for (long long p = a + tid; p < b; p += BM25_NT) {
            const uint32_t i = post_row[p] - tile_lo;
            const float w = post_w[p];
            if (i < (uint32_t)tile_rows) acc[i] += w;       // (always true for a well-formed index: keeps a damaged one inside the tile)
        }
        __syncthreads();
    }
}

// keys[0 .. c) -> descending order (bitonic over m = the next power of two >= max(c, 64), the slots in [c, m) zeroed).  The whole block,
// c block-uniform and <= BM25_CAP; earlier writes to keys[] are behind a barrier already; ends with a barrier.
__device__ __forceinline__ void bm25_sort_desc(unsigned long long* keys, int c) {
    const int tid = threadIdx.x;
    int m = 64;
    while (m < c) m <<= 1;
    for (int i = c + tid; i < m; i += BM25_NT) keys[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (m >> 1); t += BM25_NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;          // p < m <= BM25_CAP
                const unsigned long long a = keys[i], b = keys[p];
                if (((i & k) == 0) ? a < b : a > b) { keys[i] = b; keys[p] = a; }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// keys[0 .. c) -> its min(c, n) largest in keys[0 ..), descending, by rounds of a block-wide maximum.  The whole block, c and n
// block-uniform, c <= BM25_CAP; earlier writes to keys[] are behind a barrier already; ends with a barrier.
__device__ __forceinline__ void bm25_select_desc(Bm25List& sm, int c, int n) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int PER = BM25_CAP / BM25_NT;
    unsigned long long k[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) k[j] = (tid + j * BM25_NT < c) ? sm.keys[tid + j * BM25_NT] : 0ull;
    __syncthreads();                                         // every key is in a register before keys[] is rewritten
    const int rounds = c < n ? c : n;                        // the list holds c distinct keys > 0: every round finds one
    for (int r = 0; r < rounds; ++r) {
        unsigned long long m = k[0];
#pragma unroll
        for (int j = 1; j < PER; ++j) m = k[j] > m ? k[j] : m;
        m = wave_max_u64(m);
        if (lane == 0) sm.wred[r & 1][wave] = m;
        __syncthreads();
        unsigned long long g = sm.wred[r & 1][0];
#pragma unroll
        for (int w = 1; w < BM25_NT / 64; ++w) { const unsigned long long v = sm.wred[r & 1][w]; g = v > g ? v : g; }
#pragma unroll
        for (int j = 0; j < PER; ++j) if (k[j] == g) k[j] = 0ull;           // keys are distinct (distinct rows)
        if (tid == 0) sm.keys[r] = g;
    }
    __syncthreads();
}

// cut the list (c keys, any order) back to its n largest, sorted; updates cnt and thr.  The whole block, c uniform; ends with a barrier.
__device__ __forceinline__ void bm25_cut(Bm25List& sm, int c, int n) {
    if (n <= BM25_SELECT_N) bm25_select_desc(sm, c, n);
    else bm25_sort_desc(sm.keys, c);
    if (threadIdx.x == 0) {
        sm.cnt = c < n ? c : n;
        sm.thr = c >= n ? sm.keys[n - 1] : 0ull;
    }
    __syncthreads();
}

__device__ __forceinline__ void bm25_append(Bm25List& sm, unsigned long long key, unsigned long long thr) {
    if (key > thr) {
        const int pos = atomicAdd(&sm.cnt, 1);               // integer slot counter; pos < CAP: the caller cuts before a round that could overflow
        if (pos < BM25_CAP) sm.keys[pos] = key;
    }
}

// FILTERED: allow = uint64 [n_filters][n_words] row bitmaps, filter_of = the bitmap of each query (null: bitmap 0)
// part_k != null: the block's n best keys -> part_k[blocks, nq, n]; null (one block per query): the final (score, id) lists -> out_s / out_i
template <bool FILTERED>
__global__ __launch_bounds__(BM25_NT) void bm25_search_kernel(const long long* __restrict__ term_ptr, const uint32_t* __restrict__ post_row,
                                                              const float* __restrict__ post_w, int vocab, long long n_rows,
                                                              const unsigned long long* __restrict__ allow, int n_filters,
                                                              const int32_t* __restrict__ filter_of, const int32_t* __restrict__ q_terms,
                                                              const int32_t* __restrict__ q_nterms, int n, int tile_rows,
                                                              unsigned long long* __restrict__ part_k, float* __restrict__ out_s,
                                                              long long* __restrict__ out_i, long long idx_base) {
    extern __shared__ __attribute__((aligned(16))) float acc[];               // [tile_rows] f32, then Bm25SearchSmem [, Bm25FilterSmem]
    Bm25SearchSmem& ss = *reinterpret_cast<Bm25SearchSmem*>(acc + tile_rows);
    Bm25List& sm = ss.list;
    const int tid = threadIdx.x, q = blockIdx.y, nq = gridDim.y;
    const int32_t* terms = q_terms + (long long)q * BM25_MAXT;
    int nt = min(max(q_nterms[q], 0), BM25_MAXT);
    [[maybe_unused]] Bm25FilterSmem* fs = nullptr;
    [[maybe_unused]] const unsigned long long* bitmap = nullptr;
    [[maybe_unused]] const long long n_words = (n_rows + 63) >> 6;
    if constexpr (FILTERED) {
        fs = reinterpret_cast<Bm25FilterSmem*>(&ss + 1);
        const int f = filter_of ? filter_of[q] : 0;
        if (f >= 0 && f < n_filters) bitmap = allow + (long long)f * n_words;
        else nt = 0;                                         // no such filter: the query sees no row and nothing is read
    }
    for (int i = tid; i < tile_rows; i += BM25_NT) acc[i] = 0.f;
    if (tid == 0) { sm.cnt = 0; sm.thr = 0ull; }
    __syncthreads();
    const long long n_tiles = (n_rows + tile_rows - 1) / tile_rows;
    for (long long t = blockIdx.x; t < n_tiles && nt > 0; t += gridDim.x) {
        const long long lo = t * tile_rows;
        const long long hi = min(lo + (long long)tile_rows, n_rows);
        if constexpr (FILTERED) {
            // the tile's bitmap words -> LDS (the previous tile's scan ended with a barrier); lo is a multiple of 1024
            unsigned long long w = 0ull;
            if (tid < (tile_rows >> 6)) {                    // tile_rows <= BM25_TILE_MAX: inside fs->bits
                const long long wi = (lo >> 6) + tid;
                if (wi < n_words) {
                    w = bitmap[wi];
                    const long long left = n_rows - (wi << 6);                  // >= 1 rows of this word are inside the shard
                    if (left < 64) w &= ~0ull >> (64 - (int)left);
                }
                fs->bits[tid] = w;
            }
            if (!__syncthreads_or(w != 0ull)) continue;     // no allowed row: no binary searches, no posting reads; acc is still zero
        }
        bm25_accumulate_tile(term_ptr, post_row, post_w, vocab, terms, nt, (uint32_t)lo, (uint32_t)hi, tile_rows, acc, ss.ends);
        const int rows = (int)(hi - lo);
        for (int c0 = 0; c0 < rows; c0 += BM25_CHUNK) {
            const int c = sm.cnt;
            __syncthreads();                                 // everyone has read cnt before anyone appends
            if (c + BM25_CHUNK > BM25_CAP) bm25_cut(sm, c < BM25_CAP ? c : BM25_CAP, n);
            const unsigned long long thr = sm.thr;
            const int i = c0 + 2 * tid;                      // tile_rows is even and acc is zero beyond `rows`
            if (i < tile_rows) {
                const float2 v = *reinterpret_cast<const float2*>(acc + i);
                *reinterpret_cast<float2*>(acc + i) = make_float2(0.f, 0.f);
                const float s[2] = {v.x, v.y};
                [[maybe_unused]] unsigned int ok = 3u;      // the two rows' bits: i is even, so both lie in one bitmap word
                if constexpr (FILTERED) ok = (unsigned int)(fs->bits[i >> 6] >> (i & 63)) & 3u;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (s[e] > 0.f && (!FILTERED || ((ok >> e) & 1u)))
                        bm25_append(sm, ((unsigned long long)__float_as_uint(s[e]) << 32) |
                                            (unsigned long long)(0xffffffffu - (uint32_t)(lo + i + e)), thr);
                }
            }
            __syncthreads();
        }
    }
    bm25_cut(sm, sm.cnt < BM25_CAP ? sm.cnt : BM25_CAP, n);
    for (int r = tid; r < n; r += BM25_NT) {
        const unsigned long long key = r < sm.cnt ? sm.keys[r] : 0ull;
        if (part_k) {
            part_k[((long long)blockIdx.x * nq + q) * n + r] = key;
        } else {
            out_s[(long long)q * n + r] = key ? __uint_as_float((uint32_t)(key >> 32)) : -INFINITY;
            out_i[(long long)q * n + r] = key ? (long long)(0xffffffffu - (uint32_t)key) + idx_base : -1ll;
        }
    }
}

// one block per query: the parts * n keys of the query's partial lists -> its n largest, as (score, id)
__global__ __launch_bounds__(BM25_NT) void bm25_merge_kernel(const unsigned long long* __restrict__ part_k, int parts, int nq, int n,
                                                             float* __restrict__ out_s, long long* __restrict__ out_i, long long idx_base) {
    __shared__ Bm25List sm;
    const int tid = threadIdx.x, q = blockIdx.x;
    if (tid == 0) { sm.cnt = 0; sm.thr = 0ull; }
    __syncthreads();
    const int total = parts * n;                             // <= Bm25Limits::part_keys
    for (int e0 = 0; e0 < total; e0 += BM25_CHUNK) {         // block-uniform
        const int c = sm.cnt;
        __syncthreads();                                     // everyone has read cnt before anyone appends
        if (c + BM25_CHUNK > BM25_CAP) bm25_cut(sm, c < BM25_CAP ? c : BM25_CAP, n);
        const unsigned long long thr = sm.thr;
#pragma unroll
        for (int u = 0; u < BM25_CHUNK / BM25_NT; ++u) {
            const int e = e0 + u * BM25_NT + tid;
            if (e < total) {
                const int p = e / n, r = e - p * n;
                bm25_append(sm, part_k[((long long)p * nq + q) * n + r], thr);           // (thr >= 0: an empty slot is never appended)
            }
        }
        __syncthreads();
    }
    bm25_cut(sm, sm.cnt < BM25_CAP ? sm.cnt : BM25_CAP, n);
    for (int r = tid; r < n; r += BM25_NT) {
        const unsigned long long key = r < sm.cnt ? sm.keys[r] : 0ull;
        out_s[(long long)q * n + r] = key ? __uint_as_float((uint32_t)(key >> 32)) : -INFINITY;
        out_i[(long long)q * n + r] = key ? (long long)(0xffffffffu - (uint32_t)key) + idx_base : -1ll;
    }
}

// debug tap: the dense score row of ONE query for rows [row_lo, row_hi), one tile per block, through the same accumulation
__global__ __launch_bounds__(BM25_NT) void bm25_scores_kernel(const long long* __restrict__ term_ptr, const uint32_t* __restrict__ post_row,
                                                              const float* __restrict__ post_w, int vocab, const int32_t* __restrict__ terms,
                                                              int nt, long long row_lo, long long row_hi, int tile_rows, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float acc[];               // [tile_rows] f32, then the block's Bm25Ends (all dynamic LDS)
    Bm25Ends& sm = *reinterpret_cast<Bm25Ends*>(acc + tile_rows);
    const int tid = threadIdx.x;
    for (int i = tid; i < tile_rows; i += BM25_NT) acc[i] = 0.f;
    __syncthreads();
    const long long lo = row_lo + (long long)blockIdx.x * tile_rows;
    const long long hi = min(lo + (long long)tile_rows, row_hi);
    bm25_accumulate_tile(term_ptr, post_row, post_w, vocab, terms, nt, (uint32_t)lo, (uint32_t)hi, tile_rows, acc, sm);
    for (int i = tid; i < (int)(hi - lo); i += BM25_NT) out[lo - row_lo + i] = acc[i];
}

int bm25_default_tile(int64_t n_rows) {
    // small shards: one tile that just covers them (less LDS to clear and scan); large ones: the largest tile two blocks per CU allow
    const int64_t need = round_up64(n_rows, BM25_CHUNK);
    return (int)(need < BM25_TILE ? need : BM25_TILE);
}

int bm25_blocks(Bm25Limits lim, int64_t n_rows, int tile_rows, int n, int max_blocks) {
    const int64_t tiles = (n_rows + tile_rows - 1) / tile_rows;
    int64_t b = lim.part_keys / n;
    if (b > 512) b = 512;
    if (max_blocks > 0 && b > max_blocks) b = max_blocks;
    return (int)(tiles < b ? tiles : b);
}

int64_t bm25_workspace_bytes(Bm25Limits lim, int64_t n_rows, int32_t n_queries, int32_t n) {
    if (n_rows <= 0 || n_queries <= 0 || n < 1 || n > lim.n_max) return -1;
    // sized for the smallest tile a tuned call may ask for, so that one workspace serves every tile size / block count
    return round_up64((int64_t)bm25_blocks(lim, n_rows, BM25_CHUNK, n, 0) * n_queries * n * 8, 256);
}

// every top-n export: the checks, bm25_search_kernel<filtered> and, with more than one block per query, the merge
int32_t bm25_search_launch(Bm25Limits lim, bool filtered, const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab,
                           int64_t n_rows, const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const int32_t* q_terms,
                           const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores, int64_t* out_ids, int64_t idx_base, void* ws,
                           int64_t ws_bytes, int32_t tile_rows, int32_t max_blocks, void* stream) {
    ARX_REQUIRE(term_ptr && post_row && post_w && q_terms && q_nterms && out_scores && out_ids, "null pointer argument");
    if (filtered) {
        ARX_REQUIRE(allow, "allow must not be null (one row bitmap per filter)");
        ARX_REQUIRE(n_filters >= 1, "n_filters=%d must be at least 1", n_filters);
    } else {
        ARX_REQUIRE(!filter_of, "filter_of needs allow (allow == NULL is the unfiltered search)");
    }
    ARX_REQUIRE(vocab > 0, "vocab=%d must be positive", vocab);
    ARX_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "n_rows=%lld must be in [1, 2^31)", (long long)n_rows);
    ARX_REQUIRE(n_queries > 0 && n_queries <= 65535, "n_queries=%d must be in [1, 65535]", n_queries);
    ARX_REQUIRE(n >= 1 && n <= lim.n_max, "n=%d must be in [1, %d]", n, lim.n_max);
    ARX_REQUIRE(idx_base >= 0, "idx_base must be >= 0");
    ARX_REQUIRE(max_blocks >= 0, "max_blocks must be >= 0 (0 = default)");
    if (tile_rows == 0) tile_rows = bm25_default_tile(n_rows);
    ARX_REQUIRE(tile_rows >= BM25_CHUNK && tile_rows <= BM25_TILE_MAX && tile_rows % BM25_CHUNK == 0,
                "tile_rows=%d must be a multiple of %d in [%d, %d] (0 = default)", tile_rows, BM25_CHUNK, BM25_CHUNK, BM25_TILE_MAX);
    const int blocks = bm25_blocks(lim, n_rows, tile_rows, n, max_blocks);
    const int64_t need = bm25_workspace_bytes(lim, n_rows, n_queries, n);
    ARX_REQUIRE(blocks == 1 || (ws && ws_bytes >= need), "workspace too small: %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const int smem = tile_rows * 4 + (int)sizeof(Bm25SearchSmem) + (filtered ? (int)sizeof(Bm25FilterSmem) : 0);
    const auto kernel = filtered ? bm25_search_kernel<true> : bm25_search_kernel<false>;
    ARX_HIP_CHECK(arx_func_smem((const void*)kernel, smem));
    unsigned long long* part_k = blocks > 1 ? (unsigned long long*)ws : nullptr;
    kernel<<<dim3(blocks, n_queries), BM25_NT, smem, st>>>((const long long*)term_ptr, post_row, post_w, vocab, n_rows,
                                                           (const unsigned long long*)allow, n_filters, filter_of, q_terms, q_nterms, n, tile_rows,
                                                           part_k, out_scores, (long long*)out_ids, idx_base);
    ARX_HIP_CHECK(hipGetLastError());
    if (blocks > 1) {
        bm25_merge_kernel<<<n_queries, BM25_NT, 0, st>>>(part_k, blocks, n_queries, n, out_scores, (long long*)out_ids, idx_base);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}

}  // namespace

extern "C" int64_t arx_bm25_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n) {
    return bm25_workspace_bytes(BM25_NARROW, n_rows, n_queries, n);
}

extern "C" int64_t arx_bm25_wide_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n) {
    return bm25_workspace_bytes(BM25_WIDE, n_rows, n_queries, n);
}

extern "C" int32_t arx_bm25_search_tuned(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                                         const int32_t* q_terms, const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores,
                                         int64_t* out_ids, int64_t idx_base, void* ws, int64_t ws_bytes, int32_t tile_rows, int32_t max_blocks,
                                         void* stream) {
    return bm25_search_launch(BM25_NARROW, false, term_ptr, post_row, post_w, vocab, n_rows, nullptr, 0, nullptr, q_terms, q_nterms, n_queries, n,
                              out_scores, out_ids, idx_base, ws, ws_bytes, tile_rows, max_blocks, stream);
}

extern "C" int32_t arx_bm25_search(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                                   const int32_t* q_terms, const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores,
                                   int64_t* out_ids, int64_t idx_base, void* ws, int64_t ws_bytes, void* stream) {
    return arx_bm25_search_tuned(term_ptr, post_row, post_w, vocab, n_rows, q_terms, q_nterms, n_queries, n, out_scores, out_ids, idx_base,
                                 ws, ws_bytes, 0, 0, stream);
}

extern "C" int32_t arx_bm25_search_filtered_tuned(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab,
                                                  int64_t n_rows, const uint64_t* allow, int32_t n_filters, const int32_t* filter_of,
                                                  const int32_t* q_terms, const int32_t* q_nterms, int32_t n_queries, int32_t n,
                                                  float* out_scores, int64_t* out_ids, int64_t idx_base, void* ws, int64_t ws_bytes,
                                                  int32_t tile_rows, int32_t max_blocks, void* stream) {
    return bm25_search_launch(BM25_NARROW, true, term_ptr, post_row, post_w, vocab, n_rows, allow, n_filters, filter_of, q_terms, q_nterms,
                              n_queries, n, out_scores, out_ids, idx_base, ws, ws_bytes, tile_rows, max_blocks, stream);
}

extern "C" int32_t arx_bm25_search_filtered(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                                            const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const int32_t* q_terms,
                                            const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores, int64_t* out_ids,
                                            int64_t idx_base, void* ws, int64_t ws_bytes, void* stream) {
    return arx_bm25_search_filtered_tuned(term_ptr, post_row, post_w, vocab, n_rows, allow, n_filters, filter_of, q_terms, q_nterms, n_queries, n,
                                          out_scores, out_ids, idx_base, ws, ws_bytes, 0, 0, stream);
}

// allow == NULL is the unfiltered search
extern "C" int32_t arx_bm25_search_wide(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                                        const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const int32_t* q_terms,
                                        const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores, int64_t* out_ids,
                                        int64_t idx_base, void* ws, int64_t ws_bytes, int32_t tile_rows, int32_t max_blocks, void* stream) {
    return bm25_search_launch(BM25_WIDE, allow != nullptr, term_ptr, post_row, post_w, vocab, n_rows, allow, n_filters, filter_of, q_terms,
                              q_nterms, n_queries, n, out_scores, out_ids, idx_base, ws, ws_bytes, tile_rows, max_blocks, stream);
}

extern "C" int32_t arx_bm25_scores(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                                   const int32_t* q_terms, int32_t n_terms, int64_t row_lo, int64_t row_hi, int32_t tile_rows, float* out,
                                   void* stream) {
    ARX_REQUIRE(term_ptr && post_row && post_w && out && (q_terms || n_terms == 0), "null pointer argument");
    ARX_REQUIRE(vocab > 0, "vocab=%d must be positive", vocab);
    ARX_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "n_rows=%lld must be in [1, 2^31)", (long long)n_rows);
    ARX_REQUIRE(n_terms >= 0 && n_terms <= BM25_MAXT, "n_terms=%d must be in [0, %d]", n_terms, BM25_MAXT);
    ARX_REQUIRE(0 <= row_lo && row_lo < row_hi && row_hi <= n_rows, "row range [%lld, %lld) outside [0, %lld)", (long long)row_lo,
                (long long)row_hi, (long long)n_rows);
    if (tile_rows == 0) tile_rows = bm25_default_tile(row_hi - row_lo);
    ARX_REQUIRE(tile_rows >= BM25_CHUNK && tile_rows <= BM25_TILE_MAX && tile_rows % BM25_CHUNK == 0,
                "tile_rows=%d must be a multiple of %d in [%d, %d] (0 = default)", tile_rows, BM25_CHUNK, BM25_CHUNK, BM25_TILE_MAX);
    const int64_t blocks = (row_hi - row_lo + tile_rows - 1) / tile_rows;
    const int smem = tile_rows * 4 + (int)sizeof(Bm25Ends);
    ARX_HIP_CHECK(arx_func_smem((const void*)bm25_scores_kernel, smem));
    bm25_scores_kernel<<<(int)blocks, BM25_NT, smem, (hipStream_t)stream>>>((const long long*)term_ptr, post_row, post_w, vocab, q_terms, n_terms,
                                                                            row_lo, row_hi, tile_rows, out);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
