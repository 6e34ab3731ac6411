// arx_graph_search: beam search over a fixed-degree k-NN graph, exact scores (gfx950; C ABI in include/arx.h; the host layer and the
// numpy restatement are arxiv_rag_amd/graph.py; the definition is INTEGRATION.md "Graph search").  arx_graph_link and arx_graph_remap,
// which keep a built graph usable across added and compacted rows, are further down with their own notes.
//
// One block per query, every bit of state in LDS, so a query's answer cannot depend on its batch:
//   qs        the fp16 query row.
//   tab       the visited set: an open-addressing table of GRAPH_SLOTS int32 rows (-1 = empty), linear probing from a multiplicative
//             hash.  A row enters by an integer LDS compare-and-swap, so of two lanes that offer one row exactly one wins; these are the
//             kernel's only atomics.  A call can insert at most n_entries + max_iters * degree rows, and the host refuses a call where
//             that exceeds GRAPH_ROWS_MAX = GRAPH_SLOTS / 2: the table never fills and never drops a row.
//   beam      at most ef 64-bit keys, sorted descending, with an "expanded" mark each; two buffers, a merge reads one and writes the other.
//             A key is  order word of the f32 score << 32 | (0xffffffff - row)  (key_lists.h's convention): larger is better, distinct
//             rows give distinct keys, 0 is an empty slot.  A NaN score has order word 0, below -inf's 0x007fffff.
// A step (the start: the entries; then one per iteration: the neighbours of the parent, the best beam row not yet expanded):
//   1  every wave finds the parent by ballots over the marks (the same answer in every wave; no write, so no barrier).  Wave 0 reads
//      the at most 64 candidate rows, drops those outside [0, n_rows), inserts the others into tab and compacts the winners.  barrier
//   2  eight lanes score a row (exact_row_score), blockDim / 8 rows per pass, and write its key; with `allow`, the key again in a
//      second array if the row's bit is set, else 0.                                                                          barrier
//   3  every wave sorts the at most 64 new keys by a bitonic network over its lanes (shuffles) into a copy of its own, then the block
//      merges by rank: a key's slot is its index in its own list plus the number of keys of the other list above it (a binary
//      search); slots at or past ef are dropped.  Wave 0 merges the allowed keys into the k-wide second list the same way.    barrier
// Three barriers a step; no block-wide sort.  The answer is the first k beam keys, or with `allow` the second list.
// Not measured: the shape of a step.  Wave 0 alone reads the neighbour list, so one dependent global load (parent key in LDS -> its
// neighbour row -> the compare-and-swaps -> barrier) sits in front of the row gathers instead of under them, and a step has three
// barriers where two would do with the inserts spread over the block.  Both keep the bits fixed and the code short; what they cost per
// iteration has not been timed (tools/graph_bench.py times whole calls).
#include <math.h>

#include "arx_common.h"

namespace {
#include "exact_score.h"

constexpr int GRAPH_SLOTS = 16384;              // 64 KiB of LDS: with a 768-d query and the lists below a block takes 78.8 KiB, two fit a CU
constexpr int GRAPH_ROWS_MAX = GRAPH_SLOTS / 2; // rows a call may insert: a load factor of at most one half
constexpr int GRAPH_EF_MAX = 512, GRAPH_K_MAX = 32, GRAPH_DEGREE_MAX = 64, GRAPH_ENTRIES_MAX = 64, GRAPH_ITERS_MAX = 1024;
constexpr int GRAPH_NT_MAX = 256, GRAPH_NW_MAX = GRAPH_NT_MAX / 64;
typedef unsigned long long u64;

struct GraphSm {
    int32_t tab[GRAPH_SLOTS];
    u64 beam[2][GRAPH_EF_MAX];
    u64 sorted[GRAPH_NW_MAX][64];               // a wave's sorted copy of the new keys
    u64 fresh[64], fresh_ok[64];                // the new keys in candidate order; the same where the row is allowed, else 0
    u64 best[2][GRAPH_K_MAX];                   // with allow: the k best allowed keys seen
    u64 sorted_ok[64];
    int32_t cand[64];
    uint8_t done[2][GRAPH_EF_MAX];              // the expanded marks of beam[.]
    int32_t n_cand;
};

__device__ __forceinline__ uint32_t graph_order_word(float v) {
    if (v != v) return 0u;                                       // NaN: below every number
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float graph_word_score(uint32_t w) {
    if (w == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((w & 0x80000000u) ? (w & 0x7fffffffu) : ~w);
}
// the number of keys of list[0 .. n) (sorted descending, distinct) above `key`
__device__ __forceinline__ int graph_above(const u64* list, int n, u64 key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] > key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// one wave: lane l's key -> the l-th largest of the wave's 64 keys
__device__ __forceinline__ u64 graph_wave_sort(u64 v, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 o = __shfl_xor(v, j);
            const bool keep_max = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_max ? (v > o ? v : o) : (v < o ? v : o);
        }
    return v;
}

__global__ __launch_bounds__(GRAPH_NT_MAX) void graph_search_kernel(const f16_t* __restrict__ C, int64_t n_rows, int D,
                                                                     const int32_t* __restrict__ nbr, int degree, const f16_t* __restrict__ Q,
                                                                     const int32_t* __restrict__ entries, int n_entries,
                                                                     const uint64_t* __restrict__ allow, int k, int ef, int max_iters,
                                                                     float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                                     int64_t* __restrict__ out_scored, int64_t* __restrict__ out_expanded,
                                                                     int64_t idx_base) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    GraphSm& sm = *reinterpret_cast<GraphSm*>(smem + (size_t)D * 2);          // (D % 64 == 0: 128-byte aligned)
    const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6;
    const int nch = D >> 3, l8 = lane & 7, oct = tid >> 3, n_oct = nt >> 3;
    for (int i = tid; i < nch; i += nt) reinterpret_cast<u32x4*>(qs)[i] = reinterpret_cast<const u32x4*>(Q + (int64_t)q * D)[i];
    for (int i = tid; i < GRAPH_SLOTS; i += nt) sm.tab[i] = -1;
    if (tid < GRAPH_K_MAX) sm.best[0][tid] = 0ull;
    __syncthreads();
    int cur = 0, len = 0, n_best = 0, bcur = 0;                   // block-uniform (n_best, bcur: wave 0's)
    int64_t scored = 0, expanded = 0;
    for (int it = -1; it < max_iters; ++it) {                    // it = -1: the start
        // ---- 1: the parent (every wave), its neighbours into the visited set (wave 0)
        int parent = -1;
        if (it >= 0) {
            for (int b = 0; b < len; b += 64) {
                const u64 open = __ballot(b + lane < len && sm.done[cur][b + lane] == 0);
                if (open) { parent = b + __ffsll((long long)open) - 1; break; }
            }
            if (parent < 0) break;                               // block-uniform: every wave read the same marks
            ++expanded;
        }
        if (w == 0) {
            int32_t r = -1;
            if (it < 0) {
                if (lane < n_entries) r = entries[(int64_t)q * n_entries + lane];
            } else if (lane < degree) {
                const int64_t prow = (int64_t)(0xffffffffu - (uint32_t)sm.beam[cur][parent]);          // a beam row: inside [0, n_rows)
                r = nbr[prow * degree + lane];
            }
            bool fresh = false;
            if (r >= 0 && r < n_rows) {
                uint32_t s = ((uint32_t)r * 0x9E3779B1u) >> 18;                                         // 14 bits: GRAPH_SLOTS
                for (;;) {                                       // ends: the table is at most half full (the host's capacity rule)
                    const int32_t old = atomicCAS(&sm.tab[s], -1, r);
                    if (old == -1) { fresh = true; break; }
                    if (old == r) break;
                    s = (s + 1) & (GRAPH_SLOTS - 1);
                }
            }
            const u64 won = __ballot(fresh);
            if (fresh) sm.cand[__popcll(won & ((1ull << lane) - 1ull))] = r;
            if (lane == 0) sm.n_cand = __popcll(won);
        }
        __syncthreads();
        // ---- 2: score the new rows, eight lanes each
        const int n_cand = sm.n_cand;
        scored += n_cand;
        for (int c0 = 0; c0 < n_cand; c0 += n_oct) {             // wave-uniform bounds: every lane of an octet reaches the shuffles
            const int c = c0 + oct;
            const bool ok = c < n_cand;
            const int64_t row = ok ? sm.cand[c] : 0;
            bool vis = false;
            if (ok && allow) vis = (allow[row >> 6] >> (row & 63)) & 1ull;
            const float a = exact_row_score(C + row * D, qs, nch, l8, ok);
            if (ok && l8 == 0) {
                const u64 key = ((u64)graph_order_word(a) << 32) | (u64)(0xffffffffu - (uint32_t)row);
                sm.fresh[c] = key;
                sm.fresh_ok[c] = vis ? key : 0ull;
            }
        }
        if (tid < 64 && tid >= n_cand) { sm.fresh[tid] = 0ull; sm.fresh_ok[tid] = 0ull; }
        __syncthreads();
        // ---- 3: sort the new keys (every wave its own copy), merge by rank into the other beam buffer
        // (the write and the reads of `mine` below are ordered by the wave alone: all 64 lanes must reach this store together, so it must
        // stay outside any divergent branch; the same holds for sorted_ok further down)
        u64* mine = sm.sorted[w];
        mine[lane] = graph_wave_sort(sm.fresh[lane], lane);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const u64* old_b = sm.beam[cur];
        u64* new_b = sm.beam[cur ^ 1];
        for (int i = tid; i < len; i += nt) {
            const u64 key = old_b[i];
            const int pos = i + graph_above(mine, n_cand, key);
            if (pos < ef) { new_b[pos] = key; sm.done[cur ^ 1][pos] = (i == parent) ? 1 : sm.done[cur][i]; }
        }
        for (int j = tid; j < n_cand; j += nt) {
            const u64 key = mine[j];
            const int pos = j + graph_above(old_b, len, key);
            if (pos < ef) { new_b[pos] = key; sm.done[cur ^ 1][pos] = 0; }
        }
        if (allow && w == 0) {                                   // the k best allowed keys: wave 0 alone, in its own lists
            sm.sorted_ok[lane] = graph_wave_sort(sm.fresh_ok[lane], lane);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int n_ok = __popcll(__ballot(sm.sorted_ok[lane] != 0ull));
            const u64* ob = sm.best[bcur];
            u64* nb = sm.best[bcur ^ 1];
            if (lane < n_best) {
                const u64 key = ob[lane];
                const int pos = lane + graph_above(sm.sorted_ok, n_ok, key);
                if (pos < k) nb[pos] = key;
            }
            if (lane < n_ok) {
                const u64 key = sm.sorted_ok[lane];
                const int pos = lane + graph_above(ob, n_best, key);
                if (pos < k) nb[pos] = key;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            n_best = n_best + n_ok < k ? n_best + n_ok : k;
            bcur ^= 1;
        }
        len = len + n_cand < ef ? len + n_cand : ef;
        cur ^= 1;
        __syncthreads();
    }
    if (w == 0) {                                                // (wave 0 wrote best[] itself; the beam is behind the loop's last barrier)
        const u64* res = allow ? sm.best[bcur] : sm.beam[cur];
        const int n_res = allow ? n_best : (len < k ? len : k);
        if (lane < k) {
            const u64 key = lane < n_res ? res[lane] : 0ull;
            out_s[(int64_t)q * k + lane] = key ? graph_word_score((uint32_t)(key >> 32)) : -INFINITY;
            out_i[(int64_t)q * k + lane] = key ? (int64_t)(0xffffffffu - (uint32_t)key) + idx_base : -1;
        }
        if (lane == 0) {
            if (out_scored) out_scored[q] = scored;
            if (out_expanded) out_expanded[q] = expanded;
        }
    }
}

// ---- arx_graph_link: offer rows to the tails of other rows' neighbour lists (include/arx.h; INTEGRATION.md "Graph search") ---------
// One block per target slot; a slot that passes the checks below is the only writer of its row, so plain stores, no atomics and no
// workspace.  The row t is the query (staged in LDS); its head, neighbors[t][0:H], is never written.  The candidates are a stream:
// the H entries of the old tail, then the slot's offers, 64 at a time:
//   1  wave 0 reads the chunk, drops what is outside [0, n_rows), t itself and the head's rows, compacts the rest.        barrier
//   2  eight lanes score a row (exact_row_score), blockDim / 8 rows per pass, and write its key.                          barrier
//   3  wave 0 sorts the keys (the search's bitonic network), drops a key equal to its left neighbour or already in the running
//      tail (one row always gives one key: that is the whole de-duplication, there is no visited set), and merges the rest by rank
//      into the other of the two H-wide tail buffers.
// The tail is the H largest keys of a set, so it depends neither on the chunking nor on the block size.
struct LinkSm {
    u64 best[2][GRAPH_DEGREE_MAX / 2];          // the running tail, sorted descending; two buffers as for the beam
    u64 fresh[64], uniq[64];
    int32_t head[GRAPH_DEGREE_MAX / 2];
    int32_t cand[64];
    int32_t red[GRAPH_NW_MAX];
    int32_t n_cand;
};

__global__ __launch_bounds__(GRAPH_NT_MAX) void graph_link_kernel(const f16_t* __restrict__ C, int64_t n_rows, int D, int32_t* nbr, int degree,
                                                                   const int32_t* __restrict__ targets, const int32_t* __restrict__ offer_start,
                                                                   const int32_t* __restrict__ offers, int64_t n_offers) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    LinkSm& sm = *reinterpret_cast<LinkSm*>(smem + (size_t)D * 2);
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6;
    const int nch = D >> 3, l8 = lane & 7, oct = tid >> 3, n_oct = nt >> 3, H = degree >> 1;
    const int64_t t = targets[s];
    const int64_t o0 = offer_start[s], o1 = offer_start[s + 1];
    if (t < 0 || t >= n_rows || o0 < 0 || o1 < o0 || o1 > n_offers) return;          // (block-uniform, as every return below)
    // the largest valid target of the slots before this one: a slot at or below it is skipped, so no two blocks ever write one row
    int32_t before = -1;
    for (int i = tid; i < s; i += nt) {
        const int32_t v = targets[i];
        if (v < n_rows) before = max(before, v);                 // (a negative one cannot raise it)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before = max(before, __shfl_xor(before, o));
    if (lane == 0) sm.red[w] = before;
    __syncthreads();
    for (int i = 0; i < (nt >> 6); ++i) before = max(before, sm.red[i]);
    if (t <= before) return;
    for (int i = tid; i < nch; i += nt) reinterpret_cast<u32x4*>(qs)[i] = reinterpret_cast<const u32x4*>(C + t * D)[i];
    if (tid < H) sm.head[tid] = nbr[t * degree + tid];
    __syncthreads();
    const int total = H + (int)(o1 - o0);
    int cur = 0, n_best = 0;                                     // (wave 0's)
    for (int c0 = 0; c0 < total; c0 += 64) {
        // ---- 1: the chunk's candidates (wave 0)
        if (w == 0) {
            const int j = c0 + lane;
            int32_t r = -1;
            if (j < total) r = j < H ? nbr[t * degree + H + j] : offers[o0 + (j - H)];
            bool ok = r >= 0 && r < n_rows && r != t;
            for (int i = 0; i < H; ++i) ok = ok && sm.head[i] != r;
            const u64 in = __ballot(ok);
            if (ok) sm.cand[__popcll(in & ((1ull << lane) - 1ull))] = r;
            if (lane == 0) sm.n_cand = __popcll(in);
        }
        __syncthreads();
        // ---- 2: score them, eight lanes each
        const int n_cand = sm.n_cand;
        for (int b0 = 0; b0 < n_cand; b0 += n_oct) {             // wave-uniform bounds: every lane of an octet reaches the shuffles
            const int c = b0 + oct;
            const bool ok = c < n_cand;
            const int64_t row = ok ? sm.cand[c] : 0;
            const float a = exact_row_score(C + row * D, qs, nch, l8, ok);
            if (ok && l8 == 0) sm.fresh[c] = ((u64)graph_order_word(a) << 32) | (u64)(0xffffffffu - (uint32_t)row);
        }
        if (tid < 64 && tid >= n_cand) sm.fresh[tid] = 0ull;
        __syncthreads();
        // ---- 3: sort, drop the repeats, merge by rank (wave 0; the next chunk's step 1 is wave 0's too, so no barrier follows)
        if (w == 0) {
            const u64 key = graph_wave_sort(sm.fresh[lane], lane);
            const u64 left = __shfl_up(key, 1);
            const u64* ob = sm.best[cur];
            u64* nb = sm.best[cur ^ 1];
            bool fresh = key != 0ull && (lane == 0 || key != left);
            if (fresh) {
                const int p = graph_above(ob, n_best, key);
                fresh = !(p < n_best && ob[p] == key);
            }
            const u64 in = __ballot(fresh);
            const int n_new = __popcll(in);
            if (fresh) sm.uniq[__popcll(in & ((1ull << lane) - 1ull))] = key;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane < n_best) {
                const u64 k0 = ob[lane];
                const int pos = lane + graph_above(sm.uniq, n_new, k0);
                if (pos < H) nb[pos] = k0;
            }
            if (lane < n_new) {
                const u64 k1 = sm.uniq[lane];
                const int pos = lane + graph_above(ob, n_best, k1);
                if (pos < H) nb[pos] = k1;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            n_best = n_best + n_new < H ? n_best + n_new : H;
            cur ^= 1;
        }
    }
    if (w == 0 && lane < H) nbr[t * degree + H + lane] = lane < n_best ? (int32_t)(0xffffffffu - (uint32_t)sm.best[cur][lane]) : -1;
}

// ---- arx_graph_remap: renumber the moved neighbour rows of a stable compaction.  A wave per row, a lane per entry: every lane has
// read its entry before the ballot that places the survivors, so the row is rewritten in place with plain stores.
__global__ __launch_bounds__(GRAPH_NT_MAX) void graph_remap_kernel(int32_t* nbr, int64_t count, int degree, const unsigned long long* __restrict__ keep,
                                                                    const long long* __restrict__ word_rank, int64_t n_old) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * GRAPH_NW_MAX + (threadIdx.x >> 6);
    if (r >= count) return;                                      // (wave-uniform)
    int64_t e = -1;
    if (lane < degree) e = nbr[r * degree + lane];
    bool ok = false;
    if (e >= 0 && e < n_old) {
        const unsigned long long kw = keep[e >> 6];
        if ((kw >> (e & 63)) & 1ull) {
            e = word_rank[e >> 6] + __popcll(kw & ((1ull << (e & 63)) - 1ull));
            ok = e >= 0 && e < count;                            // (false only for a plan that is not this bitmap's)
        }
    }
    const u64 in = __ballot(ok);
    const int n_ok = __popcll(in);
    if (ok) nbr[r * degree + __popcll(in & ((1ull << lane) - 1ull))] = (int32_t)e;
    if (lane >= n_ok && lane < degree) nbr[r * degree + lane] = -1;
}

bool graph_shape_ok(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t degree, int32_t k, int32_t ef, int32_t max_iters, int32_t n_entries) {
    return n_rows > 0 && n_rows < (1ll << 31) && n_queries > 0 && dim > 0 && dim % 64 == 0 && dim <= 8192 && degree >= 8 &&
           degree <= GRAPH_DEGREE_MAX && degree % 8 == 0 && k >= 1 && k <= GRAPH_K_MAX && ef >= k && ef <= GRAPH_EF_MAX && max_iters >= 1 &&
           max_iters <= GRAPH_ITERS_MAX && n_entries >= 1 && n_entries <= GRAPH_ENTRIES_MAX &&
           (int64_t)n_entries + (int64_t)max_iters * degree <= GRAPH_ROWS_MAX;
}
constexpr int64_t GRAPH_WS_BYTES = 256;         // the search keeps its state in LDS: the workspace is not written
}      // namespace

extern "C" int64_t arx_graph_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t degree, int32_t k, int32_t ef,
                                             int32_t max_iters, int32_t n_entries) {
    return graph_shape_ok(n_rows, n_queries, dim, degree, k, ef, max_iters, n_entries) ? GRAPH_WS_BYTES : -1;
}

extern "C" int32_t arx_graph_search_tuned(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* neighbors, int32_t degree,
                                          const void* queries, int32_t n_queries, const int32_t* entries, int32_t n_entries,
                                          const uint64_t* allow, int32_t k, int32_t ef, int32_t max_iters, float* out_scores, int64_t* out_ids,
                                          int64_t* out_scored, int64_t* out_expanded, int64_t idx_base, void* ws, int64_t ws_bytes,
                                          int32_t threads, void* stream) {
    ARX_REQUIRE(k >= 1 && k <= GRAPH_K_MAX, "k=%d out of range 1..%d", k, GRAPH_K_MAX);
    ARX_REQUIRE(ef >= k && ef <= GRAPH_EF_MAX, "ef=%d out of range k..%d", ef, GRAPH_EF_MAX);
    ARX_REQUIRE(max_iters >= 1 && max_iters <= GRAPH_ITERS_MAX, "max_iters=%d out of range 1..%d", max_iters, GRAPH_ITERS_MAX);
    ARX_REQUIRE(degree >= 8 && degree <= GRAPH_DEGREE_MAX && degree % 8 == 0, "degree=%d must be a multiple of 8 in 8..%d", degree, GRAPH_DEGREE_MAX);
    ARX_REQUIRE(n_entries >= 1 && n_entries <= GRAPH_ENTRIES_MAX, "n_entries=%d out of range 1..%d", n_entries, GRAPH_ENTRIES_MAX);
    ARX_REQUIRE((int64_t)n_entries + (int64_t)max_iters * degree <= GRAPH_ROWS_MAX,
                "n_entries + max_iters * degree = %lld exceeds the visited table's %d rows", (long long)n_entries + (long long)max_iters * degree,
                GRAPH_ROWS_MAX);
    ARX_REQUIRE(dim > 0 && dim % 64 == 0 && dim <= 8192, "dim=%d must be a multiple of 64, at most 8192", dim);
    ARX_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 1..2^31-1", (long long)n_rows);
    ARX_REQUIRE(n_queries > 0, "n_queries=%d: empty query set", n_queries);
    ARX_REQUIRE(threads == 0 || threads == 64 || threads == 128 || threads == 256, "threads=%d: 0 (default), 64, 128 or 256", threads);
    ARX_REQUIRE(corpus && neighbors && queries && entries && out_scores && out_ids && ws, "null pointer argument");
    ARX_REQUIRE(((uintptr_t)corpus | (uintptr_t)queries) % 16 == 0, "corpus and queries must be 16-byte aligned");
    ARX_REQUIRE(ws_bytes >= GRAPH_WS_BYTES, "workspace too small: %lld < %lld (arx_graph_workspace_bytes)", (long long)ws_bytes,
                (long long)GRAPH_WS_BYTES);
    if (threads == 0) threads = degree > 16 ? 256 : 128;          // 32 rows scored per pass; a sparser graph leaves half of that idle
    const int smem = dim * 2 + (int)sizeof(GraphSm);
    ARX_HIP_CHECK(arx_func_smem((const void*)graph_search_kernel, smem));
    graph_search_kernel<<<n_queries, threads, smem, (hipStream_t)stream>>>((const f16_t*)corpus, n_rows, dim, neighbors, degree,
                                                                          (const f16_t*)queries, entries, n_entries, allow, k, ef, max_iters,
                                                                          out_scores, out_ids, out_scored, out_expanded, idx_base);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_graph_search(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* neighbors, int32_t degree,
                                    const void* queries, int32_t n_queries, const int32_t* entries, int32_t n_entries, const uint64_t* allow,
                                    int32_t k, int32_t ef, int32_t max_iters, float* out_scores, int64_t* out_ids, int64_t* out_scored,
                                    int64_t* out_expanded, int64_t idx_base, void* ws, int64_t ws_bytes, void* stream) {
    return arx_graph_search_tuned(corpus, n_rows, dim, neighbors, degree, queries, n_queries, entries, n_entries, allow, k, ef, max_iters,
                                  out_scores, out_ids, out_scored, out_expanded, idx_base, ws, ws_bytes, 0, stream);
}

extern "C" int32_t arx_graph_link_tuned(const void* corpus, int64_t n_rows, int32_t dim, int32_t* neighbors, int32_t degree, const int32_t* targets,
                                        int32_t n_targets, const int32_t* offer_start, const int32_t* offers, int64_t n_offers, int32_t threads,
                                        void* stream) {
    ARX_REQUIRE(degree >= 8 && degree <= GRAPH_DEGREE_MAX && degree % 8 == 0, "degree=%d must be a multiple of 8 in 8..%d", degree, GRAPH_DEGREE_MAX);
    ARX_REQUIRE(dim > 0 && dim % 64 == 0 && dim <= 8192, "dim=%d must be a multiple of 64, at most 8192", dim);
    ARX_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 1..2^31-1", (long long)n_rows);
    ARX_REQUIRE(n_targets >= 0, "n_targets=%d is negative", n_targets);
    ARX_REQUIRE(n_offers >= 0 && n_offers < (1ll << 31) - GRAPH_DEGREE_MAX, "n_offers=%lld out of range 0..2^31-%d", (long long)n_offers,
                GRAPH_DEGREE_MAX + 1);
    ARX_REQUIRE(threads == 0 || threads == 64 || threads == 128 || threads == 256, "threads=%d: 0 (default), 64, 128 or 256", threads);
    ARX_REQUIRE(corpus && neighbors && offer_start, "null pointer argument");
    ARX_REQUIRE(targets || n_targets == 0, "targets is a null pointer (n_targets=%d)", n_targets);
    ARX_REQUIRE(offers || n_offers == 0, "offers is a null pointer (n_offers=%lld)", (long long)n_offers);
    ARX_REQUIRE((uintptr_t)corpus % 16 == 0, "corpus must be 16-byte aligned");
    if (n_targets == 0) return ARX_OK;
    if (threads == 0) threads = degree > 16 ? 256 : 128;          // the search's choice: a first chunk of H + offers rows, 32 or 16 a pass
    const int smem = dim * 2 + (int)sizeof(LinkSm);
    graph_link_kernel<<<n_targets, threads, smem, (hipStream_t)stream>>>((const f16_t*)corpus, n_rows, dim, neighbors, degree, targets, offer_start,
                                                                        offers, n_offers);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_graph_link(const void* corpus, int64_t n_rows, int32_t dim, int32_t* neighbors, int32_t degree, const int32_t* targets,
                                  int32_t n_targets, const int32_t* offer_start, const int32_t* offers, int64_t n_offers, void* stream) {
    return arx_graph_link_tuned(corpus, n_rows, dim, neighbors, degree, targets, n_targets, offer_start, offers, n_offers, 0, stream);
}

extern "C" int32_t arx_graph_remap(int32_t* neighbors, int64_t count, int32_t degree, const uint64_t* keep, const int64_t* word_rank, int64_t n_old,
                                   void* stream) {
    ARX_REQUIRE(degree >= 8 && degree <= GRAPH_DEGREE_MAX && degree % 8 == 0, "degree=%d must be a multiple of 8 in 8..%d", degree, GRAPH_DEGREE_MAX);
    ARX_REQUIRE(n_old >= 0 && n_old < (1ll << 31), "n_old=%lld out of range 0..2^31-1", (long long)n_old);
    ARX_REQUIRE(count >= 0 && count <= n_old, "count=%lld out of range 0..n_old=%lld", (long long)count, (long long)n_old);
    if (count == 0) return ARX_OK;
    ARX_REQUIRE(neighbors && keep && word_rank, "null pointer argument");
    graph_remap_kernel<<<(unsigned)((count + GRAPH_NW_MAX - 1) / GRAPH_NW_MAX), GRAPH_NT_MAX, 0, (hipStream_t)stream>>>(
        neighbors, count, degree, (const unsigned long long*)keep, (const long long*)word_rank, n_old);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
