// arx_ivf_search: exact top-k over the rows of the inverted lists a query probes (gfx950; C ABI in include/arx.h; the host layer is
// arxiv_rag_amd/ivf.py; the definition is INTEGRATION.md "IVF probe search").
//
// The lists are topics.members' layout: `order` holds the rows sorted by (list, row), list c is order[start[c] .. start[c + 1]).  The rows
// query q sees are the entries of the distinct lists in probes[q] that lie in [0, n_lists), restricted to [0, n_rows) and, with `allow`,
// to rows whose bit is set.  Which lists a query probes is the caller's approximation; everything here is exact: a (query, row) score is
// exact_row_score (exact_score.h), the order is (score desc, row asc), and the answer is what arx_topk_search_filtered gives for the
// bitmap of those rows, bit for bit.
//   prepare   one block per query.  `start` clamped into [0, n_members] and made non-decreasing (list_starts.h's scan_starts, the block-
//             wide prefix maximum in LDS that cluster.hip reads the same lists with), the probes deduped (an entry equal to an earlier one, or outside [0, n_lists), gets length 0), every list cut at max_list_rows
//             entries -> cum[q][0 .. n_probe] the cumulative lengths, beg[q][i] the first `order` position of probe i's list.  A position
//             of the query's concatenated list maps to (probe, offset) by a binary search over cum.  The clamped lists are disjoint
//             stretches of `order`, so a query's total is at most n_members.
//   scan      block (stretch p of rows_per_block positions, query q), four waves; a block past the query's total returns at once.  A wave
//             reads 64 `order` entries coalesced, then scores eight rows per step with eight lanes each (masked_exhaustive_kernel's loop)
//             and keeps its running top-k with wave_merge64.  -> part_s / part_i [parts][nq][k] and part_n [parts][nq], the rows scored.
//   merge     one block per query over its ceil(total / rows_per_block) partial lists, any number of them: eight waves each keep a
//             running top-k over 64-entry stretches of the lists, block_merge_lists gives the k best; the counts are summed (integers).
// No float atomics; a query's answer depends on its row of queries and probes, the lists, `allow` and the corpus alone.  Every index read
// from device memory is clamped or tested before it addresses anything: see the contract in include/arx.h.
//
// arx_ivf_search_multi: the same three kernels with a bitmap per query and a score threshold per query (a scan block serves one query, so
// both are values the block loads once).
//   visible rows  query q sees what arx_ivf_search sees with `allow` replaced by the bitmap allow + filter_of[q] * ceil(n_rows / 64).
//                 filter_of is device data: a value outside [0, n_filters) means the query sees no row (all (-inf, -1), scanned = 0,
//                 hits = 0) and nothing is read through it.  allow == NULL: no filter, filter_of is ignored and may be NULL.  Any
//                 n_filters >= 1.  scanned[q] = the visible rows, each scored once.
//   min_score     a visible row qualifies when score >= min_score[q], a plain f32 compare on the exact_row_score bits: a NaN score never
//                 qualifies, a NaN threshold qualifies nothing, -inf qualifies every visible row whose score is not NaN.  A row that does
//                 not qualify reaches wave_merge64 as (-inf, -1), exactly as a lane without a row does.  min_score == NULL: every visible
//                 row qualifies and goes to wave_merge64 as arx_ivf_search passes it.  There a NaN score never starts a merge (ns >= kth
//                 is false) and, once inside wave_topk beside others, loses or wins by comparisons that are all false: scores are NaN
//                 only where the rows or the query hold inf or NaN, and the rank of such a row is not defined (it is whatever
//                 arx_ivf_search gives: the code is the same).
//   result        the best k qualifying rows by (score desc, row asc), padded with (-inf, -1), ids + idx_base.
//   hits[q]       the exact number of qualifying rows: an int64 sum of the blocks' integer counts, no cap.  With min_score == NULL
//                 hits[q] = scanned[q] (every visible row qualifies, whatever its score).
// With n_filters = 1, filter_of all zero and min_score = NULL the outputs equal arx_ivf_search's with that bitmap bit for bit, for every
// rows_per_block; query by query the outputs equal those of a call with that query alone.  Both entry points run the same kernels:
// arx_ivf_search is the call with filter_of = NULL (one bitmap or none, a block-uniform test in the scan), no threshold and no hits.  The
// scan is one template on THR: <true>, launched when min_score is given, adds the threshold and the count of qualifying rows.
#include <math.h>

#include "arx_common.h"
#include "gemm.h"
#include "gemm8.h"
#include "list_starts.h"
#include "search_consts.h"

namespace {      // the headers also define non-template kernels: internal linkage keeps this object's copies apart from search.hip's
#include "search_pass_a.h"
#include "search_tail.h"
#include "masked_topk.h"

constexpr int IVF_PROBE_MAX = 128, IVF_LISTS_MAX = 4096;
constexpr int IVF_PREP_NT = 1024;
constexpr int IVF_SCAN_NW = 4, IVF_MERGE_NW = 8;
constexpr int64_t IVF_SLOTS_MAX = 1ll << 17;      // (part, query) lists the workspace holds at most: 50 MB at k = 32
constexpr int IVF_RPB_DEFAULT = 128;              // 1 query x 32 probes x 2 400 rows = 600 blocks: two per CU and more
constexpr int IVF_RPB_WIDE = 1024;                // the default grows to this while the grid holds more than IVF_BLOCKS_ENOUGH blocks
constexpr int IVF_BLOCKS_ENOUGH = 2048;
constexpr int IVF_RPB_LIMIT = 1 << 20;

__global__ __launch_bounds__(IVF_PREP_NT) void ivf_prepare_kernel(const int64_t* __restrict__ start, int n_lists, int64_t n_members,
                                                                   int64_t max_list_rows, const int32_t* __restrict__ probes, int n_probe,
                                                                   int32_t* __restrict__ cum, int32_t* __restrict__ beg) {
    __shared__ int cs[IVF_LISTS_MAX + 1];          // start, clamped and non-decreasing
    __shared__ int wmax[IVF_PREP_NT / 64];
    __shared__ int32_t pr[IVF_PROBE_MAX], len[IVF_PROBE_MAX];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid < n_probe) pr[tid] = probes[(int64_t)q * n_probe + tid];
    scan_starts(start, n_lists, (int)n_members, cs, wmax);    // (n_members < 2^31: ivf_run; ends in a barrier, which covers pr too)
    if (tid < n_probe) {
        const int32_t c = pr[tid];
        bool use = c >= 0 && c < n_lists;
        for (int j = 0; j < tid; ++j) use = use && pr[j] != c;                     // a repeated probe counts once
        const int32_t c0 = use ? c : 0;
        const int64_t l = (int64_t)cs[c0 + 1] - cs[c0];
        len[tid] = use ? (int32_t)(l < max_list_rows ? l : max_list_rows) : 0;
        beg[(int64_t)q * n_probe + tid] = cs[c0];
    }
    __syncthreads();
    if (tid <= n_probe) {
        int32_t s = 0;                                          // (disjoint stretches of `order`: the sum is at most n_members < 2^31)
        for (int j = 0; j < tid; ++j) s += len[j];
        cum[(int64_t)q * (n_probe + 1) + tid] = s;
    }
}

// filter_of (NULL: one bitmap for every query, or none): the block's bitmap is allow + filter_of[q] * words (a filter_of outside
// [0, n_filters): the block scores nothing and writes an empty list).  THR: a row qualifies when its score >= min_score[q]; part_m holds
// the block's count of those.
template <bool THR>
__global__ __launch_bounds__(IVF_SCAN_NW * 64) void ivf_scan_kernel(const f16_t* __restrict__ C, int64_t n_rows, int D,
                                                                     const int32_t* __restrict__ order, const f16_t* __restrict__ Q, int nq,
                                                                     const int32_t* __restrict__ cum, const int32_t* __restrict__ beg, int n_probe,
                                                                     const uint64_t* __restrict__ allow, int n_filters,
                                                                     const int32_t* __restrict__ filter_of, const float* __restrict__ min_score,
                                                                     int k, int rpb, float* __restrict__ part_s, int64_t* __restrict__ part_i,
                                                                     int32_t* __restrict__ part_n, int32_t* __restrict__ part_m) {
    constexpr int NW = IVF_SCAN_NW;
    const int q = blockIdx.y, p = blockIdx.x;
    const int64_t total = cum[(int64_t)q * (n_probe + 1) + n_probe];
    const int64_t lo = (int64_t)p * rpb;
    if (lo >= total) return;                                   // block-uniform, before any barrier
    int64_t hi = lo + rpb < total ? lo + rpb : total;
    float thr = 0.f;
    if (allow && filter_of) {                                  // the query's own bitmap and threshold: block-uniform, loaded once
        const int32_t f = filter_of[q];
        if (f >= 0 && f < n_filters) allow += (int64_t)f * ((n_rows + 63) >> 6);
        else hi = lo;                                          // no row: the loop below does not run, the list stays (-inf, -1), 0 rows
    }
    if constexpr (THR) thr = min_score[q];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ int32_t s_cum[IVF_PROBE_MAX], s_beg[IVF_PROBE_MAX];
    __shared__ int s_n[NW], s_m[NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    float* sc = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15)) + w * GROUP_ROWS;
    load_query_row<NW * 64>(qs, Q, q, D);
    if (tid < n_probe) {
        s_cum[tid] = cum[(int64_t)q * (n_probe + 1) + tid];
        s_beg[tid] = beg[(int64_t)q * n_probe + tid];
    }
    __syncthreads();
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float cs = -INFINITY; int64_t ci = -1;
    int scored = 0, hits = 0;
    for (int64_t base = lo + (int64_t)w * 64; base < hi; base += NW * 64) {
        int64_t mine = -1;
        if (base + lane < hi) {
            const int32_t pos = (int32_t)(base + lane);
            int i = 0;                                         // the largest i with cum[i] <= pos: its list is not empty, as pos < total
#pragma unroll
            for (int step = IVF_PROBE_MAX / 2; step; step >>= 1) {
                const int t = i + step;
                if (t < n_probe && s_cum[t] <= pos) i = t;
            }
            const int64_t r = order[(int64_t)s_beg[i] + (pos - s_cum[i])];          // inside the clamped list: below n_members
            bool ok = r >= 0 && r < n_rows;                                          // an entry that names no row keeps its place
            if (ok && allow) ok = (allow[r >> 6] >> (r & 63)) & 1ull;
            mine = ok ? r : -1;
        }
        const unsigned long long have = __ballot(mine >= 0);
        scored += __popcll(have);
        for (int r8 = 0; r8 < 64; r8 += 8) {
            if (((have >> r8) & 0xffull) == 0ull) continue;    // wave-uniform
            const int64_t row = __shfl(mine, r8 + rsub);
            const bool ok = row >= 0;
            const float a = exact_row_score(C + (ok ? row : 0) * D, qs, nch, l8, ok);
            if (l8 == 0) sc[r8 + rsub] = a;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (THR) {
            const float v = mine >= 0 ? sc[lane] : -INFINITY;
            const bool pass = mine >= 0 && v >= thr;           // false where the score or the threshold is NaN
            hits += __popcll(__ballot(pass));
            wave_merge64(cs, ci, pass ? v : -INFINITY, pass ? mine : -1, k, lane, w_s[w], w_i[w]);
        } else {
            wave_merge64(cs, ci, mine >= 0 ? sc[lane] : -INFINITY, mine, k, lane, w_s[w], w_i[w]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (lane < k) { w_s[w][lane] = cs; w_i[w][lane] = ci; }
    if (lane == 0) { s_n[w] = scored; if constexpr (THR) s_m[w] = hits; }
    __syncthreads();
    if (w == 0) {
        block_merge_lists<NW>(w_s, w_i, k, lane, fin_s, fin_i);
        const int64_t slot = (int64_t)p * nq + q;
        if (lane < k) { part_s[slot * k + lane] = fin_s[lane]; part_i[slot * k + lane] = fin_i[lane]; }
        if (lane == 0) {
            int n = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) n += s_n[ww];
            part_n[slot] = n;
            if constexpr (THR) {
                int m = 0;
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) m += s_m[ww];
                part_m[slot] = m;
            }
        }
    }
}

// part_m: the blocks' counts of qualifying rows, or NULL where every scored row qualifies (the sum of part_n then serves both outputs).
__global__ __launch_bounds__(IVF_MERGE_NW * 64) void ivf_merge_kernel(const float* __restrict__ part_s, const int64_t* __restrict__ part_i,
                                                                       const int32_t* __restrict__ part_n, const int32_t* __restrict__ part_m,
                                                                       const int32_t* __restrict__ cum, int n_probe, int rpb, int nq, int k,
                                                                       int64_t idx_base, float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                                       int64_t* __restrict__ out_scanned, int64_t* __restrict__ out_hits) {
    constexpr int NW = IVF_MERGE_NW, NT = NW * 64;
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ unsigned long long s_n, s_m;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t total = cum[(int64_t)q * (n_probe + 1) + n_probe];
    const int64_t parts = (total + rpb - 1) / rpb;             // the scan blocks of this query that wrote a list
    const int64_t n = parts * k;
    if (tid == 0) { s_n = 0ull; s_m = 0ull; }
    __syncthreads();
    float cs = -INFINITY; int64_t ci = -1;
    for (int64_t c0 = (int64_t)w * 64; c0 < n; c0 += NT) {
        const int64_t c = c0 + lane;
        float ns = -INFINITY; int64_t ni = -1;
        if (c < n) {
            const int64_t o = ((c / k) * nq + q) * k + c % k;
            ns = part_s[o]; ni = part_i[o];
        }
        wave_merge64(cs, ci, ns, ni, k, lane, w_s[w], w_i[w]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    unsigned long long cnt = 0;
    for (int64_t p = tid; p < parts; p += NT) cnt += (unsigned long long)part_n[p * nq + q];
    if (cnt) atomicAdd(&s_n, cnt);
    if (out_hits && part_m) {                                  // block-uniform
        unsigned long long m = 0;
        for (int64_t p = tid; p < parts; p += NT) m += (unsigned long long)part_m[p * nq + q];
        if (m) atomicAdd(&s_m, m);
    }
    if (lane < k) { w_s[w][lane] = cs; w_i[w][lane] = ci; }
    __syncthreads();
    if (w == 0) {
        block_merge_lists<NW>(w_s, w_i, k, lane, fin_s, fin_i);
        if (lane < k) {
            out_s[(int64_t)q * k + lane] = fin_s[lane];
            out_i[(int64_t)q * k + lane] = fin_i[lane] >= 0 ? fin_i[lane] + idx_base : -1;
        }
        if (out_scanned && lane == 0) out_scanned[q] = (int64_t)s_n;
        if (out_hits && lane == 0) out_hits[q] = (int64_t)(part_m ? s_m : s_n);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct IvfWs { int64_t cum, beg, part_s, part_i, part_n, part_m, total, slots; int qb; };
bool ivf_shape_ok(int64_t n_members, int32_t n_lists, int32_t n_queries, int32_t n_probe, int32_t dim, int32_t k) {
    return n_members >= 0 && n_members < (1ll << 31) && n_lists >= 1 && n_lists <= IVF_LISTS_MAX && n_queries > 0 && n_probe >= 1 &&
           n_probe <= IVF_PROBE_MAX && dim > 0 && dim % 64 == 0 && dim <= 8192 && k >= 1 && k <= KMAX;
}
// multi: arx_ivf_search_multi's layout, the same with part_m [slots] behind it
IvfWs ivf_layout(int64_t n_members, int n_queries, int n_probe, int k, bool multi) {
    IvfWs w;
    w.qb = n_queries < QBATCH_MAX ? n_queries : QBATCH_MAX;
    const int64_t parts = (n_members + 63) / 64 > 0 ? (n_members + 63) / 64 : 1;      // at the smallest rows_per_block
    w.slots = parts * w.qb < IVF_SLOTS_MAX ? parts * w.qb : IVF_SLOTS_MAX;
    if (w.slots < w.qb) w.slots = w.qb;
    int64_t o = 0;
    auto take = [&](int64_t b) { int64_t r = o; o += round_up64(b, 256); return r; };
    w.cum = take((int64_t)w.qb * (n_probe + 1) * 4);
    w.beg = take((int64_t)w.qb * n_probe * 4);
    w.part_s = take(w.slots * k * 4);
    w.part_i = take(w.slots * k * 8);
    w.part_n = take(w.slots * 4);
    w.part_m = multi ? take(w.slots * 4) : -1;
    w.total = o;
    return w;
}

// multi: arx_ivf_search_multi's workspace layout and its checks of the per-query arguments.  arx_ivf_search is multi = false with
// n_filters = 1, filter_of = min_score = out_hits = NULL (one bitmap, no threshold, no hits).
int32_t ivf_run(bool multi, const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries, const int32_t* probes, int32_t n_probe,
                const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const float* min_score, int32_t k, float* out_scores,
                int64_t* out_ids, int64_t* out_scanned, int64_t* out_hits, int64_t idx_base, void* ws, int64_t ws_bytes, int32_t rows_per_block,
                void* stream) {
    ARX_REQUIRE(k >= 1 && k <= KMAX, "k=%d out of range 1..%d", k, KMAX);
    ARX_REQUIRE(n_probe >= 1 && n_probe <= IVF_PROBE_MAX, "n_probe=%d out of range 1..%d", n_probe, IVF_PROBE_MAX);
    ARX_REQUIRE(dim > 0 && dim % 64 == 0 && dim <= 8192, "dim=%d must be a multiple of 64, at most 8192", dim);
    ARX_REQUIRE(n_lists >= 1 && n_lists <= IVF_LISTS_MAX, "n_lists=%d out of range 1..%d", n_lists, IVF_LISTS_MAX);
    ARX_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 1..2^31-1", (long long)n_rows);
    ARX_REQUIRE(n_members >= 0 && n_members < (1ll << 31), "n_members=%lld out of range 0..2^31-1", (long long)n_members);
    ARX_REQUIRE(max_list_rows >= 0 && max_list_rows <= n_members, "max_list_rows=%lld out of range 0..n_members", (long long)max_list_rows);
    ARX_REQUIRE(n_queries > 0, "n_queries=%d: empty query set", n_queries);
    ARX_REQUIRE(rows_per_block == 0 || (rows_per_block >= 64 && rows_per_block % 64 == 0 && rows_per_block <= IVF_RPB_LIMIT),
                "rows_per_block=%d: 0 (default) or a multiple of 64 in 64..%d", rows_per_block, IVF_RPB_LIMIT);
    ARX_REQUIRE(corpus && start && queries && probes && out_scores && out_ids && ws && (order || n_members == 0), "null pointer argument");
    ARX_REQUIRE(((uintptr_t)corpus | (uintptr_t)queries | (uintptr_t)ws) % 16 == 0, "corpus, queries and ws must be 16-byte aligned");
    if (multi && allow) {
        ARX_REQUIRE(n_filters >= 1, "n_filters=%d: at least one bitmap when allow is given", n_filters);
        ARX_REQUIRE(filter_of != nullptr, "filter_of is null: allow needs one filter index per query");
        ARX_REQUIRE((int64_t)n_filters <= INT64_MAX / ((n_rows + 63) >> 6), "n_filters=%d: n_filters * ceil(n_rows / 64) overflows int64", n_filters);
        ARX_REQUIRE((uintptr_t)filter_of % 4 == 0, "filter_of must be 4-byte aligned");
    }
    if (min_score) ARX_REQUIRE((uintptr_t)min_score % 4 == 0, "min_score must be 4-byte aligned");
    if (!allow) filter_of = nullptr;                           // no filter: filter_of is ignored
    const IvfWs L = ivf_layout(n_members, n_queries, n_probe, k, multi);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (%s)", (long long)ws_bytes, (long long)L.total,
                multi ? "arx_ivf_multi_workspace_bytes" : "arx_ivf_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    char* wsb = (char*)ws;
    int32_t* cum = (int32_t*)(wsb + L.cum);
    int32_t* beg = (int32_t*)(wsb + L.beg);
    float* part_s = (float*)(wsb + L.part_s);
    int64_t* part_i = (int64_t*)(wsb + L.part_i);
    int32_t* part_n = (int32_t*)(wsb + L.part_n);
    const bool thr = multi && min_score;                       // (part_m exists in the multi layout alone)
    int32_t* part_m = thr ? (int32_t*)(wsb + L.part_m) : nullptr;
    // positions a query's lists can hold: n_probe lists of at most max_list_rows entries, disjoint stretches of `order`
    const int64_t P = (int64_t)n_probe * max_list_rows < n_members ? (int64_t)n_probe * max_list_rows : n_members;
    const size_t smem = (((size_t)dim * 2 + 15) & ~(size_t)15) + IVF_SCAN_NW * GROUP_ROWS * 4;
    for (int q0 = 0; q0 < n_queries; q0 += QBATCH_MAX) {
        const int nq = (n_queries - q0) < QBATCH_MAX ? (n_queries - q0) : QBATCH_MAX;
        int64_t rpb = rows_per_block;
        if (rpb == 0)
            for (rpb = IVF_RPB_DEFAULT; rpb < IVF_RPB_WIDE && (P + rpb - 1) / rpb * nq > IVF_BLOCKS_ENOUGH; rpb *= 2) {}
        const int64_t max_parts = L.slots / nq;                 // >= 1: the partial lists the workspace holds per query
        if ((P + rpb - 1) / rpb > max_parts) rpb = round_up64((P + max_parts - 1) / max_parts, 64);
        const int64_t nbx = (P + rpb - 1) / rpb > 0 ? (P + rpb - 1) / rpb : 1;
        ARX_REQUIRE(nbx <= max_parts && nbx < (1ll << 31) && rpb < (1ll << 31), "grid too large");
        const f16_t* Q = (const f16_t*)queries + (int64_t)q0 * dim;
        ivf_prepare_kernel<<<nq, IVF_PREP_NT, 0, st>>>(start, n_lists, n_members, max_list_rows, probes + (int64_t)q0 * n_probe, n_probe, cum, beg);
        ARX_HIP_CHECK(hipGetLastError());
        const dim3 grid((unsigned)nbx, (unsigned)nq);
        const int32_t* fo = filter_of ? filter_of + q0 : nullptr;
        if (thr)
            ivf_scan_kernel<true><<<grid, IVF_SCAN_NW * 64, smem, st>>>((const f16_t*)corpus, n_rows, dim, order, Q, nq, cum, beg, n_probe, allow,
                                                                        n_filters, fo, min_score + q0, k, (int)rpb, part_s, part_i, part_n, part_m);
        else
            ivf_scan_kernel<false><<<grid, IVF_SCAN_NW * 64, smem, st>>>((const f16_t*)corpus, n_rows, dim, order, Q, nq, cum, beg, n_probe, allow,
                                                                         n_filters, fo, nullptr, k, (int)rpb, part_s, part_i, part_n, nullptr);
        ARX_HIP_CHECK(hipGetLastError());
        ivf_merge_kernel<<<nq, IVF_MERGE_NW * 64, 0, st>>>(part_s, part_i, part_n, part_m, cum, n_probe, (int)rpb, nq, k, idx_base,
                                                           out_scores + (int64_t)q0 * k, out_ids + (int64_t)q0 * k,
                                                           out_scanned ? out_scanned + q0 : nullptr,
                                                           out_hits ? out_hits + q0 : nullptr);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}
}      // namespace

extern "C" int64_t arx_ivf_workspace_bytes(int64_t n_members, int32_t n_lists, int32_t n_queries, int32_t n_probe, int32_t dim, int32_t k) {
    if (!ivf_shape_ok(n_members, n_lists, n_queries, n_probe, dim, k)) return -1;
    return ivf_layout(n_members, n_queries, n_probe, k, false).total;
}

extern "C" int64_t arx_ivf_multi_workspace_bytes(int64_t n_members, int32_t n_lists, int32_t n_queries, int32_t n_probe, int32_t dim, int32_t k) {
    if (!ivf_shape_ok(n_members, n_lists, n_queries, n_probe, dim, k)) return -1;
    return ivf_layout(n_members, n_queries, n_probe, k, true).total;
}

extern "C" int32_t arx_ivf_search_tuned(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members,
                                        const int64_t* start, int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries,
                                        const int32_t* probes, int32_t n_probe, const uint64_t* allow, int32_t k, float* out_scores,
                                        int64_t* out_ids, int64_t* out_scanned, int64_t idx_base, void* ws, int64_t ws_bytes,
                                        int32_t rows_per_block, void* stream) {
    return ivf_run(false, corpus, n_rows, dim, order, n_members, start, n_lists, max_list_rows, queries, n_queries, probes, n_probe, allow, 1,
                   nullptr, nullptr, k, out_scores, out_ids, out_scanned, nullptr, idx_base, ws, ws_bytes, rows_per_block, stream);
}

extern "C" int32_t arx_ivf_search(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                                  int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries, const int32_t* probes,
                                  int32_t n_probe, const uint64_t* allow, int32_t k, float* out_scores, int64_t* out_ids, int64_t* out_scanned,
                                  int64_t idx_base, void* ws, int64_t ws_bytes, void* stream) {
    return arx_ivf_search_tuned(corpus, n_rows, dim, order, n_members, start, n_lists, max_list_rows, queries, n_queries, probes, n_probe, allow, k,
                                out_scores, out_ids, out_scanned, idx_base, ws, ws_bytes, 0, stream);
}

extern "C" int32_t arx_ivf_search_multi_tuned(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members,
                                              const int64_t* start, int32_t n_lists, int64_t max_list_rows, const void* queries,
                                              int32_t n_queries, const int32_t* probes, int32_t n_probe, const uint64_t* allow,
                                              int32_t n_filters, const int32_t* filter_of, const float* min_score, int32_t k,
                                              float* out_scores, int64_t* out_ids, int64_t* out_scanned, int64_t* out_hits, int64_t idx_base,
                                              void* ws, int64_t ws_bytes, int32_t rows_per_block, void* stream) {
    return ivf_run(true, corpus, n_rows, dim, order, n_members, start, n_lists, max_list_rows, queries, n_queries, probes, n_probe, allow,
                   n_filters, filter_of, min_score, k, out_scores, out_ids, out_scanned, out_hits, idx_base, ws, ws_bytes, rows_per_block, stream);
}

extern "C" int32_t arx_ivf_search_multi(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members,
                                        const int64_t* start, int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries,
                                        const int32_t* probes, int32_t n_probe, const uint64_t* allow, int32_t n_filters,
                                        const int32_t* filter_of, const float* min_score, int32_t k, float* out_scores, int64_t* out_ids,
                                        int64_t* out_scanned, int64_t* out_hits, int64_t idx_base, void* ws, int64_t ws_bytes, void* stream) {
    return arx_ivf_search_multi_tuned(corpus, n_rows, dim, order, n_members, start, n_lists, max_list_rows, queries, n_queries, probes, n_probe,
                                      allow, n_filters, filter_of, min_score, k, out_scores, out_ids, out_scanned, out_hits, idx_base, ws,
                                      ws_bytes, 0, stream);
}
