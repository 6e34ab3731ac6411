// arx_range_search: score-threshold search over an fp16 shard (C ABI in include/arx.h; LangChain's similarity_score_threshold, LlamaIndex's
// similarity_cutoff, and candidate lists longer than the top-k searches' 32).  For query q with threshold min_score[q] and an optional
// bitmap in the convention of arx_topk_search_filtered:
//   score(q, r)    exact_row_score (search_tail.h): the bits arx_topk_search and arx_topk_search_filtered give the pair
//   qualifies      a visible row with score(q, r) >= min_score[q], compared in f32 (-inf: every visible row; +inf or NaN: none)
//   answer         the best min(count, M) qualifying rows by (score desc, row asc), M = max_results <= 1024, (-inf, -1) padding, and
//                  out_counts[q] = the number of qualifying rows when that is <= M, M + 1 when more qualify (the list is truncated)
// The host side is masked_topk.h's scan driver (masked_scan) with RangeSearch below as its search policy and bitmap_rows.h's AllowRows as
// its mask (allow == NULL: an all-ones bitmap in the workspace).  Pass A is masked_topk.h's masked_groupmax_kernel with bitmap_rows.h's
// BitmapRows policy, unchanged.  The tail (range_tail_kernel, one block per query) finds its candidate groups by masked_topk.h's stage
// (tail_kth_key, tail_candidates) with a threshold of its own; then it keeps a variable, long, ordered list instead of a k <= 32 wave list.
// Why the tail is exact: pass A and exact_row_score differ by at most tau = tau_scale |q| (masked_tau_scale, masked_topk.h), so a qualifying
// row has a pass-A score >= min_score - tau and its group's maximum is at least that.  Let t be the (M + 1)-th largest group maximum of
// the query (-inf when fewer than M + 1 groups hold a visible row).  A qualifying row in a group with gmax < t - 2 tau has an exact score
// below t - tau, while M + 1 distinct groups each hold a visible row whose pass-A score is >= t, hence whose exact score is >= t - tau:
// those M + 1 rows all qualify (they beat a qualifying row) and all beat it, so it is not among the best M.  Candidates = every non-empty
// group with gmax >= max(min_score - tau, t - 2 tau): they hold every row of the answer, and whenever more than M rows qualify they
// alone hold M + 1 qualifying rows.  So "qualifying rows among the candidates <= M" means the list and the count are complete, and
// ">= M + 1" means truncated: the count is reported as M + 1 and nothing more is known (an exact total would make a loose threshold
// cost a full exact scan).  The (M + 1)-th largest of up to n_rows / 64 values is the block-wide radix select over order_key that
// the masked and grouped tails use (tail_kth_key).
// The list: a qualifying row is the 64-bit key (order_key(score) << 32) | (0xffffffff - row), whose unsigned order is (score desc, row
// asc); 0 = none (n_rows < 2^32).  The waves append keys to RANGE_CAP = 2048 slots in LDS (an INTEGER LDS atomic hands out the slots:
// the list's order varies, its content does not); every qualifying row is counted apart.  Before a round of 16 groups that could
// overflow the slots, the list is cut back to its M largest keys by a block-wide bitonic sort and the M-th key becomes the append
// threshold, as bm25.hip keeps its candidates.  At the end the list is sorted once more and its best min(count, M) keys are stored.
// The exhaustive path (a query whose candidate list overflows cand_cap; path 2): the shard's groups cut into T parts, block (part, query)
// keeps the same list over every visible row of its part, scored by the same function, and stores its best M keys and its count; one
// block per query then merges the T lists (at most T M <= 4096 keys, T - 1 rounds of at most one cut-back sort each: tens of
// microseconds per flagged query) and adds the counts.  Same bits.
// No float atomics; integer LDS atomics only as slot or plain counters whose order cannot reach the output; plain vector stores.  Every
// output element of a query is written.  A query's output depends on the query, its threshold, the bitmap and the corpus alone.
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

#define RANGE_MAX_RESULTS 1024       // largest M
#define RANGE_CAP 2048               // key slots of a block's list (16 KB of LDS): M kept keys + one round of 16 groups x 64 rows
#define RANGE_NT FILT_TAIL_NT        // threads of every block that keeps a list
#define RANGE_PART_KEYS 4096         // T M <= this: bounds the exhaustive path's per-part lists (and the workspace)

// ---- the list of a block ------------------------------------------------------------------------------------------------------------------
struct RangeList {
    unsigned long long keys[RANGE_CAP];
    unsigned long long thr;      // keys at or below it are not appended: 0, then the M-th key of the last cut
    int cnt;                     // slots handed out
    int n_qual;                  // qualifying rows seen, appended or not
};

__device__ __forceinline__ unsigned long long range_key(float s, int64_t row) {
    return ((unsigned long long)order_key(s) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)row);
}

// keys[0 .. c) -> descending order (bitonic, over the next power of two >= max(c, 64), the slots beyond c zeroed).  The whole block, c
// block-uniform and <= RANGE_CAP; every thread's earlier writes to keys[] are behind a barrier already; ends with a barrier.
__device__ __forceinline__ void range_sort_desc(unsigned long long* keys, int c) {
    const int tid = threadIdx.x;
    int n = 64;
    while (n < c) n <<= 1;
    for (int i = c + tid; i < n; i += RANGE_NT) keys[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < (n >> 1)) {                              // n / 2 <= RANGE_CAP / 2 = RANGE_NT pairs
                const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;
                const unsigned long long a = keys[i], b = keys[p];
                if (((i & k) == 0) ? a < b : a > b) { keys[i] = b; keys[p] = a; }
            }
            __syncthreads();
        }
}

// cut the list (c keys, any order) back to its M largest, sorted; updates cnt and thr.  The whole block, c uniform; ends with a barrier.
__device__ __forceinline__ void range_cut(RangeList& L, int c, int M) {
    range_sort_desc(L.keys, c);
    if (threadIdx.x == 0) {
        L.cnt = c < M ? c : M;
        L.thr = c >= M ? L.keys[M - 1] : 0ull;
    }
    __syncthreads();
}

// one wave: the visible rows `word` of group g scored; those at or above ms counted, and appended where their key is above thr
__device__ __forceinline__ void range_take_group(RangeList& L, const f16_t* __restrict__ C, int64_t g, uint64_t word, const f16_t* qs, int D,
                                                 int lane, float* sc, float ms, unsigned long long thr) {
    score_word_rows(C, g, word, qs, D, lane, sc);
    const bool mine = (word >> lane) & 1ull;
    const float s = mine ? sc[lane] : 0.f;
    const bool qual = mine && s >= ms;
    const unsigned long long qm = __ballot(qual);
    if (qm == 0ull) return;                                     // wave-uniform
    const unsigned long long key = range_key(s, g * GROUP_ROWS + lane);
    const bool app = qual && key > thr;
    const unsigned long long am = __ballot(app);
    int base = 0;
    if (lane == 0) {
        atomicAdd(&L.n_qual, __popcll(qm));                     // a plain counter
        if (am) base = atomicAdd(&L.cnt, __popcll(am));         // a slot counter: the list is read as a set
    }
    base = __shfl(base, 0);
    if (app) {
        const int sl = base + __popcll(am & ((1ull << lane) - 1ull));
        if (sl < RANGE_CAP) L.keys[sl] = key;                   // (always: the caller cuts the list before a round that could overflow)
    }
}

// the rounds of a block: in round r wave w takes item r * NW + w of `n_items`; group_of_item(item) names its group (< 0: none) and
// word_of(g) its visible rows.  Before a round that could overflow the slots the list is cut back.  Ends with a barrier.
template <class GroupOf, class WordOf>
__device__ __forceinline__ void range_rounds(RangeList& L, int64_t n_items, GroupOf group_of_item, WordOf word_of, const f16_t* __restrict__ C,
                                             const f16_t* qs, int D, float* sc, float ms, int M) {
    constexpr int NW = RANGE_NT / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t base = 0; base < n_items; base += NW) {       // block-uniform
        const int c = L.cnt;
        __syncthreads();                                         // everyone has read cnt before anyone appends
        if (c + NW * GROUP_ROWS > RANGE_CAP) range_cut(L, c < RANGE_CAP ? c : RANGE_CAP, M);
        const unsigned long long thr = L.thr;
        const int64_t g = base + w < n_items ? group_of_item(base + w) : -1;
        if (g >= 0) {                                            // wave-uniform
            const uint64_t word = word_of(g);
            if (word) range_take_group(L, C, g, word, qs, D, lane, sc, ms, thr);
        }
        __syncthreads();
    }
}

// the sorted list's best min(c, M) keys -> this query's M output slots (the rest padded) and its count
__device__ __forceinline__ void range_store(const RangeList& L, int c, int n_qual, int M, int64_t idx_base, float* __restrict__ out_s,
                                            int64_t* __restrict__ out_i, int32_t* __restrict__ out_c) {
    for (int r = threadIdx.x; r < M; r += RANGE_NT) {
        const unsigned long long key = r < c ? L.keys[r] : 0ull;
        out_s[r] = key ? key_value((uint32_t)(key >> 32)) : -INFINITY;
        out_i[r] = key ? (int64_t)(0xffffffffu - (uint32_t)key) + idx_base : -1;
    }
    if (threadIdx.x == 0) *out_c = n_qual < M + 1 ? n_qual : M + 1;
}

// ---- the tail: one block per query ----------------------------------------------------------------------------------------------------------
// stats: [0] queries sent to the exhaustive path, [1] candidate groups rescored, [2] (low word) "some query of this call overflowed".
// out_* / min_score point at this batch's first query.
__global__ __launch_bounds__(RANGE_NT) void range_tail_kernel(const float* __restrict__ gmax, int64_t ldg, int64_t n_groups,
                                                               const uint64_t* __restrict__ allow, const f16_t* __restrict__ Q,
                                                               const float* __restrict__ min_score, const f16_t* __restrict__ C, int64_t n_rows,
                                                               int D, int M, float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                               int32_t* __restrict__ out_c, int64_t idx_base, float tau_scale, int cand_cap,
                                                               int32_t* __restrict__ redo, unsigned long long* __restrict__ stats) {
    constexpr int NT = RANGE_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ RangeList L;
    __shared__ TailStage st;
    const int q = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
    const float ms = min_score[q];
    out_s += (int64_t)q * M; out_i += (int64_t)q * M; out_c += q;
    if (tid == 0) { st.n_c = 0; L.cnt = 0; L.n_qual = 0; L.thr = 0ull; }
    if (!(ms < INFINITY)) {                                     // block-uniform: +inf or NaN, no row qualifies
        __syncthreads();
        range_store(L, 0, 0, M, idx_base, out_s, out_i, out_c);
        if (tid == 0) redo[q] = 0;
        return;
    }
    f16_t* qs = reinterpret_cast<f16_t*>(smem);                                                  // [D] query row
    float* sc_all = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15));      // [NW][64] row scores of the group a wave is at
    int32_t* list = reinterpret_cast<int32_t*>(sc_all + NW * GROUP_ROWS);                        // [cand_cap] candidate groups
    load_query_row<NT>(qs, Q, q, D);
    const float* col = gmax + q;                                                                 // this query's column of group maxima
    uint32_t kv[FILT_REG_GROUPS];
    const uint32_t T = tail_kth_key(st, kv, col, ldg, n_groups, qs, D, M + 1);      // the (M + 1)-th largest group maximum
    const float tau = tau_scale * st.qn;
    const float thr = fmaxf(ms - tau, key_value(T) - 2.0f * tau);      // key_value(T) = -inf when fewer than M + 1 groups hold a visible row
    const int nc = tail_candidates(st, kv, col, ldg, n_groups, thr, list, cand_cap, q, redo, stats);
    if (nc < 0) return;                                        // block-uniform: flagged for the exhaustive path
    // the visible rows of the candidate groups, exactly: a group per wave at a time
    range_rounds(L, nc, [&](int64_t item) { return (int64_t)list[item]; },
                 [&](int64_t g) { return allow[g] & valid_bits(n_rows, g); }, C, qs, D, sc_all + w * GROUP_ROWS, ms, M);
    const int c = L.cnt < RANGE_CAP ? L.cnt : RANGE_CAP;
    range_sort_desc(L.keys, c);
    range_store(L, c, L.n_qual, M, idx_base, out_s, out_i, out_c);
}

// ---- exhaustive path: block (part p, query q) keeps the list over the visible rows of groups [p per, (p + 1) per) -> its best M keys
// part_k [parts][nq][M] (0 = none) and its count of qualifying rows part_c [parts][nq].  only_if / gate as masked_topk.h's.
__global__ __launch_bounds__(RANGE_NT) void range_exhaustive_kernel(const uint64_t* __restrict__ allow, const f16_t* __restrict__ Q,
                                                                     const float* __restrict__ min_score, const f16_t* __restrict__ C,
                                                                     int64_t n_rows, int64_t n_groups, int D, int nq, int M,
                                                                     unsigned long long* __restrict__ part_k, int32_t* __restrict__ part_c,
                                                                     const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int q = blockIdx.y, p = blockIdx.x, parts = gridDim.x;
    if (only_if && !only_if[q]) return;
    constexpr int NT = RANGE_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ RangeList L;
    const int tid = threadIdx.x, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    float* sc = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15)) + w * GROUP_ROWS;
    load_query_row<NT>(qs, Q, q, D);
    if (tid == 0) { L.cnt = 0; L.n_qual = 0; L.thr = 0ull; }
    __syncthreads();
    const float ms = min_score[q];
    const int64_t per = (n_groups + parts - 1) / parts;
    const int64_t ga = (int64_t)p * per, gb = ga + per < n_groups ? ga + per : n_groups;
    range_rounds(L, gb > ga ? gb - ga : 0, [&](int64_t item) { return ga + item; },
                 [&](int64_t g) { return allow[g] & valid_bits(n_rows, g); }, C, qs, D, sc, ms, M);
    const int c = L.cnt < RANGE_CAP ? L.cnt : RANGE_CAP;
    range_sort_desc(L.keys, c);
    unsigned long long* pk = part_k + ((int64_t)p * nq + q) * M;
    for (int r = tid; r < M; r += NT) pk[r] = r < c ? L.keys[r] : 0ull;
    if (tid == 0) part_c[(int64_t)p * nq + q] = L.n_qual;
}

// one block per query the exhaustive path answered: its parts' sorted lists merged (a part per round, its at most M <= RANGE_NT keys
// appended, the list cut back before a round that could overflow), the counts added
__global__ __launch_bounds__(RANGE_NT) void range_merge_kernel(const unsigned long long* __restrict__ part_k, const int32_t* __restrict__ part_c,
                                                                int parts, int nq, int M, float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                                int32_t* __restrict__ out_c, int64_t idx_base,
                                                                const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (only_if && !only_if[q]) return;
    __shared__ RangeList L;
    if (tid == 0) { L.cnt = 0; L.n_qual = 0; L.thr = 0ull; }
    __syncthreads();
    int64_t total = 0;
    for (int p = 0; p < parts; ++p) {                           // block-uniform
        total += part_c[(int64_t)p * nq + q];
        const int c = L.cnt;
        __syncthreads();                                         // everyone has read cnt before anyone appends
        if (c + M > RANGE_CAP) range_cut(L, c < RANGE_CAP ? c : RANGE_CAP, M);
        const unsigned long long thr = L.thr;
        if (tid < M) {
            const unsigned long long key = part_k[((int64_t)p * nq + q) * M + tid];
            if (key > thr) {                                     // (thr >= 0: an empty slot is never appended)
                const int sl = atomicAdd(&L.cnt, 1);             // a slot counter: the list is read as a set
                if (sl < RANGE_CAP) L.keys[sl] = key;
            }
        }
        __syncthreads();
    }
    const int c = L.cnt < RANGE_CAP ? L.cnt : RANGE_CAP;
    range_sort_desc(L.keys, c);
    range_store(L, c, (int)(total < M + 1 ? total : M + 1), M, idx_base, out_s + (int64_t)q * M, out_i + (int64_t)q * M, out_c + q);
}

// ---- the search policy (masked_topk.h: the scan driver) -----------------------------------------------------------------------------------
struct RangeSearch {
    int M; const float* min_score; float* out_s; int64_t* out_i; int32_t* out_c; int64_t idx_base;
    unsigned long long* part_k; int32_t* part_c;      // workspace: the exhaustive path's keys [parts][nq][M] and counts [parts][nq]
    static constexpr const char* workspace_fn = "arx_range_workspace_bytes";
    static constexpr size_t kSmemRaise = 32 * 1024;      // more dynamic LDS than this is asked for before the launch

    bool given() const { return min_score && out_s && out_i && out_c; }
    int check(int64_t n_rows) const {
        ARX_REQUIRE(n_rows < (1ll << 32), "n_rows=%lld: a row is 32 bits of a sort key (at most 2^32 - 1 rows per shard)", (long long)n_rows);
        ARX_REQUIRE(M >= 1 && M <= RANGE_MAX_RESULTS, "max_results=%d out of range 1..%d", M, RANGE_MAX_RESULTS);
        return ARX_OK;
    }
    void take_buffers(MaskedWs& w) {
        if (w.parts > RANGE_PART_KEYS / M) w.parts = RANGE_PART_KEYS / M;
        part_k = w.take<unsigned long long>((int64_t)w.parts * w.qb * M * 8);
        part_c = w.take<int32_t>((int64_t)w.parts * w.qb * 4);
    }
    int resolve_path(const AllowRows&, int path, int) const { return path ? path : 1; }
    int default_cand_cap() const { return 2 * (M + 1) + FILT_CAND_CAP_DEFAULT; }      // M + 1 groups reach t by definition: twice that and the masked tail's slack
    int launch_tail(const ScanSlice& s, const AllowRows& mask) const {
        const size_t smem = s.smem_q + (size_t)(RANGE_NT / 64) * GROUP_ROWS * 4 + (size_t)s.cand_cap * 4;
        if (smem > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)range_tail_kernel, (int)smem));
        range_tail_kernel<<<s.nq, RANGE_NT, smem, s.st>>>(s.L.gmax, s.L.ldg, s.L.n_groups, mask.allow, s.Q, min_score + s.q0, s.C, s.n_rows, s.dim, M,
                                                          out_s + (int64_t)s.q0 * M, out_i + (int64_t)s.q0 * M, out_c + s.q0, idx_base,
                                                          s.tau_scale, s.cand_cap, s.L.redo, s.L.stats);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    int launch_exhaustive(const ScanSlice& s, const AllowRows& mask) const {
        const size_t smem_x = s.smem_q + (size_t)(RANGE_NT / 64) * GROUP_ROWS * 4;
        if (smem_x > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)range_exhaustive_kernel, (int)smem_x));
        range_exhaustive_kernel<<<dim3(s.L.parts, s.nq), RANGE_NT, smem_x, s.st>>>(mask.allow, s.Q, min_score + s.q0, s.C, s.n_rows, s.L.n_groups,
                                                                                   s.dim, s.nq, M, part_k, part_c, s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        range_merge_kernel<<<s.nq, RANGE_NT, 0, s.st>>>(part_k, part_c, s.L.parts, s.nq, M, out_s + (int64_t)s.q0 * M, out_i + (int64_t)s.q0 * M,
                                                        out_c + s.q0, idx_base, s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
};
}      // namespace

extern "C" int64_t arx_range_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t max_results) {
    if (n_rows <= 0 || n_rows >= (1ll << 32) || n_queries <= 0 || dim <= 0 || dim % 64 != 0 || dim > 8192 || max_results <= 0 ||
        max_results > RANGE_MAX_RESULTS)
        return -1;
    RangeSearch search{max_results};
    return scan_layout<AllowRows>(search, n_rows, n_queries, nullptr).total;
}

extern "C" int32_t arx_range_search_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                          const float* min_score, int32_t n_queries, int32_t dim, int32_t max_results, float* out_scores,
                                          int64_t* out_ids, int32_t* out_counts, int64_t idx_base, float max_row_norm, void* ws,
                                          int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream) {
    return masked_scan(AllowRows{{allow}, n_allowed}, RangeSearch{max_results, min_score, out_scores, out_ids, out_counts, idx_base}, corpus, n_rows,
                       queries, n_queries, dim, max_row_norm, ws, ws_bytes, path, cand_cap, stream);
}

extern "C" int32_t arx_range_search(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                    const float* min_score, int32_t n_queries, int32_t dim, int32_t max_results, float* out_scores,
                                    int64_t* out_ids, int32_t* out_counts, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes,
                                    void* stream) {
    return arx_range_search_tuned(corpus, n_rows, allow, n_allowed, queries, min_score, n_queries, dim, max_results, out_scores, out_ids,
                                  out_counts, idx_base, max_row_norm, ws, ws_bytes, 0, 0, stream);
}

extern "C" int32_t arx_range_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    return masked_stats(ws, overflowed_queries, candidate_groups, stream);
}
