// arx_topk_search_grouped: the exact top-P PAPERS of an fp16 shard with the m best chunks of each (C ABI in include/arx.h; field
// collapsing by paper).  group_of[r] (device int32, non-decreasing, non-negative, not necessarily dense) names the paper of row r: a paper
// is a contiguous run of rows.  An optional bitmap in the convention of arx_topk_search_filtered says which rows a query may see.
//   score(q, r)    exact_row_score (search_tail.h): the bits arx_topk_search and arx_topk_search_filtered give the pair
//   paper score    the maximum of score(q, r) over the paper's visible rows; a paper without a visible row does not exist for the query
//   answer         the P best papers by (paper score desc, row of the best chunk asc), and of each the m best visible chunks by (score desc,
//                  row asc); (-inf, -1) / -1 padding
// The host side is masked_topk.h's scan driver (masked_scan) with GroupedSearch below as its search policy and bitmap_rows.h's AllowRows as
// its mask (allow == NULL: an all-ones bitmap in the workspace).  Pass A is masked_topk.h's masked_groupmax_kernel with bitmap_rows.h's
// BitmapRows policy, unchanged.  The tail (grouped_tail_kernel, one block per query) finds its candidate groups by masked_topk.h's stage
// (tail_kth_key, tail_candidates) and folds their rows by paper.  With R = max_run_rows an upper bound on the rows of any run, a run touches
// at most S = floor((R + 62) / 64) + 1 of the 64-row groups; K = P S.
// Why the tail is exact: let t be the K-th largest group maximum of the query.  The K groups at or above t each hold a visible row whose
// pass-A score is >= t; a paper touches at most S of them, so at least P distinct papers have a visible row whose pass-A score is >= t,
// hence whose exact score is >= t - tau (pass A and exact_row_score differ by at most tau = tau_scale |q|: masked_tau_scale, masked_topk.h).
// So the P-th best paper score is >= t - tau, and every paper of the true top-P - ties at the P-th score included - has its best row at
// an exact score >= t - tau, a pass-A score >= t - 2 tau: that row lies in a group with gmax >= t - 2 tau.  Candidates = every non-empty
// group with gmax >= t - 2 tau; their visible rows are rescored exactly and folded by group_of (maximum per paper, ties to the lower row).
// A paper outside the true top-P may be folded from a part of its rows only: its partial maximum is <= its score, so it cannot displace a
// true one.  With fewer than K non-empty groups t = -inf and every non-empty group is a candidate.  The K-th largest of up to n_rows / 64
// values is a block-wide radix select over order_key, one bit per step (the wave selection of k <= 32 does not stretch to K <= 512).
// The chunks: for each selected paper every visible row of its WHOLE run is scored (its other chunks need not lie in candidate groups);
// the run's ends come from two binary searches in group_of.
// The exhaustive path (a query whose candidate list overflows cand_cap; the whole call when K > 512; path 2): every visible row scored by
// the same function in parts cut at run boundaries - no paper straddles two parts, so the per-part top-P paper lists merge as plain
// lists - then the same chunk step.  Same bits.
// No float atomics; integer atomics only where the result does not depend on their order (a counter, a maximum, the slots of a list that
// is read as a set); plain vector stores.  A query's output depends on the query, the mask, group_of and the corpus alone.
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

#define GRP_KSEL_MAX 512             // largest K = P S the scan path selects for; beyond: the exhaustive path
#define GRP_CHUNKS_MAX 8             // largest m

// ---- runs of group_of ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t run_lower(const int32_t* __restrict__ g, int64_t n, int32_t v) {      // first row with g[row] >= v
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (g[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ int64_t run_upper(const int32_t* __restrict__ g, int64_t from, int64_t n, int32_t v) {      // first row >= from with g[row] > v
    int64_t lo = from, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (g[mid] <= v) lo = mid + 1; else hi = mid; }
    return lo;
}
// the bits of word g that name rows of [a, b)
__device__ __forceinline__ uint64_t range_bits(int64_t a, int64_t b, int64_t g) {
    const int64_t base = g * GROUP_ROWS;
    const int64_t l = a > base ? a - base : 0, h = b - base < GROUP_ROWS ? b - base : GROUP_ROWS;
    if (h <= l) return 0ull;
    return (h >= GROUP_ROWS ? ~0ull : ((1ull << h) - 1ull)) & ~((1ull << l) - 1ull);
}

// out[0] = the longest run (all ones = -1 as int64: group_of decreases somewhere or holds a negative value), out[1] = the number of runs;
// both start at zero.  A maximum and a counter: the order of the atomics does not matter.  The thread of a run's first row finds the run's
// end by binary search (on unsorted input the search still ends, and the answer is -1 whatever it finds).
__global__ __launch_bounds__(256) void group_runs_kernel(const int32_t* __restrict__ g, int64_t n, unsigned long long* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t v = g[i];
        const bool first = i == 0;
        const int32_t prev = first ? v : g[i - 1];
        if (v < 0 || prev > v) atomicMax(&out[0], ~0ull);
        if (first || prev != v) {
            atomicMax(&out[0], (unsigned long long)(run_upper(g, i + 1, n, v) - i));
            atomicAdd(&out[1], 1ull);
        }
    }
}

// ---- the fold by paper ----------------------------------------------------------------------------------------------------------------------
// Every lane holds R candidates (score, row, paper) in registers, row < 0 = empty.  P rounds: the best remaining candidate by (score desc,
// row asc) is the next paper's best chunk, and every candidate of that paper retires.  Entry r of (out_s, out_i, out_g) = the r-th paper,
// (-inf, -1, -1) when fewer than P papers are held.
template <int R>
__device__ __forceinline__ void wave_top_papers(float (&s)[R], int64_t (&id)[R], int32_t (&pg)[R], int P, int lane, float* out_s,
                                                int64_t* out_i, int32_t* out_g) {
    for (int r = 0; r < P; ++r) {
        float bs = -INFINITY; int64_t bi = INT64_MAX; int bj = -1; int32_t bp = -1;
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (id[j] >= 0 && (bj < 0 || s[j] > bs || (s[j] == bs && id[j] < bi))) { bs = s[j]; bi = id[j]; bj = j; bp = pg[j]; }
        float ws = bj >= 0 ? bs : -INFINITY; int64_t wi = bj >= 0 ? bi : INT64_MAX;
        wave_argbest(ws, wi);
        const bool found = wi != INT64_MAX;                     // wave-uniform
        const unsigned long long own = __ballot(found && bj >= 0 && bi == wi);      // rows are distinct: one lane
        const int32_t wp = found ? __shfl(bp, own ? __ffsll((long long)own) - 1 : 0) : -1;
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (found && pg[j] == wp) id[j] = -1;
        if (lane == 0) { out_s[r] = found ? ws : -INFINITY; out_i[r] = found ? wi : -1; out_g[r] = wp; }
    }
}
// one wave: fold 64 new (score, row, paper) into the wave's running list of the P best papers, kept as entry `lane` of (cs, ci, cp) for
// lanes < P.  Skipped when no new score reaches the P-th kept one (ties included: they may win on the row number): the list holds P
// distinct papers that all rank before such a row.
__device__ __forceinline__ void wave_merge_papers(float& cs, int64_t& ci, int32_t& cp, float ns, int64_t ni, int32_t np, int P, int lane,
                                                  float* w_s, int64_t* w_i, int32_t* w_g) {
    const float pth = __shfl(cs, P - 1);
    if (!__any(ni >= 0 && ns >= pth)) return;                  // wave-uniform
    float s2[2] = {cs, ns};
    int64_t i2[2] = {ci, ni};
    int32_t g2[2] = {cp, np};
    wave_top_papers<2>(s2, i2, g2, P, lane, w_s, w_i, w_g);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    cs = lane < P ? w_s[lane] : -INFINITY;
    ci = lane < P ? w_i[lane] : -1;
    cp = lane < P ? w_g[lane] : -1;
}
// the block's NW per-wave paper lists (entries of lanes < P) -> the final P, by wave 0
template <int NW>
__device__ __forceinline__ void block_merge_papers(const float (*w_s)[KMAX], const int64_t (*w_i)[KMAX], const int32_t (*w_g)[KMAX], int P,
                                                   int lane, float* fin_s, int64_t* fin_i, int32_t* fin_g) {
    constexpr int R4 = (NW * KMAX + 63) / 64;
    float s[R4]; int64_t id[R4]; int32_t pg[R4];
#pragma unroll
    for (int j = 0; j < R4; ++j) {
        const int i = j * 64 + lane;
        s[j] = i < NW * P ? w_s[i / P][i % P] : -INFINITY;
        id[j] = i < NW * P ? w_i[i / P][i % P] : -1;
        pg[j] = i < NW * P ? w_g[i / P][i % P] : -1;
    }
    wave_top_papers<R4>(s, id, pg, P, lane, fin_s, fin_i, fin_g);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- the chunk step: wave w of NW takes papers w, w + NW, ... of the query's P selected ones (fin_i: the row of the best chunk, < 0 = no
// such paper; fin_g: its group_of value): the run's ends, every visible row of the run scored, the m best kept ---------------------------
__device__ __forceinline__ void paper_chunks(int w, int NW, int lane, const int64_t* fin_i, const int32_t* fin_g, int P, int m,
                                             const uint64_t* __restrict__ allow, const int32_t* __restrict__ group_of,
                                             const f16_t* __restrict__ C, int64_t n_rows, int D, const f16_t* qs, float* sc, float* w_s,
                                             int64_t* w_i, int64_t idx_base, float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                             int32_t* __restrict__ out_g) {
    for (int p = w; p < P; p += NW) {
        const int64_t best = fin_i[p];
        float cs = -INFINITY; int64_t ci = -1;
        if (best >= 0) {                                        // wave-uniform
            const int32_t gv = fin_g[p];
            const int64_t lo = run_lower(group_of, best, gv), hi = run_upper(group_of, best + 1, n_rows, gv);
            for (int64_t g = lo >> 6; g <= ((hi - 1) >> 6); ++g) {
                const uint64_t word = allow[g] & valid_bits(n_rows, g) & range_bits(lo, hi, g);
                if (word == 0ull) continue;
                score_word_rows(C, g, word, qs, D, lane, sc);
                const bool mine = (word >> lane) & 1ull;
                wave_merge64(cs, ci, mine ? sc[lane] : -INFINITY, mine ? g * GROUP_ROWS + lane : -1, m, lane, w_s, w_i);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
        if (lane < m) {
            out_s[(int64_t)p * m + lane] = cs;
            out_i[(int64_t)p * m + lane] = ci >= 0 ? ci + idx_base : -1;
        }
        if (lane == 0) out_g[p] = best >= 0 ? fin_g[p] : -1;
    }
}

// ---- the tail: one block per query ----------------------------------------------------------------------------------------------------------
// ksel = K of the header comment.  stats: [0] queries sent to the exhaustive path, [1] candidate groups rescored, [2] (low word) "some
// query of this call overflowed".  out_* point at this batch's first query.
__global__ __launch_bounds__(FILT_TAIL_NT) void grouped_tail_kernel(const float* __restrict__ gmax, int64_t ldg, int64_t n_groups,
                                                                     const uint64_t* __restrict__ allow, const int32_t* __restrict__ group_of,
                                                                     const f16_t* __restrict__ Q, const f16_t* __restrict__ C, int64_t n_rows,
                                                                     int D, int P, int m, int ksel, float* __restrict__ out_s,
                                                                     int64_t* __restrict__ out_i, int32_t* __restrict__ out_g, int64_t idx_base,
                                                                     float tau_scale, int cand_cap, int32_t* __restrict__ redo,
                                                                     unsigned long long* __restrict__ stats) {
    constexpr int NT = FILT_TAIL_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ int32_t w_g[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ int32_t fin_g[KMAX];
    __shared__ TailStage st;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);                                                  // [D] query row
    float* sc_all = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15));      // [NW][64] row scores of the group a wave is at
    int32_t* list = reinterpret_cast<int32_t*>(sc_all + NW * GROUP_ROWS);                        // [cand_cap] candidate groups
    load_query_row<NT>(qs, Q, q, D);
    if (tid == 0) st.n_c = 0;
    const float* col = gmax + q;                                                                 // this query's column of group maxima
    uint32_t kv[FILT_REG_GROUPS];
    const uint32_t T = tail_kth_key(st, kv, col, ldg, n_groups, qs, D, ksel);      // the ksel-th largest group maximum
    const float thr = key_value(T) - 2.0f * tau_scale * st.qn;      // -inf when fewer than ksel groups hold a visible row
    const int nc = tail_candidates(st, kv, col, ldg, n_groups, thr, list, cand_cap, q, redo, stats);
    if (nc < 0) return;                                        // block-uniform: flagged for the exhaustive path
    // the visible rows of the candidate groups, exactly, folded by paper: a group per wave at a time
    float* sc = sc_all + w * GROUP_ROWS;
    float cs = -INFINITY; int64_t ci = -1; int32_t cp = -1;
    for (int p = w; p < nc; p += NW) {
        const int64_t gsel = list[p];
        const uint64_t word = allow[gsel] & valid_bits(n_rows, gsel);
        score_word_rows(C, gsel, word, qs, D, lane, sc);
        const bool mine = (word >> lane) & 1ull;
        const int64_t row = gsel * GROUP_ROWS + lane;
        wave_merge_papers(cs, ci, cp, mine ? sc[lane] : -INFINITY, mine ? row : -1, mine ? group_of[row] : -1, P, lane, w_s[w], w_i[w], w_g[w]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (lane < P) { w_s[w][lane] = cs; w_i[w][lane] = ci; w_g[w][lane] = cp; }
    __syncthreads();
    if (w == 0) block_merge_papers<NW>(w_s, w_i, w_g, P, lane, fin_s, fin_i, fin_g);
    __syncthreads();
    paper_chunks(w, NW, lane, fin_i, fin_g, P, m, allow, group_of, C, n_rows, D, qs, sc, w_s[w], w_i[w], idx_base,
                 out_s + (int64_t)q * P * m, out_i + (int64_t)q * P * m, out_g + (int64_t)q * P);
}

// ---- exhaustive path: block (part p, query q) folds the visible rows of part p by paper -> part_s / part_i [parts][nq][P] (local rows).
// Part p starts at the first row of the run that row p * per lies in: no paper straddles two parts.  only_if / gate as masked_topk.h's.
__device__ __forceinline__ int64_t part_cut(const int32_t* __restrict__ group_of, int64_t n_rows, int64_t per, int p) {
    const int64_t s = (int64_t)p * per;
    if (p == 0) return 0;
    if (s >= n_rows) return n_rows;
    return run_lower(group_of, s, group_of[s]);
}
__global__ __launch_bounds__(256) void grouped_exhaustive_kernel(const uint64_t* __restrict__ allow, const int32_t* __restrict__ group_of,
                                                                  const f16_t* __restrict__ Q, const f16_t* __restrict__ C, int64_t n_rows,
                                                                  int D, int nq, int P, float* __restrict__ part_s,
                                                                  int64_t* __restrict__ part_i, const int32_t* __restrict__ only_if,
                                                                  const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int q = blockIdx.y, p = blockIdx.x, parts = gridDim.x;
    if (only_if && !only_if[q]) return;
    constexpr int NW = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ int32_t w_g[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ int32_t fin_g[KMAX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    float* sc = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15)) + w * GROUP_ROWS;
    load_query_row<256>(qs, Q, q, D);
    __syncthreads();
    const int64_t per = ((n_rows + parts - 1) / parts + 63) / 64 * 64;
    const int64_t a = part_cut(group_of, n_rows, per, p), b = p + 1 < parts ? part_cut(group_of, n_rows, per, p + 1) : n_rows;
    float cs = -INFINITY; int64_t ci = -1; int32_t cp = -1;
    if (a < b)
        for (int64_t g = (a >> 6) + w; g <= ((b - 1) >> 6); g += NW) {
            const uint64_t word = allow[g] & valid_bits(n_rows, g) & range_bits(a, b, g);
            if (word == 0ull) continue;                        // wave-uniform
            score_word_rows(C, g, word, qs, D, lane, sc);
            const bool mine = (word >> lane) & 1ull;
            const int64_t row = g * GROUP_ROWS + lane;
            wave_merge_papers(cs, ci, cp, mine ? sc[lane] : -INFINITY, mine ? row : -1, mine ? group_of[row] : -1, P, lane, w_s[w], w_i[w], w_g[w]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    if (lane < P) { w_s[w][lane] = cs; w_i[w][lane] = ci; w_g[w][lane] = cp; }
    __syncthreads();
    if (w == 0) {
        block_merge_papers<NW>(w_s, w_i, w_g, P, lane, fin_s, fin_i, fin_g);
        if (lane < P) {
            const int64_t o = ((int64_t)p * nq + q) * P + lane;
            part_s[o] = fin_s[lane];
            part_i[o] = fin_i[lane];
        }
    }
}

// the chunk step of the queries the exhaustive path answered: sel_i [nq][P] = the merged lists' rows (best chunk of each selected paper)
__global__ __launch_bounds__(FILT_TAIL_NT) void grouped_chunks_kernel(const int64_t* __restrict__ sel_i, const uint64_t* __restrict__ allow,
                                                                       const int32_t* __restrict__ group_of, const f16_t* __restrict__ Q,
                                                                       const f16_t* __restrict__ C, int64_t n_rows, int D, int P, int m,
                                                                       float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                                       int32_t* __restrict__ out_g, int64_t idx_base,
                                                                       const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int q = blockIdx.x;
    if (only_if && !only_if[q]) return;
    constexpr int NT = FILT_TAIL_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ int32_t fin_g[KMAX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    float* sc = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15)) + w * GROUP_ROWS;
    load_query_row<NT>(qs, Q, q, D);
    if (tid < P) {
        const int64_t row = sel_i[(int64_t)q * P + tid];
        fin_i[tid] = row;
        fin_g[tid] = row >= 0 ? group_of[row] : -1;
    }
    __syncthreads();
    paper_chunks(w, NW, lane, fin_i, fin_g, P, m, allow, group_of, C, n_rows, D, qs, sc, w_s[w], w_i[w], idx_base,
                 out_s + (int64_t)q * P * m, out_i + (int64_t)q * P * m, out_g + (int64_t)q * P);
}

// ---- the search policy (masked_topk.h: the scan driver) -----------------------------------------------------------------------------------
struct GroupedSearch {
    int P, m; const int32_t* group_of; int64_t max_run_rows; float* out_s; int64_t* out_i; int32_t* out_g; int64_t idx_base;
    float* sel_s; int64_t* sel_i;        // workspace: the merged paper lists [nq][P] of the queries the exhaustive path answers
    float* part_s; int64_t* part_i;      // workspace: the exhaustive path's per-part paper lists [parts][nq][P]
    static constexpr const char* workspace_fn = "arx_topk_grouped_workspace_bytes";
    static constexpr size_t kSmemRaise = 48 * 1024;      // more dynamic LDS than this is asked for before the launch

    bool given() const { return group_of && out_s && out_i && out_g; }
    int check(int64_t) const {
        ARX_REQUIRE(P >= 1 && P <= KMAX, "n_groups=%d out of range 1..%d", P, KMAX);
        ARX_REQUIRE(m >= 1 && m <= GRP_CHUNKS_MAX, "chunks_per_group=%d out of range 1..%d", m, GRP_CHUNKS_MAX);
        ARX_REQUIRE(max_run_rows >= 1, "max_run_rows=%lld must be at least 1", (long long)max_run_rows);
        return ARX_OK;
    }
    void take_buffers(MaskedWs& w) {
        sel_s = w.take<float>((int64_t)w.qb * P * 4);
        sel_i = w.take<int64_t>((int64_t)w.qb * P * 8);
        part_s = w.take<float>((int64_t)w.parts * w.qb * P * 4);
        part_i = w.take<int64_t>((int64_t)w.parts * w.qb * P * 8);
    }
    // S = the 64-row groups a run of at most max_run_rows rows can touch, K = P S (the clamp only keeps the arithmetic in range)
    int64_t ksel() const {
        const int64_t R = max_run_rows < (1ll << 40) ? max_run_rows : (1ll << 40);
        return (int64_t)P * ((R + 62) / 64 + 1);
    }
    int resolve_path(const AllowRows&, int path, int) const { return ksel() > GRP_KSEL_MAX ? 2 : (path ? path : 1); }      // K too large: the whole call
    int default_cand_cap() const { return FILT_CAND_CAP_DEFAULT; }
    int launch_tail(const ScanSlice& s, const AllowRows& mask) const {
        const size_t smem = s.smem_q + (size_t)(FILT_TAIL_NT / 64) * GROUP_ROWS * 4 + (size_t)s.cand_cap * 4;
        if (smem > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)grouped_tail_kernel, (int)smem));
        grouped_tail_kernel<<<s.nq, FILT_TAIL_NT, smem, s.st>>>(s.L.gmax, s.L.ldg, s.L.n_groups, mask.allow, group_of, s.Q, s.C, s.n_rows, s.dim, P, m,
                                                                (int)ksel(), out_s + (int64_t)s.q0 * P * m, out_i + (int64_t)s.q0 * P * m,
                                                                out_g + (int64_t)s.q0 * P, idx_base, s.tau_scale, s.cand_cap, s.L.redo, s.L.stats);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    int launch_exhaustive(const ScanSlice& s, const AllowRows& mask) const {
        const size_t smem_x = s.smem_q + 4 * GROUP_ROWS * 4;
        if (smem_x > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)grouped_exhaustive_kernel, (int)smem_x));
        grouped_exhaustive_kernel<<<dim3(s.L.parts, s.nq), 256, smem_x, s.st>>>(mask.allow, group_of, s.Q, s.C, s.n_rows, s.dim, s.nq, P, part_s, part_i,
                                                                                s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        filter_merge_kernel<<<cdiv(s.nq, 4), 256, 0, s.st>>>(part_s, part_i, s.L.parts, s.nq, P, sel_s, sel_i, s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        const size_t smem_c = s.smem_q + (size_t)(FILT_TAIL_NT / 64) * GROUP_ROWS * 4;
        if (smem_c > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)grouped_chunks_kernel, (int)smem_c));
        grouped_chunks_kernel<<<s.nq, FILT_TAIL_NT, smem_c, s.st>>>(sel_i, mask.allow, group_of, s.Q, s.C, s.n_rows, s.dim, P, m,
                                                                    out_s + (int64_t)s.q0 * P * m, out_i + (int64_t)s.q0 * P * m,
                                                                    out_g + (int64_t)s.q0 * P, idx_base, s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
};
}      // namespace

extern "C" int64_t arx_topk_grouped_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t n_groups, int32_t chunks_per_group) {
    if (n_rows <= 0 || n_rows >= (1ll << 36) || n_queries <= 0 || dim <= 0 || dim % 64 != 0 || dim > 8192 || n_groups <= 0 || n_groups > KMAX ||
        chunks_per_group <= 0 || chunks_per_group > GRP_CHUNKS_MAX)
        return -1;
    GroupedSearch search{n_groups};
    return scan_layout<AllowRows>(search, n_rows, n_queries, nullptr).total;
}

extern "C" int32_t arx_group_runs_info(const int32_t* group_of, int64_t n_rows, int64_t* out, void* stream) {
    ARX_REQUIRE(group_of && out, "null pointer argument");
    ARX_REQUIRE(n_rows >= 0, "n_rows=%lld must not be negative", (long long)n_rows);
    hipStream_t st = (hipStream_t)stream;
    ARX_HIP_CHECK(hipMemsetAsync(out, 0, 16, st));
    if (n_rows == 0) return ARX_OK;
    const int64_t blocks = (n_rows + 255) / 256;
    group_runs_kernel<<<(int)(blocks < 4096 ? blocks : 4096), 256, 0, st>>>(group_of, n_rows, (unsigned long long*)out);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_topk_search_grouped_tuned(const void* corpus, int64_t n_rows, const int32_t* group_of, int64_t max_run_rows,
                                                 const uint64_t* allow, int64_t n_allowed, const void* queries, int32_t n_queries, int32_t dim,
                                                 int32_t n_groups, int32_t chunks_per_group, float* out_scores, int64_t* out_ids,
                                                 int32_t* out_groups, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes,
                                                 int32_t path, int32_t cand_cap, void* stream) {
    return masked_scan(AllowRows{{allow}, n_allowed},
                       GroupedSearch{n_groups, chunks_per_group, group_of, max_run_rows, out_scores, out_ids, out_groups, idx_base}, corpus, n_rows,
                       queries, n_queries, dim, max_row_norm, ws, ws_bytes, path, cand_cap, stream);
}

extern "C" int32_t arx_topk_search_grouped(const void* corpus, int64_t n_rows, const int32_t* group_of, int64_t max_run_rows,
                                           const uint64_t* allow, int64_t n_allowed, const void* queries, int32_t n_queries, int32_t dim,
                                           int32_t n_groups, int32_t chunks_per_group, float* out_scores, int64_t* out_ids,
                                           int32_t* out_groups, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, void* stream) {
    return arx_topk_search_grouped_tuned(corpus, n_rows, group_of, max_run_rows, allow, n_allowed, queries, n_queries, dim, n_groups,
                                         chunks_per_group, out_scores, out_ids, out_groups, idx_base, max_row_norm, ws, ws_bytes, 0, 0, stream);
}

extern "C" int32_t arx_topk_grouped_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    return masked_stats(ws, overflowed_queries, candidate_groups, stream);
}
