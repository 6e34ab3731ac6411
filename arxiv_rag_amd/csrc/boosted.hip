// arx_topk_search_boosted: the exact top-k of an fp16 shard under  cosine + weight * prior  (C ABI in include/arx.h; score boosting, a
// rank profile).  prior (device f32 [n_rows]) holds one value per row, weight (device f32 [n_queries]) one per query, and an optional
// bitmap in the convention of arx_topk_search_filtered says which rows may be returned.
//   visible        row r for query q: its bit is set (or there is no bitmap) and p(q, r) = fl32(weight[q] * prior[r]) is finite.  With a
//                  finite weight and a product that does not overflow - what the host wrapper admits - that is "prior[r] is finite"; a NaN
//                  or +-inf prior hides the row from every query, a non-finite weight hides every row from its query, and no NaN is ever
//                  ranked or returned
//   base(q, r)     exact_row_score (search_tail.h): the bits arx_topk_search and arx_topk_search_filtered give the pair
//   boosted(q, r)  fl32(base(q, r) + p(q, r)): two separately rounded f32 operations (boost_term, boost_score below: __fmul_rn and
//                  __fadd_rn, and the file is compiled without FMA contraction, as fuse.hip is); numpy: base + np.float32(w) * prior
//   answer         the k <= 32 best visible rows by (boosted desc, row asc) as three arrays: the boosted scores, the base scores of the
//                  same rows, the ids (row + idx_base); (-inf, -inf, -1) padding
// The host side is masked_topk.h's scan driver (masked_scan) with BoostedSearch below as its search policy and BoostedMask as its mask:
// filter.hip's BitmapMask over the EFFECTIVE bitmap (the caller's bitmap, or all ones, AND "the prior is finite": boost_prepare_kernel
// writes it into the workspace ahead of the first slice), plus pass A's prior policy.
//   pass A        masked_groupmax_kernel with the prior policy: fl32(acc + p) stands for a row in front of the maximum over a group's
//                 64 rows, -inf where p is not finite; gmax[group][query] = the largest APPROXIMATE boosted score of the group's visible
//                 rows.  256-row tiles without an effective bit are skipped as before.
//   the tail      boosted_tail_kernel, one block per query, on masked_topk.h's stage (tail_kth_key, tail_candidates): t = the k-th largest
//                 group maximum, candidates = every non-empty group with gmax >= t - 2 tau_b, their visible rows rescored exactly
//                 (exact_row_score, then the two rounded operations), top-k by (boosted desc, row asc); the base scores of the k winners
//                 are their exact_row_score once more (the same function of the same bytes: the same bits)
//   exhaustive    every row of the effective bitmap's list scored by the same functions (a query whose candidate list overflows; path 2;
//                 path 0 for a selective bitmap, as filter.hip chooses), per-part lists merged, then the winners' base scores.  Same bits.
// The tolerance tau_b, and why the tail is exact.  For a visible (q, r) let A be pass A's accumulator, E = base(q, r) and p the rounded
// product; pass A and the rescoring use the SAME p (same operation, same operands).  |A - E| <= tau = tau_scale |q| (masked_tau_scale:
// rescore_kernel step 5).  Pass A ranks a = fl32(A + p), the answer ranks b = fl32(E + p).  A rounded add is off by at most 2^-24 of its
// result, and |A + p|, |E + p| <= N |q| + tau + |w| M with N the rows' norm bound and M = max_abs_prior >= |prior[r]|, so
//   |a - b| <= |A - E| + 2^-24 (|a| + |b|) <= tau + 2^-23 (1 + 2^-24) (N |q| + tau + |w| M) <= tau_b := tau + 1.5 * 2^-23 (N |q| + |w| M)
// (tau <= 1.6e-4 N |q| at dim <= 8192, and |q| itself is computed within 5e-4 of its value: both sit inside the factor 1.5).  With tau_b in
// tau's place masked_tail_kernel's argument holds word for word: k distinct groups hold a visible row with a >= t, so the k-th exact
// boosted score is >= t - tau_b, and every row that reaches it has a >= t - 2 tau_b: it sits in a candidate group.  The widening grows
// with |w| M: a large weight on a prior with many equal values (or prior = -base) puts many groups within 2 tau_b of t, the list
// overflows and the query takes the exhaustive path - slower, same bits.  max_abs_prior is the caller's contract as max_row_norm is
// (arx_prior_info measures it): too small voids the argument, too large only widens the candidate set.  |w| M not finite: t - 2 tau_b is
// -inf or NaN, and the query lists every non-empty group or none; the host wrapper refuses such a call.
// No float atomics; integer atomics only where the result does not depend on their order (a counter, a maximum, the slots of a list that
// is read as a set); plain vector stores.  A query's output depends on its row of Q, its weight, the prior, the bitmap and the corpus alone.
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

// as filter.hip's: path = 0 with n_allowed known takes the exhaustive path below this many (allowed row, query) pairs
#define BOOST_EXHAUSTIVE_MAX_PAIRS_WIDE (1ll << 20)
#define BOOST_EXHAUSTIVE_MAX_PAIRS (1ll << 18)
#define BOOST_WIDE_NQ 64

// ---- the score: the ONE definition of the two rounded operations, for pass A, the tail and the exhaustive path ------------------------------
__device__ __forceinline__ float boost_term(float w, float prior) { return __fmul_rn(w, prior); }
__device__ __forceinline__ bool boost_visible(float p) { return fabsf(p) < INFINITY; }      // false for NaN
__device__ __forceinline__ float boost_score(float base, float p) { return __fadd_rn(base, p); }

// ---- ahead of a slice's pass A: the slice's weights -> wq; ahead of the first slice also the effective bitmap, one lane per row ------------
__global__ __launch_bounds__(256) void boost_prepare_kernel(const uint64_t* __restrict__ allow, const float* __restrict__ prior, int64_t n_rows,
                                                             int64_t n_words, uint64_t* __restrict__ eff, const float* __restrict__ weight,
                                                             int nq, float* __restrict__ wq, int with_bitmap) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nq) wq[i] = weight[i];
    if (!with_bitmap) return;
    const int64_t wd = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wd >= n_words) return;                                 // wave-uniform
    const int64_t row = wd * GROUP_ROWS + lane;
    const bool fin = row < n_rows && fabsf(prior[row < n_rows ? row : 0]) < INFINITY;
    const uint64_t word = __ballot(fin) & (allow ? allow[wd] : ~0ull);
    if (lane == 0) eff[wd] = word;
}

// ---- the mask policy (masked_topk.h): filter.hip's bitmap policy over the effective bitmap, and pass A's prior policy -----------------------
struct BoostedMask : BitmapRows {      // `allow` = the effective bitmap (set by bind)
    int64_t n_allowed;          // the caller's count of the set bits of ITS bitmap, -1 = unknown (host only)
    const float* prior;         // [n_rows]
    const float* weight;        // [n_queries], the call's
    const uint64_t* user_allow; // the caller's bitmap, null = every row
    uint64_t* eff;              // workspace: the effective bitmap
    float* wq;                  // workspace: the weights of the slice at hand
    int64_t* off;               // workspace: [n_groups + 1] offsets of the words' rows in `rows`
    int64_t* rows;              // workspace: the effective bitmap's rows in ascending order
    const int64_t* n_list;      // = off + n_groups: their number

    // pass A: the prior policy
    struct RowPrior {
        static constexpr bool kOn = true;
        float w;
        const float (*p)[4];
        // what stands for the row in front of the group maximum: the approximate boosted score, -inf for a row the query does not see
        __device__ __forceinline__ float operator()(float acc, int j, int r) const {
            const float t = boost_term(w, p[j][r]);
            return boost_visible(t) ? boost_score(acc, t) : -INFINITY;
        }
    };
    struct PriorRows {
        float p[GROUP_ROWS / 16][4]; const float* wq;
        __device__ __forceinline__ RowPrior of_query(int m, int nq) const { return {m < nq ? wq[m] : 0.0f, p}; }
    };
    // rows j*16 + (lane>>4)*4 + 0..3 of group g: one 16-byte load per j (prior is 16-byte aligned); past the shard's end: NaN = not visible
    __device__ __forceinline__ PriorRows prior_rows(int64_t g, int lane, int64_t n_rows) const {
        PriorRows s;
        s.wq = wq;
#pragma unroll
        for (int j = 0; j < GROUP_ROWS / 16; ++j) {
            const int64_t row0 = g * GROUP_ROWS + j * 16 + (lane >> 4) * 4;
            if (row0 + 3 < n_rows) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(prior + row0);
#pragma unroll
                for (int r = 0; r < 4; ++r) s.p[j][r] = v[r];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) s.p[j][r] = row0 + r < n_rows ? prior[row0 + r] : __uint_as_float(0x7fc00000u);
            }
        }
        return s;
    }
    // exhaustive
    __device__ __forceinline__ int64_t list_total(int) const { return *n_list; }
    static constexpr bool kListInMemory = true;
    __device__ __forceinline__ int64_t list_row(int, int64_t pos) const { return rows[pos]; }

    // host
    bool given() const { return prior && weight; }
    int check(int64_t n_rows) const {
        ARX_REQUIRE(n_allowed >= -1 && n_allowed <= n_rows, "n_allowed=%lld", (long long)n_allowed);
        return ARX_OK;
    }
    int choose_path(int32_t n_queries) const {
        return (n_allowed >= 0 && n_allowed * (int64_t)n_queries < (n_queries >= BOOST_WIDE_NQ ? BOOST_EXHAUSTIVE_MAX_PAIRS_WIDE : BOOST_EXHAUSTIVE_MAX_PAIRS))
                   ? 2 : 1;
    }
    // own[0]: off, the effective bitmap, the slice's weights, each rounded up to 256 bytes; own[1]: rows
    static int64_t off_bytes(const MaskedWs& L) { return round_up64((L.n_groups + 1) * 8, 256); }
    static int64_t eff_bytes(const MaskedWs& L) { return round_up64(L.n_groups * 8, 256); }
    static void own_bytes(const MaskedWs& L, int64_t n_rows, int64_t b[2]) { b[0] = off_bytes(L) + eff_bytes(L) + (int64_t)L.qb * 4; b[1] = n_rows * 8; }
    void bind(char* ws, const MaskedWs& L) {
        off = (int64_t*)(ws + L.own[0]);
        eff = (uint64_t*)(ws + L.own[0] + off_bytes(L));
        wq = (float*)(ws + L.own[0] + off_bytes(L) + eff_bytes(L));
        rows = (int64_t*)(ws + L.own[1]);
        n_list = off + L.n_groups;
        allow = eff;
    }
    int prepare_batch(int q0, int nq, int64_t n_rows, hipStream_t st) const {
        const int64_t n_words = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
        const int by_q = cdiv(nq, 256), by_w = cdiv(n_words, 4);      // a thread per weight; ahead of the first slice also a wave per word
        const int blocks = q0 == 0 && by_w > by_q ? by_w : by_q;
        boost_prepare_kernel<<<blocks, 256, 0, st>>>(user_allow, prior, n_rows, n_words, eff, weight + q0, nq, wq, q0 == 0);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    int prepare_lists(int q0, int path, int64_t n_rows, int64_t n_groups, const int* gate, hipStream_t st) const {
        if (q0 == 0 || path == 1) {                            // (the list does not depend on the batch; after an overflow it is built then)
            filter_scan_kernel<<<1, 1024, 0, st>>>(eff, n_groups, n_rows, off, gate);
            ARX_HIP_CHECK(hipGetLastError());
            filter_scatter_kernel<<<cdiv(n_groups, 4), 256, 0, st>>>(eff, n_groups, n_rows, off, rows, gate);
            ARX_HIP_CHECK(hipGetLastError());
        }
        return ARX_OK;
    }
};

// the base scores of a final list: one wave, ids = the k winners' local rows in LDS (< 0 = empty), 8 lanes per row -> out_b[0 .. k)
__device__ __forceinline__ void wave_base_scores(const f16_t* __restrict__ C, const f16_t* qs, int D, const int64_t* ids, int k, int lane,
                                                 float* __restrict__ out_b) {
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    for (int r8 = 0; r8 < k; r8 += 8) {                        // wave-uniform
        const int e = r8 + rsub;
        const int64_t row = e < k ? ids[e] : -1;
        const bool ok = row >= 0;
        const float a = exact_row_score(C + (ok ? row : 0) * D, qs, nch, l8, ok);
        if (l8 == 0 && e < k) out_b[e] = ok ? a : -INFINITY;
    }
}

// ---- the tail: one block per query (see the header comment).  stats: [0] queries sent to the exhaustive path, [1] candidate groups
// rescored, [2] (low word) "some query of this call overflowed".  out_* and wq point at this batch's first query. -------------------------
__global__ __launch_bounds__(FILT_TAIL_NT) void boosted_tail_kernel(const float* __restrict__ gmax, int64_t ldg, int64_t n_groups,
                                                                     const uint64_t* __restrict__ eff, const float* __restrict__ prior,
                                                                     const float* __restrict__ wq, const f16_t* __restrict__ Q,
                                                                     const f16_t* __restrict__ C, int64_t n_rows, int D, int k,
                                                                     float* __restrict__ out_s, float* __restrict__ out_b,
                                                                     int64_t* __restrict__ out_i, int64_t idx_base, float tau_scale,
                                                                     float norm_bound, float max_abs_prior, int cand_cap,
                                                                     int32_t* __restrict__ redo, unsigned long long* __restrict__ stats) {
    constexpr int NT = FILT_TAIL_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ TailStage st;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);                                                  // [D] query row
    float* sc_all = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15));      // [NW][64] row scores of the group a wave is at
    int32_t* list = reinterpret_cast<int32_t*>(sc_all + NW * GROUP_ROWS);                        // [cand_cap] candidate groups
    load_query_row<NT>(qs, Q, q, D);
    if (tid == 0) st.n_c = 0;
    const float wt = wq[q];
    const float* col = gmax + q;                                                                 // this query's column of group maxima
    uint32_t kv[FILT_REG_GROUPS];
    const uint32_t T = tail_kth_key(st, kv, col, ldg, n_groups, qs, D, k);                       // the k-th largest group maximum
    const float tau_b = tau_scale * st.qn + 1.5f * 1.1920929e-7f * (norm_bound * st.qn + fabsf(wt) * max_abs_prior);
    const float thr = key_value(T) - 2.0f * tau_b;             // -inf when fewer than k groups hold a visible row
    const int nc = tail_candidates(st, kv, col, ldg, n_groups, thr, list, cand_cap, q, redo, stats);
    if (nc < 0) return;                                        // block-uniform: flagged for the exhaustive path
    // the visible rows of the candidate groups, exactly: a group per wave at a time
    float* sc = sc_all + w * GROUP_ROWS;
    float cs = -INFINITY; int64_t ci = -1;
    for (int p = w; p < nc; p += NW) {
        const int64_t gsel = list[p];
        const int64_t row = gsel * GROUP_ROWS + lane;
        const bool bit = (eff[gsel] >> lane) & 1ull && row < n_rows;
        const float pt = boost_term(wt, prior[bit ? row : 0]);
        const bool mine = bit && boost_visible(pt);
        const uint64_t word = __ballot(mine);
        score_word_rows(C, gsel, word, qs, D, lane, sc);
        wave_merge64(cs, ci, mine ? boost_score(sc[lane], pt) : -INFINITY, mine ? row : -1, k, lane, w_s[w], w_i[w]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (lane < k) { w_s[w][lane] = cs; w_i[w][lane] = ci; }
    __syncthreads();
    if (w == 0) {
        block_merge_lists<NW>(w_s, w_i, k, lane, fin_s, fin_i);
        if (lane < k) {
            out_s[(int64_t)q * k + lane] = fin_s[lane];
            out_i[(int64_t)q * k + lane] = fin_i[lane] >= 0 ? fin_i[lane] + idx_base : -1;
        }
        wave_base_scores(C, qs, D, fin_i, k, lane, out_b + (int64_t)q * k);
    }
}

// ---- exhaustive path: block (part p, query q) scores the p-th stretch of the effective bitmap's row list -> part_s / part_i
// [parts][nq][k] (masked_exhaustive_kernel with the boosted score).  only_if / gate as masked_topk.h's. -----------------------------------
__global__ __launch_bounds__(256) void boosted_exhaustive_kernel(const BoostedMask mask, const f16_t* __restrict__ Q, const f16_t* __restrict__ C,
                                                                  int D, int nq, int k, int64_t idx_base, float* __restrict__ part_s,
                                                                  int64_t* __restrict__ part_i, const int32_t* __restrict__ only_if,
                                                                  const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int q = blockIdx.y, p = blockIdx.x, P = gridDim.x;
    if (only_if && !only_if[q]) return;
    constexpr int NW = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    float* sc = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15)) + w * GROUP_ROWS;
    load_query_row<256>(qs, Q, q, D);
    __syncthreads();
    const float wt = mask.wq[q];
    const int64_t total = mask.list_total(q);
    const int64_t per = ((total + P - 1) / P + 63) / 64 * 64;
    const int64_t lo = (int64_t)p * per, hi = (lo + per < total) ? lo + per : total;
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float cs = -INFINITY; int64_t ci = -1;
    for (int64_t base = lo + (int64_t)w * 64; base < hi; base += NW * 64) {
        const int64_t listed = base + lane < hi ? mask.list_row(q, base + lane) : -1;
        const float pt = boost_term(wt, mask.prior[listed >= 0 ? listed : 0]);
        const int64_t mine = listed >= 0 && boost_visible(pt) ? listed : -1;
        for (int r8 = 0; r8 < 64; r8 += 8) {
            if (base + r8 >= hi) break;                        // wave-uniform
            const int64_t row = __shfl(mine, r8 + rsub);
            const bool ok = row >= 0;
            const float a = exact_row_score(C + (ok ? row : 0) * D, qs, nch, l8, ok);
            if (l8 == 0) sc[r8 + rsub] = a;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wave_merge64(cs, ci, mine >= 0 ? boost_score(sc[lane], pt) : -INFINITY, mine, k, lane, w_s[w], w_i[w]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (lane < k) { w_s[w][lane] = cs; w_i[w][lane] = ci; }
    __syncthreads();
    if (w == 0) {
        block_merge_lists<NW>(w_s, w_i, k, lane, fin_s, fin_i);
        if (lane < k) {
            const int64_t o = ((int64_t)p * nq + q) * k + lane;
            part_s[o] = fin_s[lane];
            part_i[o] = fin_i[lane] >= 0 ? fin_i[lane] + idx_base : -1;
        }
    }
}

// the base scores of the queries the exhaustive path answered: one wave per query over its merged list out_i (ids with idx_base)
__global__ __launch_bounds__(64) void boosted_base_kernel(const int64_t* __restrict__ out_i, const f16_t* __restrict__ Q, const f16_t* __restrict__ C,
                                                           int D, int k, int64_t idx_base, float* __restrict__ out_b,
                                                           const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int q = blockIdx.x, lane = threadIdx.x;
    if (only_if && !only_if[q]) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int64_t ids[KMAX];
    f16_t* qs = reinterpret_cast<f16_t*>(smem);
    load_query_row<64>(qs, Q, q, D);
    if (lane < k) {
        const int64_t id = out_i[(int64_t)q * k + lane];
        ids[lane] = id >= 0 ? id - idx_base : -1;
    }
    __syncthreads();
    wave_base_scores(C, qs, D, ids, k, lane, out_b + (int64_t)q * k);
}

// ---- the search policy (masked_topk.h: the scan driver) -----------------------------------------------------------------------------------
struct BoostedSearch {
    int k; float* out_s; float* out_b; int64_t* out_i; int64_t idx_base; float norm_bound, max_abs_prior;
    float* part_s; int64_t* part_i;      // workspace: the exhaustive path's per-part lists [parts][nq][k]
    static constexpr const char* workspace_fn = "arx_topk_search_boosted_workspace_bytes";
    static constexpr size_t kSmemRaise = 48 * 1024;      // more dynamic LDS than this is asked for before the launch

    bool given() const { return out_s && out_b && out_i; }
    int check(int64_t) const {
        ARX_REQUIRE(k > 0 && k <= KMAX, "k=%d out of range 1..%d", k, KMAX);
        ARX_REQUIRE(max_abs_prior >= 0.0f && max_abs_prior < INFINITY, "max_abs_prior=%g: must be a finite bound on |prior|", (double)max_abs_prior);
        return ARX_OK;
    }
    void take_buffers(MaskedWs& w) {
        part_s = w.take<float>((int64_t)w.parts * w.qb * k * 4);
        part_i = w.take<int64_t>((int64_t)w.parts * w.qb * k * 8);
    }
    int resolve_path(const BoostedMask& mask, int path, int n_queries) const { return path ? path : mask.choose_path(n_queries); }
    int default_cand_cap() const { return FILT_CAND_CAP_DEFAULT; }
    int launch_tail(const ScanSlice& s, const BoostedMask& mask) const {
        const size_t smem = s.smem_q + (size_t)(FILT_TAIL_NT / 64) * GROUP_ROWS * 4 + (size_t)s.cand_cap * 4;
        if (smem > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)boosted_tail_kernel, (int)smem));
        boosted_tail_kernel<<<s.nq, FILT_TAIL_NT, smem, s.st>>>(s.L.gmax, s.L.ldg, s.L.n_groups, mask.eff, mask.prior, mask.wq, s.Q, s.C, s.n_rows,
                                                                s.dim, k, out_s + (int64_t)s.q0 * k, out_b + (int64_t)s.q0 * k,
                                                                out_i + (int64_t)s.q0 * k, idx_base, s.tau_scale, norm_bound, max_abs_prior,
                                                                s.cand_cap, s.L.redo, s.L.stats);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    int launch_exhaustive(const ScanSlice& s, const BoostedMask& mask) const {
        const size_t smem_x = s.smem_q + 4 * GROUP_ROWS * 4;
        if (smem_x > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)boosted_exhaustive_kernel, (int)smem_x));
        boosted_exhaustive_kernel<<<dim3(s.L.parts, s.nq), 256, smem_x, s.st>>>(mask, s.Q, s.C, s.dim, s.nq, k, idx_base, part_s, part_i, s.only_if,
                                                                                s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        filter_merge_kernel<<<cdiv(s.nq, 4), 256, 0, s.st>>>(part_s, part_i, s.L.parts, s.nq, k, out_s + (int64_t)s.q0 * k,
                                                             out_i + (int64_t)s.q0 * k, s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        boosted_base_kernel<<<s.nq, 64, s.smem_q, s.st>>>(out_i + (int64_t)s.q0 * k, s.Q, s.C, s.dim, k, idx_base, out_b + (int64_t)s.q0 * k,
                                                          s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
};

// out[0] = the bits of the largest |finite value| (a non-negative float's bits order as the unsigned integer they are), out[1] = the
// number of non-finite values; both start at zero.  A maximum and a counter: the order of the atomics does not matter.
__global__ __launch_bounds__(256) void prior_info_kernel(const float* __restrict__ prior, int64_t n, unsigned long long* __restrict__ out) {
    uint32_t mx = 0u; unsigned long long bad = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float a = fabsf(prior[i]);
        if (a < INFINITY) { const uint32_t u = __float_as_uint(a); mx = u > mx ? u : mx; }
        else ++bad;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t om = __shfl_xor(mx, o);
        mx = om > mx ? om : mx;
        bad += __shfl_xor(bad, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(&out[0], (unsigned long long)mx);
        if (bad) atomicAdd(&out[1], bad);
    }
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
}      // namespace

extern "C" int64_t arx_topk_search_boosted_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k) {
    if (n_rows <= 0 || n_rows >= (1ll << 36) || n_queries <= 0 || dim <= 0 || dim % 64 != 0 || dim > 8192 || k <= 0 || k > KMAX) return -1;
    BoostedSearch search{k};
    return scan_layout<BoostedMask>(search, n_rows, n_queries, nullptr).total;
}

extern "C" int32_t arx_prior_info(const float* prior, int64_t n_rows, int64_t* out, void* stream) {
    ARX_REQUIRE(prior && out, "null pointer argument");
    ARX_REQUIRE(!misaligned(prior, 4) && !misaligned(out, 8), "misaligned pointer argument: prior needs 4 bytes, out 8");
    ARX_REQUIRE(n_rows >= 0, "n_rows=%lld must not be negative", (long long)n_rows);
    hipStream_t st = (hipStream_t)stream;
    ARX_HIP_CHECK(hipMemsetAsync(out, 0, 16, st));
    if (n_rows == 0) return ARX_OK;
    const int64_t blocks = (n_rows + 255) / 256;
    prior_info_kernel<<<(int)(blocks < 4096 ? blocks : 4096), 256, 0, st>>>(prior, n_rows, (unsigned long long*)out);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_topk_search_boosted(const void* corpus, int64_t n_rows, const float* prior, float max_abs_prior, const float* weight,
                                           const uint64_t* allow, int64_t n_allowed, const void* queries, int32_t n_queries, int32_t dim,
                                           int32_t k, float* out_scores, float* out_base, int64_t* out_ids, int64_t idx_base,
                                           float max_row_norm, void* ws, int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream) {
    ARX_REQUIRE(corpus && prior && weight && queries && out_scores && out_base && out_ids && ws, "null pointer argument");
    ARX_REQUIRE(n_rows >= 0 && n_queries >= 0, "n_rows=%lld n_queries=%d: a size must not be negative", (long long)n_rows, n_queries);
    ARX_REQUIRE(!misaligned(corpus, 16) && !misaligned(queries, 16) && !misaligned(prior, 16) && !misaligned(ws, 16),
                "misaligned pointer argument: corpus, queries, prior and ws need 16 bytes");
    ARX_REQUIRE(!misaligned(weight, 4) && !misaligned(out_scores, 4) && !misaligned(out_base, 4) && !misaligned(out_ids, 8) && !misaligned(allow, 8),
                "misaligned pointer argument: weight, out_scores and out_base need 4 bytes, out_ids and allow 8");
    const float nb = max_row_norm > 0.0f ? max_row_norm : 1.0f + 1.0f / 512.0f;
    return masked_scan(BoostedMask{{nullptr}, n_allowed, prior, weight, allow}, BoostedSearch{k, out_scores, out_base, out_ids, idx_base, nb, max_abs_prior},
                       corpus, n_rows, queries, n_queries, dim, max_row_norm, ws, ws_bytes, path, cand_cap, stream);
}

extern "C" int32_t arx_topk_boosted_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    return masked_stats(ws, overflowed_queries, candidate_groups, stream);
}
