// arx_topk_search_prefix: exact top-k with a row limit PER QUERY over an fp16 shard (C ABI in include/arx.h).  Query q may return only
// the local rows r < row_limit[q]; with the queries pointing into the corpus and row_limit[q] = the query's own row this is the
// self-join "nearest earlier row" that near-duplicate detection needs (dedup.py).
//
// Why not filter.hip: its mask is one bitmap shared by the whole batch (a word per 64-row group, read once per wave).  Here every query of
// a tile has its own mask, but a mask of a special form — a prefix — so it needs no bitmap at all: the select in front of the group
// maximum is one integer comparison per accumulator element, and everything at or beyond the largest limit of a tile's queries is skipped.
//   masked scan   pass A as in filter.hip (fp16 MFMA, f32 accumulate; BM = 64 / 128 / 256 queries by batch size, one wave column = one
//                 64-row group); before the maximum over a group's 64 rows, the value of (query, row) is replaced by -inf unless
//                 row < row_limit[query].  A 256-row tile whose first row is at or beyond the largest limit of the block's query tile is
//                 not loaded: its group maxima are written as -inf.  For a self-join of consecutive rows that is the upper triangle.
//                 Then one block per query: t = the k-th largest group maximum, candidates = every group with gmax >= t - 2 tau that is
//                 not -inf, their rows below the limit rescored by exact_row_score (search_tail.h: the one definition of a score), top-k
//                 by (score desc, row asc).
//                 Why that is exact: k distinct groups hold a row below the limit whose pass-A score is >= t, pass A and the rescoring
//                 differ by at most tau = tau_scale |q| (rescore_kernel step 5), so the k-th exact score is >= t - tau and every row that
//                 reaches it has a pass-A score >= t - 2 tau: it sits in a candidate group.  With fewer than k non-empty groups t = -inf
//                 and every non-empty group is a candidate.  One shot, no certificate, no iteration.
//                 A query with more candidate groups than the list holds is flagged, counted and answered by the exhaustive path: a
//                 corpus with thousands of copies of one chunk puts thousands of groups within 2 tau of the top.
//   exhaustive    rows [0, row_limit[q]) cut into parts, every row scored by the same function, per-part top-k lists merged per query
//                 (filter_merge_kernel).  The rows are a prefix: no compaction.
// No float atomics.  A (query, row) score is exact_row_score's, as in arx_topk_search and arx_topk_search_filtered; both paths rank the
// same scores by the same total order, so a query's output depends on the query, its limit and the corpus alone.
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

// ---- masked pass A: filtered_groupmax_kernel's geometry with `row < lim[query]` in front of the group maximum -------------------------
template <int BM>
__global__ __launch_bounds__(512) void prefix_groupmax_kernel(const f16_t* __restrict__ Q, int nq, const f16_t* __restrict__ C, int64_t n_rows,
                                                               int D, int tiles_q, int tiles_n, const int64_t* __restrict__ lim,
                                                               const int64_t* __restrict__ tmax, float* __restrict__ gmax, int64_t ldg) {
    using ML = GemmMainloop<f16_t, BM, 256, 2, 4, true, 3>;
    static_assert(ML::TN == GROUP_ROWS, "one wave column = one group");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = xcd_remap(blockIdx.x, tiles_q * tiles_n);
    const int tile_q = t % tiles_q, tile_n = t / tiles_q;
    const int m0 = tile_q * BM;
    const int64_t n0 = (int64_t)tile_n * 256;
    const int rows_here = (int)((n_rows - n0) < 256 ? (n_rows - n0) : 256);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid / 4, wn = wid % 4;
    const int64_t g = (n0 >> 6) + wn;
    // the largest limit of this block's queries (block-uniform)
    const int n_q64 = (nq + 63) >> 6;
    int64_t top = 0;
#pragma unroll
    for (int j = 0; j < BM / 64; ++j) {
        const int b = (m0 >> 6) + j;
        const int64_t v = b < n_q64 ? tmax[b] : 0;
        top = v > top ? v : top;
    }
    float gm[ML::MI];
    if (n0 >= top) {                                           // no query of the tile may see a row of this tile: its rows are never loaded
        if (wn * GROUP_ROWS >= rows_here) return;
#pragma unroll
        for (int i = 0; i < ML::MI; ++i) gm[i] = -INFINITY;
        store_query_row<ML::MI, float>(gmax + g * ldg, gm, m0 + wm * ML::TM, nq, lane);
        return;
    }
    f32x4 acc[ML::NI][ML::MI];
    if constexpr (BM == 256) {
#ifdef ARX_STAMP
        unsigned long long dummy_stamp;
        Gemm8Phase<f16_t, 2>::run(Q, D, nq, C + n0 * D, D, rows_here, D, m0, 0, smem, acc, tile_q * 2, dummy_stamp);
#else
        Gemm8Phase<f16_t, 2>::run(Q, D, nq, C + n0 * D, D, rows_here, D, m0, 0, smem, acc, tile_q * 2);
#endif
    } else
        ML::run(Q, D, nq, C + n0 * D, D, rows_here, D, m0, 0, smem, acc, tile_q * 2);
    if (wn * GROUP_ROWS >= rows_here) return;
    // acc[j][i][r] belongs to row j*16 + (lane>>4)*4 + r of the wave's group and to query m0 + wm*TM + i*16 + (lane & 15).  The limits are
    // clamped to n_rows, so a position past the shard's end (pass A clamps its row address: a copy of the last row) is never below one.
    const int lrow = (lane >> 4) * 4;
    const int64_t g0 = g * GROUP_ROWS;
#pragma unroll
    for (int i = 0; i < ML::MI; ++i) {
        const int m = m0 + wm * ML::TM + i * 16 + (lane & 15);
        const int64_t d = (m < nq ? lim[m] : 0) - g0;
        const int rel = (int)(d < 0 ? 0 : (d > GROUP_ROWS ? GROUP_ROWS : d)) - lrow;      // rows of the group below the limit, from this lane's first
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < ML::NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, (j * 16 + r) < rel ? acc[j][i][r] : -INFINITY);      // a select: the row may hold anything finite
        gm[i] = max_over_rows(mx);
    }
    store_query_row<ML::MI, float>(gmax + g * ldg, gm, m0 + wm * ML::TM, nq, lane);
}

// the rows of group g below `lim` as a mask word (g * 64 < lim for every group the tail lists)
__device__ __forceinline__ uint64_t prefix_bits(int64_t lim, int64_t g) {
    const int64_t rem = lim - g * GROUP_ROWS;
    return rem >= GROUP_ROWS ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
}

// ---- masked scan, the tail: one block per query (filtered_tail_kernel with the prefix in place of the bitmap) ---------------------------
// Only the groups that start below the query's limit are read: the others hold -inf.
// stats: [0] queries sent to the exhaustive path, [1] candidate groups rescored, [2] (low word) "some query of this call overflowed"
__global__ __launch_bounds__(FILT_TAIL_NT) void prefix_tail_kernel(const float* __restrict__ gmax, int64_t ldg, const int64_t* __restrict__ lim,
                                                                    const f16_t* __restrict__ Q, const f16_t* __restrict__ C, int D, int k,
                                                                    float* __restrict__ out_s, int64_t* __restrict__ out_i, int64_t idx_base,
                                                                    float tau_scale, int cand_cap, int32_t* __restrict__ redo,
                                                                    unsigned long long* __restrict__ stats) {
    constexpr int NT = FILT_TAIL_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ int red[NW];
    __shared__ int n_c;
    __shared__ float sh_qn;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t limit = lim[q];
    const int64_t n_groups = (limit + GROUP_ROWS - 1) / GROUP_ROWS;                              // groups with a row below the limit
    f16_t* qs = reinterpret_cast<f16_t*>(smem);                                                  // [D] query row
    float* sc_all = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15));      // [NW][64] row scores of the group a wave is at
    int32_t* list = reinterpret_cast<int32_t*>(sc_all + NW * GROUP_ROWS);                        // [cand_cap] candidate groups
    for (int i = tid; i < (D >> 3); i += NT)
        reinterpret_cast<u32x4*>(qs)[i] = reinterpret_cast<const u32x4*>(Q + (int64_t)q * D)[i];
    if (tid == 0) n_c = 0;
    // this query's column of group maxima, as ordered keys: the first FILT_REG_GROUPS per thread stay in registers
    const float* col = gmax + q;
    uint32_t kv[FILT_REG_GROUPS];
#pragma unroll
    for (int j = 0; j < FILT_REG_GROUPS; ++j) {
        const int64_t g = (int64_t)j * NT + tid;
        kv[j] = g < n_groups ? order_key(col[g * ldg]) : 0u;
    }
    __syncthreads();
    if (w == 0) {
        float qq = 0.f;
        for (int i = lane; i < D; i += 64) { const float v = (float)qs[i]; qq = fmaf(v, v, qq); }
        qq = wave_sum(qq);
        if (lane == 0) sh_qn = sqrtf(qq);
    }
    // T = the largest key that at least k groups reach = the k-th largest group maximum, bit by bit
    uint32_t T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        int c = 0;
#pragma unroll
        for (int j = 0; j < FILT_REG_GROUPS; ++j) c += __popcll(__ballot(kv[j] >= cand));
        for (int64_t g0 = (int64_t)FILT_REG_GROUPS * NT + w * 64; g0 < n_groups; g0 += NT) {          // (wave-uniform bounds)
            const int64_t g = g0 + lane;
            c += __popcll(__ballot(g < n_groups && order_key(col[(g < n_groups ? g : 0) * ldg]) >= cand));
        }
        if (lane == 0) red[w] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) tot += red[ww];
        __syncthreads();
        T = tot >= k ? cand : T;
    }
    const float thr = key_value(T) - 2.0f * tau_scale * sh_qn;      // -inf when fewer than k groups hold a row below the limit
    // candidates: every non-empty group at or above the threshold
    auto consider = [&](int64_t g, float v) {
        if (v >= thr && v > -INFINITY) {
            const int sl = atomicAdd(&n_c, 1);
            if (sl < cand_cap) list[sl] = (int32_t)g;
        }
    };
#pragma unroll
    for (int j = 0; j < FILT_REG_GROUPS; ++j) {
        const int64_t g = (int64_t)j * NT + tid;
        if (g < n_groups) consider(g, key_value(kv[j]));
    }
    for (int64_t g = (int64_t)FILT_REG_GROUPS * NT + tid; g < n_groups; g += NT) consider(g, col[g * ldg]);
    __syncthreads();
    const int nc = n_c;
    if (nc > cand_cap) {                                       // block-uniform: never an answer from a truncated list
        if (tid == 0) {
            redo[q] = 1;
            atomicAdd(&stats[0], 1ull);
            reinterpret_cast<int*>(stats + 2)[0] = 1;
        }
        return;
    }
    if (tid == 0) { redo[q] = 0; if (nc) atomicAdd(&stats[1], (unsigned long long)nc); }
    // the rows of the candidate groups below the limit, exactly: 8 lanes per row, a group per wave at a time
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float* sc = sc_all + w * GROUP_ROWS;
    float cs = -INFINITY; int64_t ci = -1;
    for (int p = w; p < nc; p += NW) {
        const int64_t gsel = list[p];
        const uint64_t word = prefix_bits(limit, gsel);
        for (int r8 = 0; r8 < GROUP_ROWS; r8 += 8) {
            if (((word >> r8) & 0xffull) == 0ull) break;        // wave-uniform; a prefix: nothing further on either
            const int rr = r8 + rsub;
            const bool ok = (word >> rr) & 1ull;
            const float a = exact_row_score(C + (gsel * GROUP_ROWS + rr) * D, qs, nch, l8, ok);
            if (l8 == 0) sc[rr] = a;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const bool mine = (word >> lane) & 1ull;
        wave_merge64(cs, ci, mine ? sc[lane] : -INFINITY, mine ? gsel * GROUP_ROWS + lane : -1, k, lane, w_s[w], w_i[w]);
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
    }
}

// ---- exhaustive path: block (part p, query q) scores the p-th stretch of rows [0, lim[q]) -> part_s / part_i [parts][nq][k] ------------
// only_if: only the queries it flags.  gate: run only if *gate != 0 (the masked scan's "some query overflowed").
__global__ __launch_bounds__(256) void prefix_exhaustive_kernel(const int64_t* __restrict__ lim, const f16_t* __restrict__ Q,
                                                                 const f16_t* __restrict__ C, int D, int nq, int k, int64_t idx_base,
                                                                 float* __restrict__ part_s, int64_t* __restrict__ part_i,
                                                                 const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
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
    for (int i = tid; i < (D >> 3); i += 256)
        reinterpret_cast<u32x4*>(qs)[i] = reinterpret_cast<const u32x4*>(Q + (int64_t)q * D)[i];
    __syncthreads();
    const int64_t total = lim[q];
    const int64_t per = ((total + P - 1) / P + 63) / 64 * 64;
    const int64_t lo = (int64_t)p * per, hi = (lo + per < total) ? lo + per : total;
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float cs = -INFINITY; int64_t ci = -1;
    for (int64_t base = lo + (int64_t)w * 64; base < hi; base += NW * 64) {
        for (int r8 = 0; r8 < 64; r8 += 8) {
            if (base + r8 >= hi) break;                        // wave-uniform
            const int64_t row = base + r8 + rsub;
            const bool ok = row < hi;
            const float a = exact_row_score(C + (ok ? row : 0) * D, qs, nch, l8, ok);
            if (l8 == 0) sc[r8 + rsub] = a;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const bool mine = base + lane < hi;
        wave_merge64(cs, ci, mine ? sc[lane] : -INFINITY, mine ? base + lane : -1, k, lane, w_s[w], w_i[w]);
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

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct PrefWs { int64_t stats, gmax, lim, tmax, redo, part_s, part_i, total, ldg, n_groups; int parts; };
PrefWs pref_layout(int64_t n_rows, int nq, int k) {
    PrefWs w;
    const int qb = nq < QBATCH_MAX ? nq : QBATCH_MAX;
    w.ldg = round_up64(qb, 64);
    w.n_groups = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
    const int64_t want = (n_rows + 255) / 256;
    w.parts = (int)(want < FILT_PARTS_MAX ? want : FILT_PARTS_MAX);
    int64_t o = 0;
    auto take = [&](int64_t b) { int64_t r = o; o += round_up64(b, 256); return r; };
    w.stats = take(64);                                         // at the allocation's start: arx_topk_prefix_stats reads it
    w.gmax = take(w.n_groups * w.ldg * 4);
    w.lim = take(w.ldg * 8);
    w.tmax = take(w.ldg / 64 * 8);
    w.redo = take((int64_t)qb * 4);
    w.part_s = take((int64_t)w.parts * qb * k * 4);
    w.part_i = take((int64_t)w.parts * qb * k * 8);
    w.total = o;
    return w;
}

template <int BM>
int launch_prefix_groupmax(const f16_t* Q, int nq, const f16_t* C, int64_t n_rows, int D, const int64_t* lim, const int64_t* tmax, float* gmax,
                           int64_t ldg, hipStream_t st) {
    using ML = GemmMainloop<f16_t, BM, 256, 2, 4, true, 3>;
    auto kern = prefix_groupmax_kernel<BM>;
    constexpr int smem_bytes = BM == 256 ? Gemm8Phase<f16_t, 2>::STAGE_OFF : ML::SMEM_BYTES;
    ARX_HIP_CHECK(arx_func_smem((const void*)kern, smem_bytes));
    const int tq = cdiv(nq, BM);
    const int64_t tn = (n_rows + 255) / 256;
    ARX_REQUIRE(tq * tn < (1ll << 31), "grid too large");
    kern<<<(int)(tq * tn), 512, smem_bytes, st>>>(Q, nq, C, n_rows, D, tq, (int)tn, lim, tmax, gmax, ldg);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

int prefix_impl(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit, int32_t n_queries, int32_t dim, int32_t k,
                float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                int32_t cand_cap, void* stream) {
    ARX_REQUIRE(corpus && queries && row_limit && out_scores && out_ids && ws, "null pointer argument");
    ARX_REQUIRE(n_rows > 0 && n_queries > 0, "empty corpus or query set");
    ARX_REQUIRE(n_rows < (1ll << 36), "n_rows=%lld: group numbers are 32-bit", (long long)n_rows);
    ARX_REQUIRE(dim > 0 && dim % 64 == 0 && dim <= 8192, "dim=%d must be a multiple of 64", dim);
    ARX_REQUIRE(k > 0 && k <= KMAX, "k=%d out of range 1..%d", k, KMAX);
    ARX_REQUIRE(path >= 0 && path <= 2, "path=%d: 0 (library's choice), 1 (masked scan) or 2 (exhaustive)", path);
    ARX_REQUIRE(cand_cap >= 0 && cand_cap <= FILT_CAND_CAP_MAX, "cand_cap=%d out of range 0..%d", cand_cap, FILT_CAND_CAP_MAX);
    ARX_REQUIRE(max_row_norm >= 0.0f && max_row_norm < INFINITY, "max_row_norm=%g: must be a finite bound (0 = unit rows)", (double)max_row_norm);
    const PrefWs L = pref_layout(n_rows, n_queries, k);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (arx_topk_prefix_workspace_bytes)", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    if (path == 0) path = 1;      // no crossover against the exhaustive path has been measured: the masked scan with its fallback
    if (cand_cap == 0) cand_cap = FILT_CAND_CAP_DEFAULT;
    const f16_t* C = (const f16_t*)corpus;
    char* wsb = (char*)ws;
    unsigned long long* stats = (unsigned long long*)(wsb + L.stats);
    const int* gate = path == 1 ? (const int*)(stats + 2) : nullptr;      // masked scan: the exhaustive kernels run only after an overflow
    float* gmax = (float*)(wsb + L.gmax);
    int64_t* lim = (int64_t*)(wsb + L.lim);
    int64_t* tmax = (int64_t*)(wsb + L.tmax);
    int32_t* redo = (int32_t*)(wsb + L.redo);
    float* part_s = (float*)(wsb + L.part_s);
    int64_t* part_i = (int64_t*)(wsb + L.part_i);
    const float tau_scale = (0.3125f * (float)dim + 4.0f) * 5.9604645e-8f * (max_row_norm > 0.0f ? max_row_norm : 1.0f + 1.0f / 512.0f);
    ARX_HIP_CHECK(hipMemsetAsync(stats, 0, 64, st));
    const size_t smem_q = ((size_t)dim * 2 + 15) & ~(size_t)15;
    for (int q0 = 0; q0 < n_queries; q0 += QBATCH_MAX) {
        const int nq = (n_queries - q0) < QBATCH_MAX ? (n_queries - q0) : QBATCH_MAX;
        const f16_t* Q = (const f16_t*)queries + (int64_t)q0 * dim;
        float* os = out_scores + (int64_t)q0 * k;
        int64_t* oi = out_ids + (int64_t)q0 * k;
        prefix_limits_kernel<<<cdiv(nq, 64), 64, 0, st>>>(row_limit + q0, nq, n_rows, lim, tmax);
        ARX_HIP_CHECK(hipGetLastError());
        if (path == 1) {
            {
                ProfScope ps(ARX_K_SEARCH_GROUPMAX, st);
                const int rc = nq <= 64 ? launch_prefix_groupmax<64>(Q, nq, C, n_rows, dim, lim, tmax, gmax, L.ldg, st)
                             : nq <= 128 ? launch_prefix_groupmax<128>(Q, nq, C, n_rows, dim, lim, tmax, gmax, L.ldg, st)
                                         : launch_prefix_groupmax<256>(Q, nq, C, n_rows, dim, lim, tmax, gmax, L.ldg, st);
                if (rc != ARX_OK) return rc;
            }
            ProfScope ps(ARX_K_SEARCH_RESCORE, st);
            const size_t smem = smem_q + (size_t)(FILT_TAIL_NT / 64) * GROUP_ROWS * 4 + (size_t)cand_cap * 4;
            if (smem > 48 * 1024) ARX_HIP_CHECK(arx_func_smem((const void*)prefix_tail_kernel, (int)smem));
            prefix_tail_kernel<<<nq, FILT_TAIL_NT, smem, st>>>(gmax, L.ldg, lim, Q, C, dim, k, os, oi, idx_base, tau_scale, cand_cap, redo, stats);
            ARX_HIP_CHECK(hipGetLastError());
        }
        // exhaustive over the rows below the limit: every query (path 2) or the queries the tail flagged (the kernels return at once if none)
        const int32_t* only_if = path == 1 ? redo : nullptr;
        const size_t smem_x = smem_q + 4 * GROUP_ROWS * 4;
        if (smem_x > 48 * 1024) ARX_HIP_CHECK(arx_func_smem((const void*)prefix_exhaustive_kernel, (int)smem_x));
        prefix_exhaustive_kernel<<<dim3(L.parts, nq), 256, smem_x, st>>>(lim, Q, C, dim, nq, k, idx_base, part_s, part_i, only_if, gate);
        ARX_HIP_CHECK(hipGetLastError());
        filter_merge_kernel<<<cdiv(nq, 4), 256, 0, st>>>(part_s, part_i, L.parts, nq, k, os, oi, only_if, gate);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}
}      // namespace

extern "C" int64_t arx_topk_prefix_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k) {
    if (n_rows <= 0 || n_queries <= 0 || dim <= 0 || dim % 64 != 0 || k <= 0 || k > KMAX) return -1;
    return pref_layout(n_rows, n_queries, k).total;
}

extern "C" int32_t arx_topk_search_prefix(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit, int32_t n_queries,
                                          int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm,
                                          void* ws, int64_t ws_bytes, void* stream) {
    return prefix_impl(corpus, n_rows, queries, row_limit, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm, ws, ws_bytes, 0, 0,
                       stream);
}

extern "C" int32_t arx_topk_search_prefix_tuned(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit,
                                                int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids,
                                                int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                                                int32_t cand_cap, void* stream) {
    return prefix_impl(corpus, n_rows, queries, row_limit, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm, ws, ws_bytes, path,
                       cand_cap, stream);
}

extern "C" int32_t arx_topk_prefix_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    ARX_REQUIRE(ws && overflowed_queries && candidate_groups, "null pointer argument");
    unsigned long long h[2] = {0, 0};
    ARX_HIP_CHECK(hipMemcpyAsync(h, ws, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ARX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *overflowed_queries = (int64_t)h[0]; *candidate_groups = (int64_t)h[1];
    return ARX_OK;
}
