// arx_topk_search_filtered: exact top-k over the ALLOWED rows of an fp16 shard (C ABI in include/arx.h; Chroma's `where`).
//
// The filter is a bitmap, one 64-bit word per 64-row group (bit r & 63 of word r >> 6 = row r may be returned; bits at or beyond n_rows
// are ignored).  Two device paths, same bits:
//   masked scan   pass A as in search.hip (fp16 MFMA, f32 accumulate) with the filter applied in the epilogue BEFORE the maximum over a
//                 group's 64 rows: a disallowed row's value is replaced by -inf (a select), gmax[group][query] is the maximum over the
//                 allowed rows, -inf for a group with none; a 256-row tile whose four words are zero is not loaded at all.  Then one block
//                 per query: t = the k-th largest group maximum, candidates = every group with gmax >= t - 2 tau, their allowed rows
//                 rescored by exact_row_score (search_tail.h: the one definition of a score), top-k by (score desc, row asc).
//                 Why that is exact: k distinct groups hold an allowed row whose pass-A score is >= t, pass A and pass B differ by at most
//                 tau = tau_scale |q| (rescore_kernel step 5), so the k-th exact score is >= t - tau and every row that reaches it has a
//                 pass-A score >= t - 2 tau: it sits in a candidate group.  One shot, no certificate, no iteration.
//                 A query with more candidate groups than the list holds is answered by the exhaustive path and counted.
//   exhaustive    the bitmap compacted to the list of allowed rows (popcount + scan, scatter), every (query, allowed row) scored by the
//                 same function, per-block top-k lists merged per query.  Reads only the allowed rows.
// No float atomics; a row's score depends on the row and the query alone.
#include <math.h>

#include "arx_common.h"
#include "gemm.h"
#include "gemm8.h"
#include "search_consts.h"

namespace {      // the two headers also define non-template kernels: internal linkage keeps this object's copies apart from search.hip's
#include "search_pass_a.h"
#include "search_tail.h"
#include "masked_topk.h"      // shared with prefix.hip: list sizes, ordered keys, the tails' merges, filter_merge_kernel

// path = 0 with n_allowed known: the exhaustive path below this many (allowed row, query) pairs.  Measured (profiles/filter_bench.json:
// 1 M x 768 unit rows, k = 10, ms per batch, exhaustive against masked scan): 64 queries — 0.239 / 0.321 at 0.67 M pairs, 0.287 / 0.334 at
// 1.05 M, 1.146 / 0.347 at 6.7 M; 1 query (the exhaustive grid is then 128 blocks) — 0.176 / 0.347 at 0.10 M, 0.173 / 0.184 at 0.13 M,
// 0.424 / 0.353 at 0.52 M.  Hence 2^20 pairs from 64 queries on, 2^18 below.
#define FILT_EXHAUSTIVE_MAX_PAIRS_WIDE (1ll << 20)
#define FILT_EXHAUSTIVE_MAX_PAIRS (1ll << 18)
#define FILT_WIDE_NQ 64

__device__ __forceinline__ uint64_t valid_bits(int64_t n_rows, int64_t g) {      // the bits of word g that name rows of the shard
    const int64_t rem = n_rows - g * GROUP_ROWS;
    return rem >= GROUP_ROWS ? ~0ull : ((1ull << rem) - 1ull);
}

// ---- masked pass A: search_groupmax_kernel with the filter in front of the group maximum ------------------------------------------------
template <int BM>
__global__ __launch_bounds__(512) void filtered_groupmax_kernel(const f16_t* __restrict__ Q, int nq, const f16_t* __restrict__ C, int64_t n_rows,
                                                                 int D, int tiles_q, int tiles_n, const uint64_t* __restrict__ allow,
                                                                 float* __restrict__ gmax, int64_t ldg) {
    using ML = GemmMainloop<f16_t, BM, 256, 2, 4, true, 3>;
    static_assert(ML::TN == GROUP_ROWS, "one wave column = one group = one mask word");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = xcd_remap(blockIdx.x, tiles_q * tiles_n);
    const int tile_q = t % tiles_q, tile_n = t / tiles_q;
    const int m0 = tile_q * BM;
    const int64_t n0 = (int64_t)tile_n * 256;
    const int rows_here = (int)((n_rows - n0) < 256 ? (n_rows - n0) : 256);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid / 4, wn = wid % 4;
    const int64_t n_groups = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
    const int64_t g = (n0 >> 6) + wn;
    // the tile's four words (block-uniform) and this wave's own
    uint64_t any = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t gj = (n0 >> 6) + j;
        const uint64_t w = gj < n_groups ? (allow[gj] & valid_bits(n_rows, gj)) : 0ull;
        any |= w;
        mine = j == wn ? w : mine;
    }
    float gm[ML::MI];
    if (any == 0ull) {                                         // nothing allowed in this tile: its rows are never loaded
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
    // acc[j][i][r] belongs to row j*16 + (lane>>4)*4 + r of the wave's group
    const uint32_t lrow = (uint32_t)(lane >> 4) * 4u;
    bool on[ML::NI][4];
#pragma unroll
    for (int j = 0; j < ML::NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) on[j][r] = (mine >> ((uint32_t)(j * 16 + r) + lrow)) & 1ull;
#pragma unroll
    for (int i = 0; i < ML::MI; ++i) {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < ML::NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, on[j][r] ? acc[j][i][r] : -INFINITY);      // a select: the row may hold anything finite
        gm[i] = max_over_rows(mx);
    }
    store_query_row<ML::MI, float>(gmax + g * ldg, gm, m0 + wm * ML::TM, nq, lane);
}

// ---- masked scan, the tail: one block per query ------------------------------------------------------------------------------------------
// stats: [0] queries sent to the exhaustive path, [1] candidate groups rescored, [2] (low word) "some query of this batch overflowed"
__global__ __launch_bounds__(FILT_TAIL_NT) void filtered_tail_kernel(const float* __restrict__ gmax, int64_t ldg, int64_t n_groups,
                                                                      const uint64_t* __restrict__ allow, const f16_t* __restrict__ Q,
                                                                      const f16_t* __restrict__ C, int64_t n_rows, int D, int k,
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
    const float thr = key_value(T) - 2.0f * tau_scale * sh_qn;      // -inf when fewer than k groups hold an allowed row
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
    // the allowed rows of the candidate groups, exactly: 8 lanes per row, a group per wave at a time
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float* sc = sc_all + w * GROUP_ROWS;
    float cs = -INFINITY; int64_t ci = -1;
    for (int p = w; p < nc; p += NW) {
        const int64_t gsel = list[p];
        const uint64_t word = allow[gsel] & valid_bits(n_rows, gsel);
        for (int r8 = 0; r8 < GROUP_ROWS; r8 += 8) {
            if (((word >> r8) & 0xffull) == 0ull) continue;      // wave-uniform
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

// ---- exhaustive path ---------------------------------------------------------------------------------------------------------------------
// offsets of the words' rows in the compacted list (exclusive scan of the popcounts; off[n_words] = the number of allowed rows).  One
// block: thread t owns a contiguous run of words.  `gate`: run only if *gate != 0 (the masked scan's "some query overflowed").
__global__ __launch_bounds__(1024) void filter_scan_kernel(const uint64_t* __restrict__ allow, int64_t n_words, int64_t n_rows,
                                                            int64_t* __restrict__ off, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ int64_t wave_tot[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t per = (n_words + 1023) / 1024;
    const int64_t a = (int64_t)tid * per, b = (a + per < n_words) ? a + per : n_words;
    int64_t mine = 0;
    for (int64_t i = a; i < b; ++i) mine += __popcll(allow[i] & valid_bits(n_rows, i));
    int64_t inc = mine;                                        // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t up = __shfl_up(inc, o);
        inc += lane >= o ? up : 0;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    int64_t base = 0;
    for (int ww = 0; ww < w; ++ww) base += wave_tot[ww];
    int64_t run = base + inc - mine;
    for (int64_t i = a; i < b; ++i) {
        off[i] = run;
        run += __popcll(allow[i] & valid_bits(n_rows, i));
    }
    if (tid == 1023) off[n_words] = base + inc;
}
// one lane per row: the allowed rows in ascending order
__global__ __launch_bounds__(256) void filter_scatter_kernel(const uint64_t* __restrict__ allow, int64_t n_words, int64_t n_rows,
                                                              const int64_t* __restrict__ off, int64_t* __restrict__ rows,
                                                              const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int lane = threadIdx.x & 63;
    const int64_t wd = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wd >= n_words) return;
    const uint64_t word = allow[wd] & valid_bits(n_rows, wd);
    if ((word >> lane) & 1ull) rows[off[wd] + __popcll(word & ((1ull << lane) - 1ull))] = wd * GROUP_ROWS + lane;
}

// block (part p, query q): the p-th stretch of the row list against query q, top-k -> part_s / part_i [parts][nq][k] (the layout
// arx_topk_merge reads).  only_if: only the queries it flags.
__global__ __launch_bounds__(256) void filter_exhaustive_kernel(const int64_t* __restrict__ rows, const int64_t* __restrict__ n_list,
                                                                 const f16_t* __restrict__ Q, const f16_t* __restrict__ C, int D, int nq, int k,
                                                                 int64_t idx_base, float* __restrict__ part_s, int64_t* __restrict__ part_i,
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
    const int64_t total = *n_list;
    const int64_t per = ((total + P - 1) / P + 63) / 64 * 64;
    const int64_t lo = (int64_t)p * per, hi = (lo + per < total) ? lo + per : total;
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float cs = -INFINITY; int64_t ci = -1;
    for (int64_t base = lo + (int64_t)w * 64; base < hi; base += NW * 64) {
        const int64_t mine = base + lane < hi ? rows[base + lane] : -1;
        for (int r8 = 0; r8 < 64; r8 += 8) {
            if (base + r8 >= hi) break;                        // wave-uniform
            const int64_t row = __shfl(mine, r8 + rsub);
            const bool ok = row >= 0;
            const float a = exact_row_score(C + (ok ? row : 0) * D, qs, nch, l8, ok);
            if (l8 == 0) sc[r8 + rsub] = a;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wave_merge64(cs, ci, mine >= 0 ? sc[lane] : -INFINITY, mine, k, lane, w_s[w], w_i[w]);
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

// (the merge of the per-part lists, filter_merge_kernel: masked_topk.h)

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct FiltWs { int64_t stats, gmax, off, rows, redo, part_s, part_i, total, ldg, n_groups; int parts; };
FiltWs filt_layout(int64_t n_rows, int nq, int k) {
    FiltWs w;
    const int qb = nq < QBATCH_MAX ? nq : QBATCH_MAX;
    w.ldg = round_up64(qb, 64);
    w.n_groups = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
    const int64_t want = (n_rows + 255) / 256;
    w.parts = (int)(want < FILT_PARTS_MAX ? want : FILT_PARTS_MAX);
    int64_t o = 0;
    auto take = [&](int64_t b) { int64_t r = o; o += round_up64(b, 256); return r; };
    w.stats = take(64);                                         // at the allocation's start: arx_topk_filtered_stats reads it
    w.gmax = take(w.n_groups * w.ldg * 4);
    w.off = take((w.n_groups + 1) * 8);
    w.rows = take(n_rows * 8);
    w.redo = take((int64_t)qb * 4);
    w.part_s = take((int64_t)w.parts * qb * k * 4);
    w.part_i = take((int64_t)w.parts * qb * k * 8);
    w.total = o;
    return w;
}

template <int BM>
int launch_filtered_groupmax(const f16_t* Q, int nq, const f16_t* C, int64_t n_rows, int D, const uint64_t* allow, float* gmax, int64_t ldg,
                             hipStream_t st) {
    using ML = GemmMainloop<f16_t, BM, 256, 2, 4, true, 3>;
    auto kern = filtered_groupmax_kernel<BM>;
    constexpr int smem_bytes = BM == 256 ? Gemm8Phase<f16_t, 2>::STAGE_OFF : ML::SMEM_BYTES;
    ARX_HIP_CHECK(arx_func_smem((const void*)kern, smem_bytes));
    const int tq = cdiv(nq, BM);
    const int64_t tn = (n_rows + 255) / 256;
    ARX_REQUIRE(tq * tn < (1ll << 31), "grid too large");
    kern<<<(int)(tq * tn), 512, smem_bytes, st>>>(Q, nq, C, n_rows, D, tq, (int)tn, allow, gmax, ldg);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

int filtered_impl(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries, int32_t n_queries,
                  int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm, void* ws,
                  int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream) {
    ARX_REQUIRE(corpus && allow && queries && out_scores && out_ids && ws, "null pointer argument");
    ARX_REQUIRE(n_rows > 0 && n_queries > 0, "empty corpus or query set");
    ARX_REQUIRE(n_rows < (1ll << 36), "n_rows=%lld: group numbers are 32-bit", (long long)n_rows);
    ARX_REQUIRE(dim > 0 && dim % 64 == 0 && dim <= 8192, "dim=%d must be a multiple of 64", dim);
    ARX_REQUIRE(k > 0 && k <= KMAX, "k=%d out of range 1..%d", k, KMAX);
    ARX_REQUIRE(path >= 0 && path <= 2, "path=%d: 0 (library's choice), 1 (masked scan) or 2 (exhaustive)", path);
    ARX_REQUIRE(cand_cap >= 0 && cand_cap <= FILT_CAND_CAP_MAX, "cand_cap=%d out of range 0..%d", cand_cap, FILT_CAND_CAP_MAX);
    ARX_REQUIRE(n_allowed >= -1 && n_allowed <= n_rows, "n_allowed=%lld", (long long)n_allowed);
    ARX_REQUIRE(max_row_norm >= 0.0f && max_row_norm < INFINITY, "max_row_norm=%g: must be a finite bound (0 = unit rows)", (double)max_row_norm);
    const FiltWs L = filt_layout(n_rows, n_queries, k);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (arx_topk_filtered_workspace_bytes)", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    if (path == 0)
        path = (n_allowed >= 0 && n_allowed * (int64_t)n_queries < (n_queries >= FILT_WIDE_NQ ? FILT_EXHAUSTIVE_MAX_PAIRS_WIDE : FILT_EXHAUSTIVE_MAX_PAIRS))
                   ? 2 : 1;
    if (cand_cap == 0) cand_cap = FILT_CAND_CAP_DEFAULT;
    const f16_t* C = (const f16_t*)corpus;
    char* wsb = (char*)ws;
    unsigned long long* stats = (unsigned long long*)(wsb + L.stats);
    const int* gate = path == 1 ? (const int*)(stats + 2) : nullptr;      // masked scan: the exhaustive kernels run only after an overflow
    float* gmax = (float*)(wsb + L.gmax);
    int64_t* off = (int64_t*)(wsb + L.off);
    int64_t* rows = (int64_t*)(wsb + L.rows);
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
        if (path == 1) {
            {
                ProfScope ps(ARX_K_SEARCH_GROUPMAX, st);
                const int rc = nq <= 64 ? launch_filtered_groupmax<64>(Q, nq, C, n_rows, dim, allow, gmax, L.ldg, st)
                             : nq <= 128 ? launch_filtered_groupmax<128>(Q, nq, C, n_rows, dim, allow, gmax, L.ldg, st)
                                         : launch_filtered_groupmax<256>(Q, nq, C, n_rows, dim, allow, gmax, L.ldg, st);
                if (rc != ARX_OK) return rc;
            }
            ProfScope ps(ARX_K_SEARCH_RESCORE, st);
            const size_t smem = smem_q + (size_t)(FILT_TAIL_NT / 64) * GROUP_ROWS * 4 + (size_t)cand_cap * 4;
            if (smem > 48 * 1024) ARX_HIP_CHECK(arx_func_smem((const void*)filtered_tail_kernel, (int)smem));
            filtered_tail_kernel<<<nq, FILT_TAIL_NT, smem, st>>>(gmax, L.ldg, L.n_groups, allow, Q, C, n_rows, dim, k, os, oi, idx_base, tau_scale,
                                                                 cand_cap, redo, stats);
            ARX_HIP_CHECK(hipGetLastError());
        }
        // exhaustive over the allowed rows: every query (path 2) or the queries the tail flagged (the kernels return at once if none)
        if (q0 == 0 || path == 1) {                            // (the list does not depend on the batch; after an overflow it is built then)
            filter_scan_kernel<<<1, 1024, 0, st>>>(allow, L.n_groups, n_rows, off, gate);
            ARX_HIP_CHECK(hipGetLastError());
            filter_scatter_kernel<<<cdiv(L.n_groups, 4), 256, 0, st>>>(allow, L.n_groups, n_rows, off, rows, gate);
            ARX_HIP_CHECK(hipGetLastError());
        }
        const int32_t* only_if = path == 1 ? redo : nullptr;
        const size_t smem_x = smem_q + 4 * GROUP_ROWS * 4;
        if (smem_x > 48 * 1024) ARX_HIP_CHECK(arx_func_smem((const void*)filter_exhaustive_kernel, (int)smem_x));
        filter_exhaustive_kernel<<<dim3(L.parts, nq), 256, smem_x, st>>>(rows, off + L.n_groups, Q, C, dim, nq, k, idx_base, part_s, part_i, only_if, gate);
        ARX_HIP_CHECK(hipGetLastError());
        filter_merge_kernel<<<cdiv(nq, 4), 256, 0, st>>>(part_s, part_i, L.parts, nq, k, os, oi, only_if, gate);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}
}      // namespace

extern "C" int64_t arx_topk_filtered_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k) {
    if (n_rows <= 0 || n_queries <= 0 || dim <= 0 || dim % 64 != 0 || k <= 0 || k > KMAX) return -1;
    return filt_layout(n_rows, n_queries, k).total;
}

extern "C" int32_t arx_topk_search_filtered(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                            int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                                            float max_row_norm, void* ws, int64_t ws_bytes, void* stream) {
    return filtered_impl(corpus, n_rows, allow, n_allowed, queries, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm, ws, ws_bytes,
                         0, 0, stream);
}

extern "C" int32_t arx_topk_search_filtered_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                                  int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids,
                                                  int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                                                  int32_t cand_cap, void* stream) {
    return filtered_impl(corpus, n_rows, allow, n_allowed, queries, n_queries, dim, k, out_scores, out_ids, idx_base, max_row_norm, ws, ws_bytes,
                         path, cand_cap, stream);
}

extern "C" int32_t arx_topk_filtered_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    ARX_REQUIRE(ws && overflowed_queries && candidate_groups, "null pointer argument");
    unsigned long long h[2] = {0, 0};
    ARX_HIP_CHECK(hipMemcpyAsync(h, ws, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ARX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *overflowed_queries = (int64_t)h[0]; *candidate_groups = (int64_t)h[1];
    return ARX_OK;
}
