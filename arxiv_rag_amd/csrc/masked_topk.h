// The masked exact top-k search: exact top-k over the rows of an fp16 shard that a mask lets a query see.  One definition, with the kind
// of mask as a compile-time policy (filter.hip: one bitmap per call; prefix.hip: one row limit per query; filter_multi.hip: a set of
// bitmaps and one filter index per query).  Two device paths, same bits:
//   masked scan   pass A as in search.hip (fp16 MFMA, f32 accumulate; BM = 64 / 128 / 256 queries by batch size, one wave column = one
//                 64-row group) with the mask applied in the epilogue BEFORE the maximum over a group's 64 rows: a masked row's value is
//                 replaced by -inf (a select), gmax[group][query] is the maximum over the rows the query may see, -inf for a group with
//                 none; a 256-row tile of which no query of the block's tile may see a row is not loaded at all.  Then one block per
//                 query (masked_tail_kernel, with the exactness argument) rescores the rows of the candidate groups.
//   exhaustive    the query's visible rows as a list cut into parts, every row scored by the same function (exact_row_score,
//                 search_tail.h: the one definition of a score), per-part top-k lists merged per query.  Reads only visible rows.
// No float atomics; a (query, row) score depends on the row and the query alone, and both paths rank the same scores by the same total
// order (score desc, row asc), so a query's output depends on the query, its mask and the corpus alone.
//
// A mask policy `Mask` is a struct of pointers passed to the kernels by value.  On the device it supplies
//   tile<BM>(n0, wn, m0, nq, n_rows)   pass A: block-uniform `.empty` (no query of the tile sees a row of the 256-row tile at n0) and
//                                      `.lane_rows(g, lane)`, the select of this lane's 16 accumulator rows of group g; its
//                                      `.of_query(m, nq)` narrows that to query m, and the result called with (j, r) says whether
//                                      row j*16 + (lane>>4)*4 + r is kept
//   query(q, n_rows, n_groups)         the tail: `.n_groups` the query reads and `.word(g)`, its visible rows of group g as 64 bits
//   list_total(q), list_row(q, pos)    exhaustive: the length of query q's row list and the row at a position of it; kListInMemory:
//                                      list_row is a load
// and on the host
//   given(), check(n_rows)             its own arguments: non-null, in range
//   choose_path(n_queries)             what path = 0 means for a top-k search
//   own_bytes(L, n_rows, b)            its two workspace buffers (between gmax and redo), bind(ws, L) points the mask at them
//   prepare_batch / prepare_lists      kernels of its own before pass A of a batch / before the exhaustive kernel
//   kWorkspaceFn                       the name of its arx_topk_*_workspace_bytes, for the error text
//
// The host side is ONE scan driver (masked_scan) for every search that reads a row mask: these three, range.hip, grouped.hip and
// boosted.hip (whose mask also carries pass A's prior policy: PriorOf below).  It owns the protocol their exactness rests on: the common argument checks, the workspace prefix (stats at offset 0, gmax, the mask's buffers,
// redo) and its reset, gate / only_if, tau_scale, and the loop over slices of QBATCH_MAX queries with pass A, the tail and the gated
// exhaustive kernels in that order.  What differs comes from a search policy `Search`, a plain host struct passed by value like the mask
// (TopkSearch for these three): given(), check(n_rows) for its own arguments and limits; take_buffers(L) for its workspace buffers after
// redo; resolve_path(mask, path, nq) and default_cand_cap() for what path = 0 and cand_cap = 0 mean; launch_tail(slice, mask) and
// launch_exhaustive(slice, mask) for its kernels of one slice, the merge included; workspace_fn, and kSmemRaise, the dynamic LDS above
// which its launches ask for more.
// Included inside the including file's anonymous namespace after search_pass_a.h and search_tail.h; not a stand-alone header.
#pragma once

#define FILT_CAND_CAP_DEFAULT 1024      // candidate groups a query's block lists (4 KB of LDS); unit rows need about k of them
#define FILT_CAND_CAP_MAX 8192
#define FILT_PARTS_MAX 128              // per-query partial lists of the exhaustive path: parts * k <= 64 * 64 (one bit per slot and lane in the merge)
#define FILT_TAIL_NT 1024
#define FILT_REG_GROUPS 16              // group maxima a tail thread keeps in registers (16 x 1 024 groups = 1 M rows); beyond: re-read from L2

// floats ordered as unsigned integers (-inf lowest of the values pass A writes; 0 = "no such group")
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t key) {
    if (key <= 0x007fffffu) return -INFINITY;                  // -inf itself, or fewer than k groups
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// one wave: merge the scores of a group's (or a 64-entry stretch of the row list's) rows into the wave's running top-k, kept as entry
// `lane` of (cs, ci) for lanes < k.  Skipped when no new score reaches the k-th kept one (ties included: they may win on the row number).
__device__ __forceinline__ void wave_merge64(float& cs, int64_t& ci, float ns, int64_t ni, int k, int lane, float* w_s, int64_t* w_i) {
    const float kth = __shfl(cs, k - 1);
    if (!__any(ni >= 0 && ns >= kth)) return;                  // wave-uniform
    float s2[2] = {cs, ns};
    int64_t i2[2] = {ci, ni};
    wave_topk<2>(s2, i2, k, lane, w_s, w_i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    cs = lane < k ? w_s[lane] : -INFINITY;
    ci = lane < k ? w_i[lane] : -1;
}
// the block's NW per-wave lists (entries of lanes < k in w_s / w_i) -> the final k, by wave 0, into fin_s / fin_i
template <int NW>
__device__ __forceinline__ void block_merge_lists(const float (*w_s)[KMAX], const int64_t (*w_i)[KMAX], int k, int lane, float* fin_s, int64_t* fin_i) {
    constexpr int R4 = (NW * KMAX + 63) / 64;
    float s[R4]; int64_t id[R4];
#pragma unroll
    for (int j = 0; j < R4; ++j) {
        const int i = j * 64 + lane;
        s[j] = i < NW * k ? w_s[i / k][i % k] : -INFINITY;
        id[j] = i < NW * k ? w_i[i / k][i % k] : -1;
    }
    wave_topk<R4>(s, id, k, lane, fin_s, fin_i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// the block's NT threads: row q of Q -> qs in LDS (readable after the caller's next barrier)
template <int NT>
__device__ __forceinline__ void load_query_row(f16_t* qs, const f16_t* __restrict__ Q, int q, int D) {
    for (int i = threadIdx.x; i < (D >> 3); i += NT)
        reinterpret_cast<u32x4*>(qs)[i] = reinterpret_cast<const u32x4*>(Q + (int64_t)q * D)[i];
}
// one wave: the exact scores of the rows of group g that `word` names -> sc[0..64) (entries of other rows are not written): 8 lanes per row
__device__ __forceinline__ void score_word_rows(const f16_t* __restrict__ C, int64_t g, uint64_t word, const f16_t* qs, int D, int lane,
                                                float* sc) {
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    for (int r8 = 0; r8 < GROUP_ROWS; r8 += 8) {
        if (((word >> r8) & 0xffull) == 0ull) continue;          // wave-uniform
        const int rr = r8 + rsub;
        const bool ok = (word >> rr) & 1ull;
        const float a = exact_row_score(C + (g * GROUP_ROWS + rr) * D, qs, nch, l8, ok);
        if (l8 == 0) sc[rr] = a;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- the prior policy of pass A: what a mask adds to a (query, row) value in front of the group maximum.  A mask type that declares a
// member type `RowPrior` (boosted.hip) supplies `prior_rows(g, lane, n_rows)`, the lane's 16 rows' priors taken once, and its
// `.of_query(m, nq)`, whose result called with (v, j, r) gives the value that stands for row j*16 + (lane>>4)*4 + r instead of v.  Every
// other mask has NoPrior, and its pass A is the code it was before the policy existed: the branches below are compile-time.
struct NoPrior { static constexpr bool kOn = false; };
template <class Mask, class = void> struct PriorOf { using type = NoPrior; };
template <class Mask> struct PriorOf<Mask, decltype((void)sizeof(typename Mask::RowPrior))> { using type = typename Mask::RowPrior; };

// ---- masked pass A: search_groupmax_kernel with the mask in front of the group maximum ---------------------------------------------------
template <int BM, class Mask>
__global__ __launch_bounds__(512) void masked_groupmax_kernel(const f16_t* __restrict__ Q, int nq, const f16_t* __restrict__ C, int64_t n_rows,
                                                               int D, int tiles_q, int tiles_n, const Mask mask, float* __restrict__ gmax,
                                                               int64_t ldg) {
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
    const int64_t g = (n0 >> 6) + wn;
    const auto tile = mask.template tile<BM>(n0, wn, m0, nq, n_rows);
    float gm[ML::MI];
    if (tile.empty) {                                          // block-uniform: the tile's rows are never loaded
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
    // acc[j][i][r] belongs to row j*16 + (lane>>4)*4 + r of the wave's group and to query m0 + wm*TM + i*16 + (lane & 15)
    using Prior = typename PriorOf<Mask>::type;
    const auto rows = tile.lane_rows(g, lane);
    if constexpr (Prior::kOn) {
        // the same epilogue with the prior policy's value in the row's place: 16 priors per lane and one weight per accumulator column,
        // loaded here, after the k-loop, as the mixed-filter policy loads its words
        const auto priors = mask.prior_rows(g, lane, n_rows);
#pragma unroll
        for (int i = 0; i < ML::MI; ++i) {
            const int m = m0 + wm * ML::TM + i * 16 + (lane & 15);
            const auto keep = rows.of_query(m, nq);
            const auto boost = priors.of_query(m, nq);
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < ML::NI; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, keep(j, r) ? boost(acc[j][i][r], j, r) : -INFINITY);
            gm[i] = max_over_rows(mx);
        }
    } else {
#pragma unroll
    for (int i = 0; i < ML::MI; ++i) {
        const auto keep = rows.of_query(m0 + wm * ML::TM + i * 16 + (lane & 15), nq);
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < ML::NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, keep(j, r) ? acc[j][i][r] : -INFINITY);      // a select: the row may hold anything finite
        gm[i] = max_over_rows(mx);
    }
    }
    store_query_row<ML::MI, float>(gmax + g * ldg, gm, m0 + wm * ML::TM, nq, lane);
}

// ---- the candidate-group stage of a tail block: masked_tail_kernel below, range.hip's and grouped.hip's tails (FILT_TAIL_NT threads, one
// query).  A kernel copies its query row to LDS, zeroes st.n_c, calls tail_kth_key, computes ITS threshold from the key and st.qn, and
// calls tail_candidates.  The exactness of every masked scan rests on these two functions and the kernel's threshold between them.
// (masked_tail_kernel carries tail_kth_key's text inline, for the speed of the self-join: see there.)
struct TailStage { int red[FILT_TAIL_NT / 64]; int n_c; float qn; };

// kv = this thread's first FILT_REG_GROUPS group maxima of column `col` (the query's) as ordered keys, kept in registers for
// tail_candidates; st.qn = |q| of the query row qs, by wave 0; returns T = the largest key that at least ksel groups reach = the ksel-th
// largest group maximum, by a block-wide radix select, one bit per step.  Its first barrier also publishes qs and st.n_c.
__device__ __forceinline__ uint32_t tail_kth_key(TailStage& st, uint32_t (&kv)[FILT_REG_GROUPS], const float* __restrict__ col, int64_t ldg,
                                                 int64_t n_groups, const f16_t* qs, int D, int ksel) {
    constexpr int NT = FILT_TAIL_NT, NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int j = 0; j < FILT_REG_GROUPS; ++j) {
        const int64_t g = (int64_t)j * NT + tid;
        kv[j] = g < n_groups ? order_key(col[g * ldg]) : 0u;
    }
    __syncthreads();
    if (w == 0) {
        const float qn = wave_query_norm(qs, D, lane);
        if (lane == 0) st.qn = qn;
    }
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
        if (lane == 0) st.red[w] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) tot += st.red[ww];
        __syncthreads();
        T = tot >= ksel ? cand : T;
    }
    return T;
}

// candidates = every non-empty group at or above thr -> list[0 .. cand_cap), in any order (an integer LDS atomic hands out the slots).
// Returns their number (block-uniform) after recording redo[q] = 0 and stats[1]; or, when the list cannot hold them, -1 after flagging
// the query for the exhaustive path (redo[q] = 1, stats[0], the gate word): never an answer from a truncated list.
__device__ __forceinline__ int tail_candidates(TailStage& st, const uint32_t (&kv)[FILT_REG_GROUPS], const float* __restrict__ col, int64_t ldg,
                                               int64_t n_groups, float thr, int32_t* list, int cand_cap, int q, int32_t* __restrict__ redo,
                                               unsigned long long* __restrict__ stats) {
    constexpr int NT = FILT_TAIL_NT;
    const int tid = threadIdx.x;
    auto consider = [&](int64_t g, float v) {
        if (v >= thr && v > -INFINITY) {
            const int sl = atomicAdd(&st.n_c, 1);
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
    const int nc = st.n_c;
    if (nc > cand_cap) {                                       // block-uniform
        if (tid == 0) {
            redo[q] = 1;
            atomicAdd(&stats[0], 1ull);
            reinterpret_cast<int*>(stats + 2)[0] = 1;
        }
        return -1;
    }
    if (tid == 0) { redo[q] = 0; if (nc) atomicAdd(&stats[1], (unsigned long long)nc); }
    return nc;
}

// ---- masked scan, the tail: one block per query ------------------------------------------------------------------------------------------
// t = the k-th largest group maximum, candidates = every group with gmax >= t - 2 tau that is not -inf, their visible rows rescored by
// exact_row_score, top-k by (score desc, row asc).
// Why that is exact: k distinct groups hold a visible row whose pass-A score is >= t, pass A and the rescoring differ by at most
// tau = tau_scale |q| (rescore_kernel step 5), so the k-th exact score is >= t - tau and every row that reaches it has a pass-A score
// >= t - 2 tau: it sits in a candidate group.  With fewer than k non-empty groups t = -inf and every non-empty group is a candidate.
// One shot, no certificate, no iteration.  A query with more candidate groups than the list holds is flagged, counted and answered by
// the exhaustive path (a corpus with thousands of copies of one chunk puts thousands of groups within 2 tau of the top).
// stats: [0] queries sent to the exhaustive path, [1] candidate groups rescored, [2] (low word) "some query of this call overflowed"
template <class Mask>
__global__ __launch_bounds__(FILT_TAIL_NT) void masked_tail_kernel(const float* __restrict__ gmax, int64_t ldg, int64_t n_groups_all,
                                                                    const Mask mask, const f16_t* __restrict__ Q, const f16_t* __restrict__ C,
                                                                    int64_t n_rows, int D, int k, float* __restrict__ out_s,
                                                                    int64_t* __restrict__ out_i, int64_t idx_base, float tau_scale, int cand_cap,
                                                                    int32_t* __restrict__ redo, unsigned long long* __restrict__ stats) {
    constexpr int NT = FILT_TAIL_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float w_s[NW][KMAX];
    __shared__ int64_t w_i[NW][KMAX];
    __shared__ float fin_s[KMAX];
    __shared__ int64_t fin_i[KMAX];
    __shared__ TailStage st;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const auto qm = mask.query(q, n_rows, n_groups_all);
    const int64_t n_groups = qm.n_groups;                                                        // groups that may hold a visible row
    f16_t* qs = reinterpret_cast<f16_t*>(smem);                                                  // [D] query row
    float* sc_all = reinterpret_cast<float*>(smem + (((size_t)D * 2 + 15) & ~(size_t)15));      // [NW][64] row scores of the group a wave is at
    int32_t* list = reinterpret_cast<int32_t*>(sc_all + NW * GROUP_ROWS);                        // [cand_cap] candidate groups
    load_query_row<NT>(qs, Q, q, D);
    if (tid == 0) st.n_c = 0;
    // tail_kth_key(st, kv, col, ldg, n_groups, qs, D, k), written out: through the function the compiler schedules the select loop's
    // second barrier after the compare and select, and the 200 000 blocks of the prefix self-join took 1.4 % longer
    // (profiles/tail_stages_refactor.md).  Keep the two texts the same.
    const float* col = gmax + q;
    uint32_t kv[FILT_REG_GROUPS];
#pragma unroll
    for (int j = 0; j < FILT_REG_GROUPS; ++j) {
        const int64_t g = (int64_t)j * NT + tid;
        kv[j] = g < n_groups ? order_key(col[g * ldg]) : 0u;
    }
    __syncthreads();
    if (w == 0) {
        const float qn = wave_query_norm(qs, D, lane);
        if (lane == 0) st.qn = qn;
    }
    uint32_t T = 0u;                                           // -> the k-th largest group maximum
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        int c = 0;
#pragma unroll
        for (int j = 0; j < FILT_REG_GROUPS; ++j) c += __popcll(__ballot(kv[j] >= cand));
        for (int64_t g0 = (int64_t)FILT_REG_GROUPS * NT + w * 64; g0 < n_groups; g0 += NT) {          // (wave-uniform bounds)
            const int64_t g = g0 + lane;
            c += __popcll(__ballot(g < n_groups && order_key(col[(g < n_groups ? g : 0) * ldg]) >= cand));
        }
        if (lane == 0) st.red[w] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) tot += st.red[ww];
        __syncthreads();
        T = tot >= k ? cand : T;
    }
    const float thr = key_value(T) - 2.0f * tau_scale * st.qn;     // -inf when fewer than k groups hold a visible row
    const int nc = tail_candidates(st, kv, col, ldg, n_groups, thr, list, cand_cap, q, redo, stats);
    if (nc < 0) return;                                        // block-uniform: flagged for the exhaustive path
    // the visible rows of the candidate groups, exactly: a group per wave at a time
    float* sc = sc_all + w * GROUP_ROWS;
    float cs = -INFINITY; int64_t ci = -1;
    for (int p = w; p < nc; p += NW) {
        const int64_t gsel = list[p];
        const uint64_t word = qm.word(gsel);
        score_word_rows(C, gsel, word, qs, D, lane, sc);
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

// ---- exhaustive path: block (part p, query q) scores the p-th stretch of query q's row list -> part_s / part_i [parts][nq][k] (the
// layout arx_topk_merge reads).  only_if: only the queries it flags.  gate: run only if *gate != 0 (the masked scan's "some query
// overflowed").
template <class Mask>
__global__ __launch_bounds__(256) void masked_exhaustive_kernel(const Mask mask, const f16_t* __restrict__ Q, const f16_t* __restrict__ C, int D,
                                                                 int nq, int k, int64_t idx_base, float* __restrict__ part_s,
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
    const int64_t total = mask.list_total(q);
    const int64_t per = ((total + P - 1) / P + 63) / 64 * 64;
    const int64_t lo = (int64_t)p * per, hi = (lo + per < total) ? lo + per : total;
    const int nch = D >> 3, l8 = lane & 7, rsub = lane >> 3;
    float cs = -INFINITY; int64_t ci = -1;
    for (int64_t base = lo + (int64_t)w * 64; base < hi; base += NW * 64) {
        const int64_t mine = base + lane < hi ? mask.list_row(q, base + lane) : -1;
        for (int r8 = 0; r8 < 64; r8 += 8) {
            if (base + r8 >= hi) break;                        // wave-uniform
            // a list kept in memory was read once for the 64 entries and is handed round; a computed one is computed again
            const int64_t row = Mask::kListInMemory ? __shfl(mine, r8 + rsub) : (base + r8 + rsub < hi ? mask.list_row(q, base + r8 + rsub) : -1);
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

// merge_kernel (search_tail.h) for the queries `only_if` flags: one wave per query over its P lists [parts][nq][k]
__global__ __launch_bounds__(256) void filter_merge_kernel(const float* __restrict__ ps, const int64_t* __restrict__ pi, int P, int nq, int k,
                                                            float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                            const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq || (only_if && !only_if[q])) return;
    const int n = P * k;
    uint64_t taken = 0;
    for (int r = 0; r < k; ++r) {
        float bs = -INFINITY; int64_t bi = INT64_MAX; int bslot = -1;
        for (int c = lane, sl = 0; c < n; c += 64, ++sl) {
            if (taken >> sl & 1) continue;
            const int p = c / k, e = c % k;
            const int64_t o = ((int64_t)p * nq + q) * k + e;
            const float v = ps[o]; const int64_t vi = pi[o];
            if (vi < 0) continue;
            if (bslot < 0 || v > bs || (v == bs && vi < bi)) { bs = v; bi = vi; bslot = sl; }
        }
        float ws = bslot >= 0 ? bs : -INFINITY; int64_t wi = bslot >= 0 ? bi : INT64_MAX;
        wave_argbest(ws, wi);
        const bool found = wi != INT64_MAX;
        if (found && bslot >= 0 && bi == wi && bs == ws) taken |= (1ull << bslot);
        if (lane == 0) {
            out_s[(int64_t)q * k + r] = found ? ws : -INFINITY;
            out_i[(int64_t)q * k + r] = found ? wi : -1;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// The workspace of a scan: the common prefix (stats, gmax, the mask's two buffers, redo), then the search's own buffers in the order it
// takes them, each rounded up to 256 bytes.  qb = the queries of a slice, parts = the blocks per query of the exhaustive path.
struct MaskedWs {
    char* base;                                                 // the allocation; null = sizes only
    int64_t total, own[2], ldg, n_groups; int qb, parts;
    unsigned long long* stats; float* gmax; int32_t* redo;
    template <class T>
    T* take(int64_t bytes) { const int64_t o = total; total += round_up64(bytes, 256); return base ? (T*)(base + o) : nullptr; }
};
// `search.take_buffers(w)` takes the search's buffers (it may lower w.parts first).  With ws = null only the sizes mean anything.
template <class Mask, class Search>
MaskedWs scan_layout(Search& search, int64_t n_rows, int nq, char* ws) {
    MaskedWs w;
    w.base = ws; w.total = 0;
    w.qb = nq < QBATCH_MAX ? nq : QBATCH_MAX;
    w.ldg = round_up64(w.qb, 64);
    w.n_groups = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
    const int64_t want = (n_rows + 255) / 256;
    w.parts = (int)(want < FILT_PARTS_MAX ? want : FILT_PARTS_MAX);
    w.stats = w.take<unsigned long long>(64);                   // at the allocation's start: masked_stats reads it
    w.gmax = w.take<float>(w.n_groups * w.ldg * 4);
    int64_t own[2];
    Mask::own_bytes(w, n_rows, own);
    for (int i = 0; i < 2; ++i) { w.own[i] = w.total; w.take<char>(own[i]); }
    w.redo = w.take<int32_t>((int64_t)w.qb * 4);
    search.take_buffers(w);
    return w;
}

template <int BM, class Mask>
int launch_masked_groupmax(const f16_t* Q, int nq, const f16_t* C, int64_t n_rows, int D, const Mask& mask, float* gmax, int64_t ldg,
                           hipStream_t st) {
    using ML = GemmMainloop<f16_t, BM, 256, 2, 4, true, 3>;
    auto kern = masked_groupmax_kernel<BM, Mask>;
    constexpr int smem_bytes = BM == 256 ? Gemm8Phase<f16_t, 2>::STAGE_OFF : ML::SMEM_BYTES;
    ARX_HIP_CHECK(arx_func_smem((const void*)kern, smem_bytes));
    const int tq = cdiv(nq, BM);
    const int64_t tn = (n_rows + 255) / 256;
    ARX_REQUIRE(tq * tn < (1ll << 31), "grid too large");
    kern<<<(int)(tq * tn), 512, smem_bytes, st>>>(Q, nq, C, n_rows, D, tq, (int)tn, mask, gmax, ldg);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
// pass A of a batch of nq queries: the query tile by the batch's size
template <class Mask>
int launch_masked_pass_a(const f16_t* Q, int nq, const f16_t* C, int64_t n_rows, int D, const Mask& mask, float* gmax, int64_t ldg,
                         hipStream_t st) {
    ProfScope ps(ARX_K_SEARCH_GROUPMAX, st);
    return nq <= 64 ? launch_masked_groupmax<64>(Q, nq, C, n_rows, D, mask, gmax, ldg, st)
         : nq <= 128 ? launch_masked_groupmax<128>(Q, nq, C, n_rows, D, mask, gmax, ldg, st)
                     : launch_masked_groupmax<256>(Q, nq, C, n_rows, D, mask, gmax, ldg, st);
}
// tau = masked_tau_scale |q| bounds the difference between a row's pass-A score and its exact_row_score (rescore_kernel step 5);
// max_row_norm = 0: unit rows, with search.hip's default norm bound of 1 + 1/512
float masked_tau_scale(int dim, float max_row_norm) {
    return (0.3125f * (float)dim + 4.0f) * 5.9604645e-8f * (max_row_norm > 0.0f ? max_row_norm : 1.0f + 1.0f / 512.0f);
}

// what pass A's kernel takes of a mask: the mask itself, unless a mask with host-only members says otherwise (bitmap_rows.h: AllowRows)
template <class Mask>
const Mask& pass_a_mask(const Mask& mask) { return mask; }

// ---- the scan driver: see the header comment -------------------------------------------------------------------------------------------------
// What a search's launches are given: a slice of at most QBATCH_MAX queries (q0 = its first query in the call: the search advances its
// own per-query pointers by it; Q = its rows) and what the driver bound for the whole call
struct ScanSlice {
    int q0, nq; const f16_t* Q;
    const MaskedWs& L; const f16_t* C; int64_t n_rows; int dim; float tau_scale; int cand_cap;
    const int32_t* only_if; const int* gate;      // the exhaustive kernels' restriction: the scan's redo[] and overflow word; null on path 2
    size_t smem_q;                                // a query row in LDS, rounded up to 16 bytes
    hipStream_t st;
};
// `mask` and `search` arrive with the caller's arguments set; their workspace pointers are bound here.  path / cand_cap = 0: the search's
// choice.  The tail answers a query or flags it in redo[] and sets the gate word: never an answer from a truncated list.
template <class Mask, class Search>
int masked_scan(Mask mask, Search search, const void* corpus, int64_t n_rows, const void* queries, int32_t n_queries, int32_t dim,
                float max_row_norm, void* ws, int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream) {
    ARX_REQUIRE(corpus && mask.given() && queries && search.given() && ws, "null pointer argument");
    ARX_REQUIRE(n_rows > 0 && n_queries > 0, "empty corpus or query set");
    if (const int rc = search.check(n_rows); rc != ARX_OK) return rc;
    ARX_REQUIRE(n_rows < (1ll << 36), "n_rows=%lld: group numbers are 32-bit", (long long)n_rows);
    ARX_REQUIRE(dim > 0 && dim % 64 == 0 && dim <= 8192, "dim=%d must be a multiple of 64", dim);
    ARX_REQUIRE(path >= 0 && path <= 2, "path=%d: 0 (library's choice), 1 (masked scan) or 2 (exhaustive)", path);
    ARX_REQUIRE(cand_cap >= 0 && cand_cap <= FILT_CAND_CAP_MAX, "cand_cap=%d out of range 0..%d", cand_cap, FILT_CAND_CAP_MAX);
    if (const int rc = mask.check(n_rows); rc != ARX_OK) return rc;
    ARX_REQUIRE(max_row_norm >= 0.0f && max_row_norm < INFINITY, "max_row_norm=%g: must be a finite bound (0 = unit rows)", (double)max_row_norm);
    const MaskedWs L = scan_layout<Mask>(search, n_rows, n_queries, (char*)ws);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (%s)", (long long)ws_bytes, (long long)L.total, search.workspace_fn);
    hipStream_t st = (hipStream_t)stream;
    path = search.resolve_path(mask, path, n_queries);
    if (cand_cap == 0) cand_cap = search.default_cand_cap();
    mask.bind(L.base, L);
    const int* gate = path == 1 ? (const int*)(L.stats + 2) : nullptr;      // masked scan: the exhaustive kernels run only after an overflow
    ScanSlice s{0, 0, nullptr, L, (const f16_t*)corpus, n_rows, dim, masked_tau_scale(dim, max_row_norm), cand_cap,
                path == 1 ? L.redo : nullptr, gate, ((size_t)dim * 2 + 15) & ~(size_t)15, st};
    ARX_HIP_CHECK(hipMemsetAsync(L.stats, 0, 64, st));
    for (s.q0 = 0; s.q0 < n_queries; s.q0 += QBATCH_MAX) {
        s.nq = (n_queries - s.q0) < QBATCH_MAX ? (n_queries - s.q0) : QBATCH_MAX;
        s.Q = (const f16_t*)queries + (int64_t)s.q0 * dim;
        if (const int rc = mask.prepare_batch(s.q0, s.nq, n_rows, st); rc != ARX_OK) return rc;
        if (path == 1) {
            if (const int rc = launch_masked_pass_a(s.Q, s.nq, s.C, n_rows, dim, pass_a_mask(mask), L.gmax, L.ldg, st); rc != ARX_OK) return rc;
            ProfScope ps(ARX_K_SEARCH_RESCORE, st);
            if (const int rc = search.launch_tail(s, mask); rc != ARX_OK) return rc;
        }
        // exhaustive over the visible rows: every query (path 2) or the queries the tail flagged (the kernels return at once if none)
        if (const int rc = mask.prepare_lists(s.q0, path, n_rows, L.n_groups, gate, st); rc != ARX_OK) return rc;
        if (const int rc = search.launch_exhaustive(s, mask); rc != ARX_OK) return rc;
    }
    return ARX_OK;
}

// ---- the top-k search policy: masked_tail_kernel, masked_exhaustive_kernel and filter_merge_kernel ---------------------------------------
struct TopkSearch {
    int k; float* out_s; int64_t* out_i; int64_t idx_base;
    const char* workspace_fn;   // the name of the entry point's arx_topk_*_workspace_bytes, for the error text
    float* part_s; int64_t* part_i;      // workspace: the exhaustive path's per-part lists [parts][nq][k]
    static constexpr size_t kSmemRaise = 48 * 1024;      // more dynamic LDS than this is asked for before the launch

    bool given() const { return out_s && out_i; }
    int check(int64_t) const { ARX_REQUIRE(k > 0 && k <= KMAX, "k=%d out of range 1..%d", k, KMAX); return ARX_OK; }
    void take_buffers(MaskedWs& w) {
        part_s = w.take<float>((int64_t)w.parts * w.qb * k * 4);
        part_i = w.take<int64_t>((int64_t)w.parts * w.qb * k * 8);
    }
    template <class Mask>
    int resolve_path(const Mask& mask, int path, int n_queries) const { return path ? path : mask.choose_path(n_queries); }
    int default_cand_cap() const { return FILT_CAND_CAP_DEFAULT; }
    template <class Mask>
    int launch_tail(const ScanSlice& s, const Mask& mask) const {
        const size_t smem = s.smem_q + (size_t)(FILT_TAIL_NT / 64) * GROUP_ROWS * 4 + (size_t)s.cand_cap * 4;
        if (smem > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)masked_tail_kernel<Mask>, (int)smem));
        masked_tail_kernel<Mask><<<s.nq, FILT_TAIL_NT, smem, s.st>>>(s.L.gmax, s.L.ldg, s.L.n_groups, mask, s.Q, s.C, s.n_rows, s.dim, k,
                                                                     out_s + (int64_t)s.q0 * k, out_i + (int64_t)s.q0 * k, idx_base, s.tau_scale,
                                                                     s.cand_cap, s.L.redo, s.L.stats);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
    template <class Mask>
    int launch_exhaustive(const ScanSlice& s, const Mask& mask) const {
        const size_t smem_x = s.smem_q + 4 * GROUP_ROWS * 4;
        if (smem_x > kSmemRaise) ARX_HIP_CHECK(arx_func_smem((const void*)masked_exhaustive_kernel<Mask>, (int)smem_x));
        masked_exhaustive_kernel<Mask><<<dim3(s.L.parts, s.nq), 256, smem_x, s.st>>>(mask, s.Q, s.C, s.dim, s.nq, k, idx_base, part_s, part_i,
                                                                                     s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        filter_merge_kernel<<<cdiv(s.nq, 4), 256, 0, s.st>>>(part_s, part_i, s.L.parts, s.nq, k, out_s + (int64_t)s.q0 * k,
                                                             out_i + (int64_t)s.q0 * k, s.only_if, s.gate);
        ARX_HIP_CHECK(hipGetLastError());
        return ARX_OK;
    }
};
template <class Mask>
int64_t masked_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k) {
    if (n_rows <= 0 || n_queries <= 0 || dim <= 0 || dim % 64 != 0 || k <= 0 || k > KMAX) return -1;
    TopkSearch search{k};
    return scan_layout<Mask>(search, n_rows, n_queries, nullptr).total;
}
template <class Mask>
int masked_search_impl(Mask mask, const void* corpus, int64_t n_rows, const void* queries, int32_t n_queries, int32_t dim, int32_t k,
                       float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path,
                       int32_t cand_cap, void* stream) {
    return masked_scan(mask, TopkSearch{k, out_scores, out_ids, idx_base, Mask::kWorkspaceFn}, corpus, n_rows, queries, n_queries, dim,
                       max_row_norm, ws, ws_bytes, path, cand_cap, stream);
}

// the counters of the last search that used workspace `ws`
int masked_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream) {
    ARX_REQUIRE(ws && overflowed_queries && candidate_groups, "null pointer argument");
    unsigned long long h[2] = {0, 0};
    ARX_HIP_CHECK(hipMemcpyAsync(h, ws, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ARX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    *overflowed_queries = (int64_t)h[0]; *candidate_groups = (int64_t)h[1];
    return ARX_OK;
}
