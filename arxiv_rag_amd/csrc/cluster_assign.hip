// arx_cluster_assign: the assign half of a spherical k-means (Lloyd) iteration, and "label rows against given centroids" (gfx950; C ABI in
// include/arx.h; the host layer is arxiv_rag_amd/topics.py; the definitions are INTEGRATION.md "Topics").
//
//   label[i] = the lowest c that maximises exact_row_score(centroid c, row i)        score[i] = that f32 value
// exact_row_score (exact_score.h) is the score of arx_topk_search, so for finite inputs the answer is that search's k = 1 answer over the
// centroids, bit for bit.  The search is built for few queries over many rows; here there are many rows and at most 4096 centroids.
//
// Fast pass (assign_fast_kernel).  A block of four waves owns R = 32 or 64 rows (`rows_per_block`) and walks every centroid.  Scores come
// from __builtin_amdgcn_mfma_f32_32x32x16_f16 with the CENTROIDS as the A operand and the rows as B: lane l then holds, for row l & 31,
// the scores of the 16 centroids 8 (e >> 2) + 4 (l >> 5) + (e & 3) of a 32-centroid tile, so the reduction over the centroid axis is
// in-lane.  A lane keeps (best score, its centroid, second-best score) across all its tiles; its tiles come in ascending order, so a
// strict '>' keeps the lower centroid on ties.  At the end the 8 lists of a row (4 waves x 2 lane halves) are merged through LDS by
// (score desc, centroid asc).
//   operands   The row tile is staged in LDS (row stride dim + 8 halves: the 16-byte fragment reads of 16 rows then cover all 64 banks).
//              A lane reads 64 contiguous bytes of "its" centroid per 64-deep k block straight from global memory (L2 / MALL: the
//              centroids are at most a few MB and every block reads all of them), the two lane halves together one 128-byte line; the k
//              order inside a block is permuted the same way for both operands, which a dot product does not see.
//   residency  Wave w takes tiles t0 + w, t0 + 4 + w, ... of a GROUP of 4 G tiles (G = 4 at R = 32, 2 at R = 64) and holds their
//              accumulators.  Where R x dim <= 49152 halves (dim <= 1536 at R = 32) the row tile is staged ONCE and X is read from HBM
//              once.  Otherwise it is staged in chunks of 32768 / R columns, once per group: X is then read ceil(C / (128 G)) times
//              (8 times at C = 4096, R = 32), all but the first from L2.
//   padding    A tile's centroids past C read centroid C - 1 and enter the reduction as -inf; rows past n_rows read row n_rows - 1 and
//              are never stored.
// Certificate.  a(c) is the MFMA score, e(c) exact_row_score.  Both are f32 sums of the D exact products x_k c_k (fp16 x fp16 is exact in
// f32), in different orders:
//   |e - x.c| <= B(D) u |x| |c|,  B(D) = D / 16 + 4   (the search's pass-B budget: two chains of D / 16 adds, the chain sum, the butterfly)
//   |a - x.c| <= A(D) u |x| |c|,  A(D) = D            (ANY order of D - 1 rounded adds: (D - 1) u sum |x_k c_k| to first order, and
//                                                      sum |x_k c_k| <= |x| |c|.  The search allows its own MFMA chain 8 roundings per
//                                                      32-deep step, 0.25 D; this file assumes nothing about the order inside the
//                                                      instruction and allows 32.)
// with u = 2^-24.  tau_i = tau_mult (1.0625 D + 4) u |x_i| max_centroid_norm; |x_i| is summed in f32 from the staged row and multiplied
// by 1 + 2^-10 (its own roundings, D u / 2 relative, and the second-order terms above).  If a_best - a_second > 2 tau_i then e(best) >
// e(c) for every other c: the best centroid is the unique exact winner and one exact_row_score gives the score.  The test is written
// !(a_best - a_second > 2 tau_i): a NaN or infinite row is flagged.  With C = 1 the second best is -inf and nothing is flagged, whatever
// tau_mult.
// Slow path (assign_slow_kernel).  A flagged row goes on a list behind an integer counter; the second launch reads the count on the
// device (no host read) and gives each listed row to a block: 8 lanes per centroid score every centroid with exact_row_score, strict '>'
// in ascending order per octet, then (score desc, centroid asc) over the 32 octets.  When two centroids are identical every row is
// flagged and the call costs n C D FMAs, which is what the search pays.
// Every out_labels / out_scores element is written once by a plain store (fast pass: certified rows; slow path: flagged rows).  The only
// atomic is the integer add on the list counter; stats are plain stores of one thread (count, count * C).  The list's order depends on
// arrival, the results do not.
#include <math.h>

#include "arx_common.h"
#include "exact_score.h"

namespace {

constexpr int CA_NT = 256, CA_NW = CA_NT / 64;
constexpr int CA_DIM_MAX = 8192, CA_C_MAX = 4096;
constexpr int CA_PAD = 8;                                     // halves a staged row is padded by
constexpr int CA_WHOLE_HALVES = 32 * 1536;                    // a row tile of at most this many halves is staged whole
constexpr int CA_CHUNK_HALVES = 32 * 1024;                    // ... a larger one in chunks of this many
constexpr int CA_SLOW_BLOCKS = 2048;
constexpr int CA_NONE = 0x7fffffff;

template <int RT, int G>
__global__ __launch_bounds__(CA_NT) void assign_fast_kernel(const f16_t* __restrict__ X, int n, int D, const f16_t* __restrict__ Cn, int C, int KC,
                                                            float tau2, int32_t* __restrict__ out_labels, float* __restrict__ out_scores,
                                                            int32_t* __restrict__ flagged, int* __restrict__ counter) {
    constexpr int R = 32 * RT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f16_t* xs = reinterpret_cast<f16_t*>(smem);               // [R][KC + CA_PAD]
    __shared__ float nsq[R];
    __shared__ float m_b[2 * CA_NW][R], m_s[2 * CA_NW][R];
    __shared__ int m_i[2 * CA_NW][R];
    __shared__ int lab[R];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, slot = lane & 31, h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int ld = KC + CA_PAD;
    const int ntiles = (C + 31) >> 5, nchunks = (D + KC - 1) / KC;
    if (tid < R) nsq[tid] = 0.f;
    float bb[RT], bs[RT]; int bi[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { bb[rt] = -INFINITY; bs[rt] = -INFINITY; bi[rt] = CA_NONE; }
    for (int t0 = 0; t0 < ntiles; t0 += CA_NW * G) {
        f32x16 acc[G][RT];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[g][rt][e] = 0.f;
        for (int kc = 0; kc < nchunks; ++kc) {
            const int k0 = kc * KC, kn = D - k0 < KC ? D - k0 : KC, kch = kn >> 3;
            if (nchunks > 1 || t0 == 0) {                     // (block-uniform) a tile staged whole is staged once
                __syncthreads();
                for (int i = tid; i < R * kch; i += CA_NT) {
                    const int r = i / kch, c = i - r * kch;
                    const int64_t gr = row0 + r < n ? row0 + r : (int64_t)n - 1;
                    *reinterpret_cast<u32x4*>(xs + r * ld + c * 8) = *reinterpret_cast<const u32x4*>(X + gr * D + k0 + c * 8);
                }
                __syncthreads();
                if (t0 == 0) {                                // |x|^2, 8 lanes per row; one thread owns a row's sum
                    for (int r = tid >> 3; r < R; r += CA_NT / 8) {
                        float q = 0.f;
                        for (int c = tid & 7; c < kch; c += 8) {
                            const f16x8 v = *reinterpret_cast<const f16x8*>(xs + r * ld + c * 8);
#pragma unroll
                            for (int e = 0; e < 8; ++e) q = fmaf((float)v[e], (float)v[e], q);
                        }
                        q += __shfl_xor(q, 4); q += __shfl_xor(q, 2); q += __shfl_xor(q, 1);
                        if ((tid & 7) == 0) nsq[r] += q;
                    }
                }
            }
            for (int kb = 0; kb < kn; kb += 64) {
                f16x8 bf[RT][4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) bf[rt][j] = *reinterpret_cast<const f16x8*>(xs + (rt * 32 + slot) * ld + kb + 32 * h + 8 * j);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int tile = t0 + g * CA_NW + w;      // (wave-uniform)
                    if (tile < ntiles) {
                        const int c = tile * 32 + slot < C ? tile * 32 + slot : C - 1;
                        const f16_t* ap = Cn + (int64_t)c * D + k0 + kb + 32 * h;
                        f16x8 af[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) af[j] = *reinterpret_cast<const f16x8*>(ap + 8 * j);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) acc[g][rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[j], bf[rt][j], acc[g][rt], 0, 0, 0);
                    }
                }
            }
        }
        // the group's scores into the lane's running (best, centroid, second best): ascending centroids, so '>' keeps the lower one
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int tile = t0 + g * CA_NW + w;
            if (tile < ntiles) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int c = tile * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
                        const float v = c < C ? acc[g][rt][e] : -INFINITY;
                        const bool take = v > bb[rt];
                        bs[rt] = take ? bb[rt] : fmaxf(bs[rt], v);
                        bi[rt] = take ? c : bi[rt];
                        bb[rt] = take ? v : bb[rt];
                    }
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { m_b[2 * w + h][rt * 32 + slot] = bb[rt]; m_s[2 * w + h][rt * 32 + slot] = bs[rt]; m_i[2 * w + h][rt * 32 + slot] = bi[rt]; }
    __syncthreads();
    if (tid < R) {
        float b = m_b[0][tid], s = m_s[0][tid]; int i = m_i[0][tid];
#pragma unroll
        for (int p = 1; p < 2 * CA_NW; ++p) {
            const float ob = m_b[p][tid], os = m_s[p][tid]; const int oi = m_i[p][tid];
            const bool take = ob > b || (ob == b && oi < i);
            s = fmaxf(fmaxf(s, os), take ? b : ob);
            i = take ? oi : i;
            b = take ? ob : b;
        }
        const float tau2_i = tau2 * (sqrtf(nsq[tid]) * (1.0f + 0.0009765625f));
        const bool flag = !(b - s > tau2_i) || i < 0 || i >= C;
        lab[tid] = flag ? -1 : i;
        if (flag && row0 + tid < n) flagged[atomicAdd(counter, 1)] = (int32_t)(row0 + tid);
    }
    __syncthreads();
    // certified rows: the winner's exact score, 8 lanes per row
    for (int r = tid >> 3; r < R; r += CA_NT / 8) {
        const int c = lab[r];
        const bool ok = row0 + r < n && c >= 0;
        const float a = exact_row_score(Cn + (int64_t)(ok ? c : 0) * D, X + (ok ? row0 + r : 0) * D, D >> 3, tid & 7, ok);
        if (ok && (tid & 7) == 0) { out_labels[row0 + r] = c; out_scores[row0 + r] = a; }
    }
}

__global__ __launch_bounds__(CA_NT) void assign_slow_kernel(const f16_t* __restrict__ X, int n, int D, const f16_t* __restrict__ Cn, int C,
                                                            const int32_t* __restrict__ flagged, const int* __restrict__ counter,
                                                            int32_t* __restrict__ out_labels, float* __restrict__ out_scores,
                                                            int64_t* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f16_t* qs = reinterpret_cast<f16_t*>(smem);               // [D] the flagged row
    __shared__ float o_s[CA_NT / 8];
    __shared__ int o_i[CA_NT / 8];
    const int tid = threadIdx.x, o = tid >> 3, l8 = tid & 7, nch = D >> 3;
    int count = *counter;
    count = count < 0 ? 0 : (count > n ? n : count);
    if (stats && blockIdx.x == 0 && tid == 0) { stats[0] = count; stats[1] = (int64_t)count * C; }
    for (int f = blockIdx.x; f < count; f += gridDim.x) {
        const int row = flagged[f];
        if (row < 0 || row >= n) continue;                    // (block-uniform; the fast pass lists rows of the shard only)
        __syncthreads();
        for (int i = tid; i < nch; i += CA_NT) reinterpret_cast<u32x4*>(qs)[i] = reinterpret_cast<const u32x4*>(X + (int64_t)row * D)[i];
        __syncthreads();
        float b = -INFINITY; int bi = CA_NONE;
        for (int c0 = 0; c0 < C; c0 += CA_NT / 8) {
            const int c = c0 + o;
            const bool ok = c < C;
            const float a = exact_row_score(Cn + (int64_t)(ok ? c : 0) * D, qs, nch, l8, ok);
            if (ok && (bi == CA_NONE || a > b)) { b = a; bi = c; }
        }
        if (l8 == 0) { o_s[o] = b; o_i[o] = bi; }
        __syncthreads();
        if (tid == 0) {
            float s = o_s[0]; int i = o_i[0];                 // octet 0 always holds centroid 0
            for (int p = 1; p < CA_NT / 8; ++p) {
                const float ps = o_s[p]; const int pi = o_i[p];
                if (pi != CA_NONE && (ps > s || (ps == s && pi < i))) { s = ps; i = pi; }
            }
            out_labels[row] = i;
            out_scores[row] = s;
        }
    }
}

int cluster_assign_impl(const void* rows, int64_t n_rows, int32_t dim, const void* centroids, int32_t C, float max_centroid_norm,
                        int32_t* out_labels, float* out_scores, int64_t* stats, void* ws, int64_t ws_bytes, float tau_mult,
                        int32_t rows_per_block, void* stream) {
    ARX_REQUIRE(dim >= 64 && dim <= CA_DIM_MAX && dim % 64 == 0, "dim=%d must be a multiple of 64 in [64, %d]", dim, CA_DIM_MAX);
    ARX_REQUIRE(C >= 1 && C <= CA_C_MAX, "C=%d must be in [1, %d]", C, CA_C_MAX);
    ARX_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows=%lld must be in [0, 2^31)", (long long)n_rows);
    ARX_REQUIRE(max_centroid_norm >= 0.0f && max_centroid_norm < INFINITY,
                "max_centroid_norm=%g must be positive and finite (0: 1 + 2^-9)", (double)max_centroid_norm);
    ARX_REQUIRE(tau_mult == 0.0f || (tau_mult >= 1.0f && tau_mult < INFINITY), "tau_mult=%g must be 0 (= 1) or a finite value >= 1",
                (double)tau_mult);
    ARX_REQUIRE(rows_per_block == 0 || rows_per_block == 32 || rows_per_block == 64, "rows_per_block=%d must be 0 (default), 32 or 64",
                rows_per_block);
    ARX_REQUIRE(rows || n_rows == 0, "rows is a null pointer (n_rows=%lld)", (long long)n_rows);
    ARX_REQUIRE((uintptr_t)rows % 16 == 0, "rows must be 16-byte aligned");
    ARX_REQUIRE(centroids, "centroids_f16 is a null pointer");
    ARX_REQUIRE((uintptr_t)centroids % 16 == 0, "centroids_f16 must be 16-byte aligned");
    ARX_REQUIRE(out_labels || n_rows == 0, "out_labels is a null pointer");
    ARX_REQUIRE(out_scores || n_rows == 0, "out_scores is a null pointer");
    ARX_REQUIRE((uintptr_t)out_labels % 16 == 0 && (uintptr_t)out_scores % 16 == 0, "out_labels and out_scores must be 16-byte aligned");
    ARX_REQUIRE((uintptr_t)stats % 8 == 0, "stats must be 8-byte aligned");
    const int64_t need = arx_cluster_assign_workspace_bytes(n_rows, C, dim);
    ARX_REQUIRE(ws_bytes >= need, "ws_bytes=%lld is below the %lld bytes arx_cluster_assign_workspace_bytes gives", (long long)ws_bytes,
                (long long)need);
    ARX_REQUIRE(ws, "ws is a null pointer");
    ARX_REQUIRE((uintptr_t)ws % 16 == 0, "ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        if (stats) ARX_HIP_CHECK(hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), st));
        return ARX_OK;
    }
    const float bound = max_centroid_norm == 0.0f ? 1.0f + 1.0f / 512.0f : max_centroid_norm;
    const float tau2 = 2.0f * (tau_mult == 0.0f ? 1.0f : tau_mult) * (1.0625f * (float)dim + 4.0f) * 5.9604645e-8f * bound;
    const int R = rows_per_block ? rows_per_block : 32;
    const int KC = (int64_t)R * dim <= CA_WHOLE_HALVES ? dim : CA_CHUNK_HALVES / R;
    const int smem = R * (KC + CA_PAD) * (int)sizeof(f16_t);
    int* counter = (int*)ws;
    int32_t* list = (int32_t*)((char*)ws + 16);
    ARX_HIP_CHECK(hipMemsetAsync(counter, 0, 16, st));
    const unsigned blocks = (unsigned)((n_rows + R - 1) / R);
    if (R == 32) {
        ARX_HIP_CHECK(arx_func_smem((const void*)assign_fast_kernel<1, 4>, smem));
        assign_fast_kernel<1, 4><<<blocks, CA_NT, smem, st>>>((const f16_t*)rows, (int)n_rows, dim, (const f16_t*)centroids, C, KC, tau2, out_labels,
                                                              out_scores, list, counter);
    } else {
        ARX_HIP_CHECK(arx_func_smem((const void*)assign_fast_kernel<2, 2>, smem));
        assign_fast_kernel<2, 2><<<blocks, CA_NT, smem, st>>>((const f16_t*)rows, (int)n_rows, dim, (const f16_t*)centroids, C, KC, tau2, out_labels,
                                                              out_scores, list, counter);
    }
    const unsigned sblocks = (unsigned)(n_rows < CA_SLOW_BLOCKS ? n_rows : CA_SLOW_BLOCKS);
    assign_slow_kernel<<<sblocks, CA_NT, dim * (int)sizeof(f16_t), st>>>((const f16_t*)rows, (int)n_rows, dim, (const f16_t*)centroids, C, list, counter,
                                                                        out_labels, out_scores, stats);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

}  // namespace

extern "C" int64_t arx_cluster_assign_workspace_bytes(int64_t n_rows, int32_t C, int32_t dim) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || C < 1 || C > CA_C_MAX || dim < 64 || dim > CA_DIM_MAX || dim % 64 != 0) return -1;
    return 16 + round_up64(n_rows * (int64_t)sizeof(int32_t), 16);
}

extern "C" int32_t arx_cluster_assign(const void* rows, int64_t n_rows, int32_t dim, const void* centroids_f16, int32_t C, float max_centroid_norm,
                                      int32_t* out_labels, float* out_scores, int64_t* stats, void* ws, int64_t ws_bytes, void* stream) {
    return cluster_assign_impl(rows, n_rows, dim, centroids_f16, C, max_centroid_norm, out_labels, out_scores, stats, ws, ws_bytes, 0.0f, 0, stream);
}

extern "C" int32_t arx_cluster_assign_tuned(const void* rows, int64_t n_rows, int32_t dim, const void* centroids_f16, int32_t C,
                                            float max_centroid_norm, int32_t* out_labels, float* out_scores, int64_t* stats, void* ws,
                                            int64_t ws_bytes, float tau_mult, int32_t rows_per_block, void* stream) {
    return cluster_assign_impl(rows, n_rows, dim, centroids_f16, C, max_centroid_norm, out_labels, out_scores, stats, ws, ws_bytes, tau_mult,
                               rows_per_block, stream);
}
