// arx_cluster_sums / arx_cluster_finish: the update half of a spherical k-means (Lloyd) iteration over fp16 rows (gfx950; C ABI in
// include/arx.h; the host layer is arxiv_rag_amd/topics.py; the definitions are INTEGRATION.md "Topics").  The assign half is
// arx_cluster_assign (cluster_assign.hip).
//
// Sums.  `order` lists the member rows sorted by (cluster, row), `start[c]` is where cluster c begins in it.  s = start clamped into
// [0, n_members] and made non-decreasing (a running maximum), so cluster c owns order[s[c], s[c + 1]).  Its members are cut into RUNS
// of 256 consecutive entries of `order`; run j of cluster c is entries [s[c] + 256 j, min(s[c] + 256 j + 256, s[c + 1])).
//   1. partials   p(c, j)[d] = 0.0f, then += float(X[r][d]) entry by entry in ascending position, each a plain f32 add (fp16 -> f32 is
//                 exact).  An entry outside [0, n_rows) keeps its position in the run and adds nothing.
//   2. sums       S_c[d] = 0.0f, then += p(c, 0)[d], p(c, 1)[d], ... in ascending j.
// Every (run, 8 dims) is added by ONE thread in this order and every (cluster, 4 dims) of the second pass by one thread, so the bits
// depend on `order` and `start` alone, never on the launch shape.  No atomics.
// Where a partial lives: slot(c, j) = (s[c] >> 8) + c + j.  (s[c] >> 8) + c rises strictly with c and a cluster's runs end before the
// next cluster's first slot (ceil(m / 256) <= floor((s + m) / 256) - floor(s / 256) + 1), so the slots are distinct, lie below
// ceil(n_members / 256) + C (the workspace) and need no prefix sum: the first launch covers every slot, a block finds the cluster of a
// slot by binary search over s and leaves alone a slot no run owns (the second pass never reads it).  The host writes no run table.
// s itself is a running maximum over C + 1 values (list_starts.h, shared with ivf.hip): every block of the first launch scans them into
// LDS (scan_starts: 4 (C + 1) bytes, beside the 256 x dim x 2 bytes a run reads), a block of the second reduces the two values it needs.
// Launch shape of the partials: a thread owns 8 consecutive dims of one run (one 16-byte load per row), dim / 8 threads make a run, a
// block carries `runs_per_block` runs side by side so that small dims still fill its waves (dim 64: 8 lanes a run, 32 runs in a
// 256-thread block); with fewer threads than that, a thread takes several (run, 8 dims) units one after the other.  The loads of 8
// rows are issued before their 8 ordered adds: a wave then keeps 8 KiB in flight and a CU with 8 or more waves resident the 64-72 KiB
// that hide an HBM miss on this chip; all loads are unconditional (a bad or missing entry reads row 0 and is dropped by a select), so
// none waits for another.
//
// Finish.  One wave per cluster.  q_l = the f32 sum over d = l, l + 64, l + 128, ... (ascending) of S[d] * S[d] (the product rounded,
// then added: this file is compiled without FMA contraction), l = lane 0..63; then six butterfly steps v_l = v_l + v_(l ^ o), o = 32,
// 16, 8, 4, 2, 1 (an f32 add commutes, so the two lanes of a pair get the same bits), after which every lane holds the same sum of squares; norm = sqrtf of it; centroid[d] = S[d] / norm (IEEE division).
// A cluster that is empty (s[c + 1] == s[c], start clamped below at 0) or whose norm is 0 or not finite keeps prev[c] bit for bit.
// out_f16 = the f32 centroid rounded to nearest even.
#include "arx_common.h"
#include "list_starts.h"

namespace {

constexpr int CL_RUN = 256;                                   // members of a run
constexpr int CL_DEPTH = 8;                                   // rows whose loads are in flight ahead of the ordered adds
constexpr int CL_DIM_MAX = 8192, CL_C_MAX = 4096;

__global__ __launch_bounds__(1024) void cluster_partials_kernel(const f16_t* __restrict__ rows, int64_t n_rows, int dim, const int* __restrict__ order, int n_members,
                                        const int64_t* __restrict__ start, int C, float* __restrict__ partials, int n_slots,
                                        int runs_per_block) {
    extern __shared__ int s_mem[];
    int* s_start = s_mem;                                     // [C + 1]
    int* s_wave = s_mem + C + 1;                              // [16]
    scan_starts(start, C, n_members, s_start, s_wave);
    const int tpr = dim >> 3;                                 // threads (8-dim chunks) of a run
    const int units = runs_per_block * tpr;
    for (int u = threadIdx.x; u < units; u += blockDim.x) {
        const int sl = u / tpr, ch = u - sl * tpr;
        const int64_t g64 = (int64_t)blockIdx.x * runs_per_block + sl;
        if (g64 >= n_slots) continue;
        const int g = (int)g64;
        int lo = 0, hi = C - 1;                               // the largest c with (s[c] >> 8) + c <= g
        if ((s_start[0] >> 8) > g) continue;                  // (a slot before the first cluster's: s[0] > 0 is outside the contract)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((s_start[mid] >> 8) + mid <= g) lo = mid; else hi = mid - 1;
        }
        const int c = lo, j = g - ((s_start[c] >> 8) + c);
        const int64_t first = (int64_t)s_start[c] + (int64_t)j * CL_RUN;
        const int64_t left = (int64_t)s_start[c + 1] - first;
        if (left <= 0) continue;                              // no run owns this slot
        const int len = left < CL_RUN ? (int)left : CL_RUN;   // first + len <= s[c + 1] <= n_members
        const int* ord = order + first;
        const f16_t* src = rows + ch * 8;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int r[CL_DEPTH], r_next[CL_DEPTH];                    // row numbers of this batch and the next; -1: the entry adds nothing
        auto entries = [&](int i0, int (&out)[CL_DEPTH]) {
#pragma unroll
            for (int k = 0; k < CL_DEPTH; ++k) {
                const int i = i0 + k < len ? i0 + k : len - 1;
                const int v = ord[i];
                out[k] = (i0 + k < len && v >= 0 && v < n_rows) ? v : -1;
            }
        };
        entries(0, r);
        for (int i0 = 0; i0 < len; i0 += CL_DEPTH) {
            f16x8 x[CL_DEPTH];
#pragma unroll
            for (int k = 0; k < CL_DEPTH; ++k) x[k] = *(const f16x8*)(src + (int64_t)(r[k] < 0 ? 0 : r[k]) * dim);
            entries(i0 + CL_DEPTH, r_next);                   // (the next batch's row numbers travel under this batch's rows)
#pragma unroll
            for (int k = 0; k < CL_DEPTH; ++k) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += r[k] < 0 ? 0.0f : (float)x[k][e];  // (+0.0f leaves a sum that began at +0.0f as it is)
            }
#pragma unroll
            for (int k = 0; k < CL_DEPTH; ++k) r[k] = r_next[k];
        }
        float* p = partials + (int64_t)g * dim + ch * 8;
        *(f32x4*)p = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *(f32x4*)(p + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
}

// the running maximum of the clamped start[0 .. c] and of start[0 .. c + 1] (one block, every thread gets both)
__device__ __forceinline__ void cluster_range(const int64_t* __restrict__ start, int c, int n_members, int* s_wave, int& a, int& b) {
    int mine = 0;
    for (int i = threadIdx.x; i <= c; i += blockDim.x) {
        const int v = clamp_start(start[i], n_members);
        mine = v > mine ? v : mine;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(mine, o);
        mine = other > mine ? other : mine;
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    a = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) a = s_wave[w] > a ? s_wave[w] : a;
    const int next = clamp_start(start[c + 1], n_members);
    b = next > a ? next : a;
}

__global__ __launch_bounds__(256) void cluster_reduce_kernel(const float* __restrict__ partials, const int64_t* __restrict__ start, int C,
                                                             int n_members, int dim, int n_slots, float* __restrict__ sums) {
    __shared__ int s_wave[4];
    const int c = blockIdx.x;
    int a, b;
    cluster_range(start, c, n_members, s_wave, a, b);
    const int n_runs = (b - a + CL_RUN - 1) / CL_RUN;
    const int64_t slot0 = (int64_t)(a >> 8) + c;              // slot0 + n_runs <= n_slots (file header); checked all the same
    const int runs = slot0 + n_runs <= n_slots ? n_runs : 0;
    for (int q = threadIdx.x; q < (dim >> 2); q += blockDim.x) {
        const float* p = partials + slot0 * dim + q * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < runs; j0 += CL_DEPTH) {
            f32x4 v[CL_DEPTH];
#pragma unroll
            for (int k = 0; k < CL_DEPTH; ++k) {
                const int j = j0 + k < runs ? j0 + k : runs - 1;
                v[k] = *(const f32x4*)(p + (int64_t)j * dim);
            }
#pragma unroll
            for (int k = 0; k < CL_DEPTH; ++k)
                if (j0 + k < runs) acc += v[k];
        }
        *(f32x4*)(sums + (int64_t)c * dim + q * 4) = acc;
    }
}

__global__ __launch_bounds__(64) void cluster_finish_kernel(const float* __restrict__ sums, const int64_t* __restrict__ start,
                                                            const float* __restrict__ prev, int C, int dim, float* __restrict__ out_f32,
                                                            f16_t* __restrict__ out_f16) {
    __shared__ int s_wave[1];
    const int c = blockIdx.x, lane = threadIdx.x;
    int a, b;
    cluster_range(start, c, 0x7fffffff, s_wave, a, b);
    const float* S = sums + (int64_t)c * dim;
    float q = 0.0f;
    for (int d = lane; d < dim; d += 64) q += S[d] * S[d];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q = q + __shfl_xor(q, o);
    const float norm = sqrtf(q);
    const bool keep = b == a || !(norm > 0.0f) || !(norm < __builtin_inff());      // (a NaN norm fails both comparisons)
    const float* P = prev + (int64_t)c * dim;
    for (int d = lane; d < dim; d += 64) {
        const float v = keep ? P[d] : S[d] / norm;
        out_f32[(int64_t)c * dim + d] = v;
        out_f16[(int64_t)c * dim + d] = (f16_t)v;
    }
}

// runs a block carries by default: the fewest that fill whole waves, doubled while the block stays within `block_threads`
int default_runs_per_block(int dim, int block_threads) {
    const int tpr = dim / 8;
    int g = tpr, m = 64;
    while (m) { const int t = g % m; g = m; m = t; }          // g = gcd(tpr, 64)
    int rpb = 64 / g;
    if (rpb * tpr > block_threads) return 1;
    while (rpb * tpr * 2 <= block_threads) rpb *= 2;
    return rpb;
}

int cluster_sums_impl(const void* rows, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start, int32_t C,
                      void* partials, int64_t ws_bytes, float* sums, int32_t block_threads, int32_t runs_per_block, void* stream) {
    ARX_REQUIRE(dim >= 64 && dim <= CL_DIM_MAX && dim % 64 == 0, "dim=%d must be a multiple of 64 in [64, %d]", dim, CL_DIM_MAX);
    ARX_REQUIRE(C >= 1 && C <= CL_C_MAX, "C=%d must be in [1, %d]", C, CL_C_MAX);
    ARX_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows=%lld must be in [0, 2^31)", (long long)n_rows);
    ARX_REQUIRE(n_members >= 0 && n_members < ((int64_t)1 << 31), "n_members=%lld must be in [0, 2^31)", (long long)n_members);
    ARX_REQUIRE(block_threads >= 64 && block_threads <= 1024 && block_threads % 64 == 0,
                "block_threads=%d must be a multiple of 64 in [64, 1024]", block_threads);
    ARX_REQUIRE(runs_per_block >= 0 && runs_per_block <= 64, "runs_per_block=%d must be in [0, 64] (0: the default)", runs_per_block);
    ARX_REQUIRE(start, "start is a null pointer");
    ARX_REQUIRE(sums, "sums is a null pointer");
    ARX_REQUIRE(rows || n_rows == 0, "rows is a null pointer (n_rows=%lld)", (long long)n_rows);
    ARX_REQUIRE((uintptr_t)rows % 16 == 0, "rows must be 16-byte aligned");
    ARX_REQUIRE(order || n_members == 0, "order is a null pointer (n_members=%lld)", (long long)n_members);
    const int64_t need = arx_cluster_sums_workspace_bytes(n_members, C, dim);
    ARX_REQUIRE(ws_bytes >= need, "ws_bytes=%lld is below the %lld bytes arx_cluster_sums_workspace_bytes gives", (long long)ws_bytes,
                (long long)need);
    ARX_REQUIRE(partials, "partials is a null pointer");
    ARX_REQUIRE((uintptr_t)partials % 16 == 0 && (uintptr_t)sums % 16 == 0, "partials and sums must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n_members == 0 || n_rows == 0) {                      // no member adds anything
        ARX_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)C * dim * sizeof(float), st));
        return ARX_OK;
    }
    const int n_slots = (int)((n_members + CL_RUN - 1) / CL_RUN) + C;
    const int rpb = runs_per_block > 0 ? runs_per_block : default_runs_per_block(dim, block_threads);
    const int smem = (C + 1 + 16) * (int)sizeof(int);
    cluster_partials_kernel<<<(unsigned)((n_slots + rpb - 1) / rpb), block_threads, smem, st>>>(
        (const f16_t*)rows, n_rows, dim, order, (int)n_members, start, C, (float*)partials, n_slots, rpb);
    cluster_reduce_kernel<<<(unsigned)C, 256, 0, st>>>((const float*)partials, start, C, (int)n_members, dim, n_slots, sums);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

}  // namespace

extern "C" int64_t arx_cluster_sums_workspace_bytes(int64_t n_members, int32_t C, int32_t dim) {
    if (n_members < 0 || n_members >= ((int64_t)1 << 31) || C < 1 || C > CL_C_MAX || dim < 64 || dim > CL_DIM_MAX || dim % 64 != 0) return -1;
    return ((n_members + CL_RUN - 1) / CL_RUN + C) * dim * (int64_t)sizeof(float);
}

extern "C" int32_t arx_cluster_sums(const void* rows, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                                    int32_t C, void* partials, int64_t ws_bytes, float* sums, void* stream) {
    return cluster_sums_impl(rows, n_rows, dim, order, n_members, start, C, partials, ws_bytes, sums, 256, 0, stream);
}

extern "C" int32_t arx_cluster_sums_tuned(const void* rows, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members,
                                          const int64_t* start, int32_t C, void* partials, int64_t ws_bytes, float* sums, int32_t block_threads,
                                          int32_t runs_per_block, void* stream) {
    return cluster_sums_impl(rows, n_rows, dim, order, n_members, start, C, partials, ws_bytes, sums, block_threads, runs_per_block, stream);
}

extern "C" int32_t arx_cluster_finish(const float* sums, const int64_t* start, const float* prev, int32_t C, int32_t dim, float* out_f32,
                                      void* out_f16, void* stream) {
    ARX_REQUIRE(dim >= 64 && dim <= CL_DIM_MAX && dim % 64 == 0, "dim=%d must be a multiple of 64 in [64, %d]", dim, CL_DIM_MAX);
    ARX_REQUIRE(C >= 1 && C <= CL_C_MAX, "C=%d must be in [1, %d]", C, CL_C_MAX);
    ARX_REQUIRE(sums, "sums is a null pointer");
    ARX_REQUIRE(start, "start is a null pointer");
    ARX_REQUIRE(prev, "prev is a null pointer");
    ARX_REQUIRE(out_f32, "out_f32 is a null pointer");
    ARX_REQUIRE(out_f16, "out_f16 is a null pointer");
    cluster_finish_kernel<<<(unsigned)C, 64, 0, (hipStream_t)stream>>>(sums, start, prev, C, dim, out_f32, (f16_t*)out_f16);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
