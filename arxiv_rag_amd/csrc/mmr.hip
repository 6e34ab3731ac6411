// arx_gather_rows / arx_mmr_select: maximal-marginal-relevance re-ordering of a query's n <= 32 search candidates (C ABI in
// include/arx.h; the definition is INTEGRATION.md "MMR").
//
//   gather   out[s] = shard row ids[s] - idx_base, or zeros where that row is not in the shard (id -1, a row of another rank): one lane
//            per 16 bytes, every output element written once by a plain vector store.
//   select   one 256-thread block per query.
//            Gram matrix G = C C^T of the query's candidates (32 x 32 x dim, slots >= n and slots with id < 0 are zero rows) on
//            __builtin_amdgcn_mfma_f32_32x32x16_f16: for that instruction lane l holds A[row l & 31][k = 8 (l >> 5) + j] and
//            B[k = 8 (l >> 5) + j][col l & 31] in element j of its fragment, so for C C^T the A fragment and the B fragment of a lane are
//            the SAME eight halves: a lane loads 16 bytes of candidate l & 31 at k0 + 8 (l >> 5) straight from global memory and passes
//            that register as both operands.  No LDS staging of operands.
//            q . c_i comes from a SECOND accumulator of the same instruction with the query fragment (the same k range, the same 16 bytes
//            in every lane of a half) as the A operand and the candidate fragment as B: every row of that product is the vector
//            (q . c_j)_j, so lane l holds q . c_(l & 31) in each of its registers.  q . q is summed on the VALU from the query fragments
//            (fmaf of exact fp16 products), c_i . c_i is the diagonal of G.
//            The four waves split K into four contiguous quarters and sum their accumulators through LDS in wave order 0, 1, 2, 3; the
//            normalised 32 x 32 cosine matrix stays in LDS (4 KiB) and wave 0 runs the greedy loop: lane i holds rel[i], its running
//            maximum similarity to the picks and an "available" flag, the argmax is a wave reduction over (objective, slot) with ties to the
//            lower slot, and after a pick lane i reads sim[pick][i].
// A query's outputs depend on its own query row, candidates and ids only: one block, a fixed accumulation order, no atomics.
#include <math.h>

#include "arx_common.h"

namespace {
#define MMR_SLOTS 32
#define MMR_NT 256
#define MMR_NW (MMR_NT / 64)
#define MMR_AHEAD 8

__global__ __launch_bounds__(256) void gather_rows_kernel(const u32x4* __restrict__ shard, int64_t n_rows, int chunks_per_row, int64_t idx_base,
                                                           const int64_t* __restrict__ ids, int64_t total_chunks, u32x4* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total_chunks) return;
    const int64_t s = t / chunks_per_row;
    const int c = (int)(t - s * chunks_per_row);
    const int64_t id = ids[s];
    u32x4 v = {0u, 0u, 0u, 0u};
    if (id >= idx_base && id - idx_base < n_rows) v = shard[(id - idx_base) * chunks_per_row + c];
    out[t] = v;
}

__global__ __launch_bounds__(MMR_NT) void mmr_select_kernel(const f16_t* __restrict__ Q, const f16_t* __restrict__ cand, const int64_t* __restrict__ ids,
                                                             int n, int D, int m, float lam, int32_t* __restrict__ order, float* __restrict__ mmr) {
    __shared__ float part[MMR_NW][MMR_SLOTS * MMR_SLOTS];       // per-wave partial Gram matrices; part[0] becomes G, then sim
    __shared__ float relp[MMR_NW][MMR_SLOTS];                   // per-wave partial q . c_i
    __shared__ float qqp[MMR_NW][2];                            // per-wave, per lane half partial q . q
    __shared__ float rel_s[MMR_SLOTS], nn_s[MMR_SLOTS];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int slot = lane & 31, h = lane >> 5;
    const bool valid = slot < n && ids[(int64_t)q * n + (slot < n ? slot : 0)] >= 0;
    const f16_t* crow = cand + ((int64_t)q * n + (valid ? slot : 0)) * D;
    const f16_t* qrow = Q + (int64_t)q * D;
    // this wave's quarter of K, 16 values per step; the loads of MMR_AHEAD steps are in flight before the first of them is used
    const int steps = D >> 6, k0 = w * (D >> 2) + 8 * h;
    f32x16 g = {0}, r = {0};
    float qq = 0.f;
    for (int s0 = 0; s0 < steps; s0 += MMR_AHEAD) {
        f16x8 cf[MMR_AHEAD], qf[MMR_AHEAD];
#pragma unroll
        for (int j = 0; j < MMR_AHEAD; ++j) {
            cf[j] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
            qf[j] = cf[j];
            if (s0 + j < steps) {                              // (wave-uniform)
                if (valid) cf[j] = *reinterpret_cast<const f16x8*>(crow + k0 + 16 * (s0 + j));
                qf[j] = *reinterpret_cast<const f16x8*>(qrow + k0 + 16 * (s0 + j));
            }
        }
#pragma unroll
        for (int j = 0; j < MMR_AHEAD; ++j) {
            if (s0 + j < steps) {
                g = __builtin_amdgcn_mfma_f32_32x32x16_f16(cf[j], cf[j], g, 0, 0, 0);
                r = __builtin_amdgcn_mfma_f32_32x32x16_f16(qf[j], cf[j], r, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float v = (float)qf[j][e]; qq = fmaf(v, v, qq); }
            }
        }
    }
    // g[e] belongs to row 8 (e >> 2) + 4 h + (e & 3), column `slot`
#pragma unroll
    for (int e = 0; e < 16; ++e) part[w][(8 * (e >> 2) + 4 * h + (e & 3)) * MMR_SLOTS + slot] = g[e];
    if (h == 0) relp[w][slot] = r[0];
    if (slot == 0) qqp[w][h] = qq;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {                               // G = the partials added in wave order
        const int e = tid + j * MMR_NT;
        part[0][e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
    }
    __syncthreads();
    if (tid < MMR_SLOTS) {
        const float nn = part[0][tid * MMR_SLOTS + tid];
        const float qc = ((relp[0][tid] + relp[1][tid]) + relp[2][tid]) + relp[3][tid];
        const float q2 = ((((((qqp[0][0] + qqp[0][1]) + qqp[1][0]) + qqp[1][1]) + qqp[2][0]) + qqp[2][1]) + qqp[3][0]) + qqp[3][1];
        nn_s[tid] = nn;
        rel_s[tid] = (nn > 0.f && q2 > 0.f) ? qc / sqrtf(q2 * nn) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {                               // sim in place: a thread reads only its own element of G and the norms
        const int e = tid + j * MMR_NT;
        const float ni = nn_s[e >> 5], nj = nn_s[e & 31];
        part[0][e] = (ni > 0.f && nj > 0.f) ? part[0][e] / sqrtf(ni * nj) : 0.f;
    }
    __syncthreads();
    if (w != 0) return;
    // greedy loop, one wave: lanes >= 32 take part in the reduction as unavailable slots
    const float oml = 1.0f - lam;
    const float relv = rel_s[slot];
    bool avail = valid && h == 0;
    float maxsim = -INFINITY;
    for (int t = 0; t < m; ++t) {
        const float obj = t == 0 ? lam * relv : lam * relv - oml * maxsim;
        float bv = avail ? obj : -INFINITY;
        int bp = avail ? lane : 64;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int op = __shfl_xor(bp, o);
            if (op < 64 && (bp == 64 || ov > bv || (ov == bv && op < bp))) { bv = ov; bp = op; }
        }
        const bool found = bp < 64;                            // wave-uniform
        if (lane == 0) {
            order[(int64_t)q * m + t] = found ? bp : -1;
            mmr[(int64_t)q * m + t] = found ? bv : -INFINITY;
        }
        if (!found) continue;
        if (lane == bp) avail = false;
        maxsim = fmaxf(maxsim, part[0][bp * MMR_SLOTS + slot]);
    }
}
}      // namespace

extern "C" int32_t arx_gather_rows(const void* shard, int64_t n_rows, int32_t dim, int64_t idx_base, const int64_t* ids, int64_t count,
                                   void* out, void* stream) {
    ARX_REQUIRE(n_rows >= 0 && count >= 0, "n_rows=%lld count=%lld: must not be negative", (long long)n_rows, (long long)count);
    ARX_REQUIRE(dim > 0 && dim % 8 == 0, "dim=%d must be a positive multiple of 8 (16-byte chunks)", dim);
    if (count == 0) return ARX_OK;
    ARX_REQUIRE((shard || n_rows == 0) && ids && out, "null pointer argument");
    ARX_REQUIRE((uintptr_t)shard % 16 == 0 && (uintptr_t)out % 16 == 0, "shard and out must be 16-byte aligned");
    const int cpr = dim / 8;
    const int64_t total = count * cpr;
    ARX_REQUIRE((total + 255) / 256 < (1ll << 31), "grid too large");
    gather_rows_kernel<<<(int)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>((const u32x4*)shard, n_rows, cpr, idx_base, ids, total,
                                                                                    (u32x4*)out);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_mmr_select(const void* q, const void* cand, const int64_t* ids, int32_t n_queries, int32_t n, int32_t dim, int32_t m,
                                  float lambda, int32_t* order, float* mmr, void* stream) {
    ARX_REQUIRE(dim > 0 && dim % 64 == 0, "dim=%d must be a multiple of 64", dim);
    ARX_REQUIRE(dim <= 8192, "dim=%d: at most 8192", dim);
    ARX_REQUIRE(1 <= m && m <= n && n <= MMR_SLOTS, "m=%d n=%d: need 1 <= m <= n <= %d", m, n, MMR_SLOTS);
    ARX_REQUIRE(lambda >= 0.0f && lambda <= 1.0f, "lambda=%g must be in [0, 1]", (double)lambda);      // (also refuses nan)
    ARX_REQUIRE(n_queries >= 0, "n_queries=%d", n_queries);
    if (n_queries == 0) return ARX_OK;
    ARX_REQUIRE(q && cand && ids && order && mmr, "null pointer argument");
    ARX_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)cand % 16 == 0, "q and cand must be 16-byte aligned");
    mmr_select_kernel<<<n_queries, MMR_NT, 0, (hipStream_t)stream>>>((const f16_t*)q, (const f16_t*)cand, ids, n, dim, m, lambda, order, mmr);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
