// arx_hybrid_fuse: relative-score fusion of a dense and a keyword candidate list per query, on the device (gfx950; C ABI in
// include/arx.h).  It computes arxiv_rag_amd/keyword.py `fuse`, bit for bit:
//   members    the slots of a list with id >= 0 (ids are distinct within a list: the caller's contract)
//   norm       per list, in float64: (s - min) / (max - min) over its members, 1.0 for every member when max == min
//   fused      alpha * normD + (1.0 - alpha) * normK over the union of the two lists, a row absent from a list getting 0.0 from that
//              side: two separately rounded float64 multiplications and one addition
//   answer     the best k rows by (fused desc, id asc) as (fused f64, id, dense f32, keyword f32); the two score columns are NaN where
//              the row was not in that list; unused slots are (-inf, -1, NaN, NaN)
// No FMA contraction: this file is compiled with -ffp-contract=off (csrc/build.sh) AND carries the pragma below, so the statement
// `alpha * nd + oma * nk` stays two v_mul_f64 and one v_add_f64 whatever the library's default flags are.  The f64 division is the
// compiler's IEEE-rounded sequence (no fast-math flag is given).
// One block of 512 threads per query, everything in LDS (static, 40 KiB): up to 2048 entries of (id i64, key u64, payload u32).
//   1. the n_dense + n_kw slots are loaded as (id, source slot); a slot with id < 0 gets id = INT64_MAX and sorts to the end
//   2. bitonic sort by (id asc, source asc): a row of both lists is two neighbours, the dense one first
//   3. min and max of each list's members: wave shuffles, then one LDS round (f32: the conversion to f64 is monotonic and exact)
//   4. the first entry of every run of equal ids becomes the row's (fused key, id, dense slot, keyword slot); every other entry "none"
//   5. bitonic sort by (fused desc, id asc); fused >= 0, so its f64 bit pattern + 1 is an unsigned key with 0 left for "none"
//   6. the first k entries are stored
// Ids are compared as int64 throughout: nothing is packed into 32 bits.  No atomics of any kind, no workspace, plain vector stores; a
// query's output depends on its own two lists, alpha and k alone.
#include <math.h>

#include "arx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FUSE_NT = 512;
constexpr int FUSE_MAX = 1024;                  // longest list, largest k
constexpr int FUSE_CAP = 2 * FUSE_MAX;          // entries of a block
constexpr int FUSE_PER = FUSE_CAP / FUSE_NT;    // entries per thread in step 4
constexpr long long FUSE_NO_ID = 0x7fffffffffffffffll;

struct FuseSmem {
    long long id[FUSE_CAP];
    unsigned long long key[FUSE_CAP];           // step 5: f64 bits of fused + 1, 0 = none
    uint32_t pay[FUSE_CAP];                     // steps 1-2: the source slot (dense: e, keyword: n_dense + e); steps 4-6: (dense slot + 1) | (keyword slot + 1) << 16, 0 = absent
    float red[4][FUSE_NT / 64];                 // dense min, dense max, keyword min, keyword max per wave
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// bitonic sort of m entries (a power of two, <= FUSE_CAP): before(a, b) = the entry at a must precede the entry at b.  The whole block;
// earlier writes are behind a barrier already; ends with a barrier.
template <class Before, class Swap>
__device__ __forceinline__ void fuse_bitonic(int m, Before before, Swap swap) {
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (m >> 1); t += FUSE_NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;          // p < m
                if (((i & k) == 0) ? before(p, i) : before(i, p)) swap(i, p);
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(FUSE_NT) void hybrid_fuse_kernel(const float* __restrict__ dense_s, const long long* __restrict__ dense_i, int n_dense,
                                                              const float* __restrict__ kw_s, const long long* __restrict__ kw_i, int n_kw,
                                                              double alpha, int k, double* __restrict__ out_f, long long* __restrict__ out_i,
                                                              float* __restrict__ out_d, float* __restrict__ out_k) {
    __shared__ FuseSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    dense_s += (long long)q * n_dense; dense_i += (long long)q * n_dense;
    kw_s += (long long)q * n_kw; kw_i += (long long)q * n_kw;
    const int total = n_dense + n_kw;                        // <= FUSE_CAP
    int m = 64;
    while (m < total) m <<= 1;
    // 1 + 3a: load, and each thread's share of the four extrema
    float dlo = INFINITY, dhi = -INFINITY, klo = INFINITY, khi = -INFINITY;
    for (int e = tid; e < m; e += FUSE_NT) {
        long long id = FUSE_NO_ID;
        if (e < total) {
            const bool d = e < n_dense;
            const long long v = d ? dense_i[e] : kw_i[e - n_dense];
            if (v >= 0) {
                id = v;
                const float s = d ? dense_s[e] : kw_s[e - n_dense];
                if (d) { dlo = fminf(dlo, s); dhi = fmaxf(dhi, s); } else { klo = fminf(klo, s); khi = fmaxf(khi, s); }
            }
        }
        sm.id[e] = id;
        sm.pay[e] = (uint32_t)e;
    }
    dlo = wave_min(dlo); dhi = wave_max(dhi); klo = wave_min(klo); khi = wave_max(khi);
    if (lane == 0) { sm.red[0][wave] = dlo; sm.red[1][wave] = dhi; sm.red[2][wave] = klo; sm.red[3][wave] = khi; }
    __syncthreads();
    // 2
    fuse_bitonic(m,
                 [&](int a, int b) { return sm.id[a] < sm.id[b] || (sm.id[a] == sm.id[b] && sm.pay[a] < sm.pay[b]); },
                 [&](int a, int b) {
                     const long long x = sm.id[a]; sm.id[a] = sm.id[b]; sm.id[b] = x;
                     const uint32_t y = sm.pay[a]; sm.pay[a] = sm.pay[b]; sm.pay[b] = y;
                 });
    // 3b
#pragma unroll
    for (int w = 0; w < FUSE_NT / 64; ++w) {
        dlo = fminf(dlo, sm.red[0][w]); dhi = fmaxf(dhi, sm.red[1][w]); klo = fminf(klo, sm.red[2][w]); khi = fmaxf(khi, sm.red[3][w]);
    }
    const double dlo64 = (double)dlo, dspan = (double)dhi - (double)dlo, klo64 = (double)klo, kspan = (double)khi - (double)klo;
    const double oma = 1.0 - alpha;
    // 4: into registers, a barrier, then back (an entry reads its right neighbour's payload)
    unsigned long long nkey[FUSE_PER];
    uint32_t npay[FUSE_PER];
#pragma unroll
    for (int u = 0; u < FUSE_PER; ++u) {
        const int e = tid + u * FUSE_NT;
        nkey[u] = 0ull; npay[u] = 0u;
        if (e < m) {
            const long long id = sm.id[e];
            if (id != FUSE_NO_ID && (e == 0 || sm.id[e - 1] != id)) {
                int ds = -1, ks = -1;                        // the row's slot in the dense / the keyword list
                const int s0 = (int)sm.pay[e];
                if (s0 < n_dense) ds = s0; else ks = s0 - n_dense;
                if (e + 1 < m && sm.id[e + 1] == id) {       // its other list (the dense entry sorts first)
                    const int s1 = (int)sm.pay[e + 1];
                    if (s1 < n_dense) ds = s1; else ks = s1 - n_dense;
                }
                double nd = 0.0, nk = 0.0;
                if (ds >= 0) nd = dspan == 0.0 ? 1.0 : ((double)dense_s[ds] - dlo64) / dspan;
                if (ks >= 0) nk = kspan == 0.0 ? 1.0 : ((double)kw_s[ks] - klo64) / kspan;
                const double a = alpha * nd, b = oma * nk;   // (contraction is off: two products, one sum)
                const double fused = a + b;
                nkey[u] = (unsigned long long)__double_as_longlong(fused) + 1ull;
                npay[u] = (uint32_t)(ds + 1) | ((uint32_t)(ks + 1) << 16);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < FUSE_PER; ++u) {
        const int e = tid + u * FUSE_NT;
        if (e < m) {
            sm.key[e] = nkey[u];
            sm.pay[e] = npay[u];
            if (nkey[u] == 0ull) sm.id[e] = FUSE_NO_ID;      // every "none" entry is the same entry
        }
    }
    __syncthreads();
    // 5
    fuse_bitonic(m,
                 [&](int a, int b) { return sm.key[a] > sm.key[b] || (sm.key[a] == sm.key[b] && sm.id[a] < sm.id[b]); },
                 [&](int a, int b) {
                     const unsigned long long z = sm.key[a]; sm.key[a] = sm.key[b]; sm.key[b] = z;
                     const long long x = sm.id[a]; sm.id[a] = sm.id[b]; sm.id[b] = x;
                     const uint32_t y = sm.pay[a]; sm.pay[a] = sm.pay[b]; sm.pay[b] = y;
                 });
    // 6
    const float nan32 = __uint_as_float(0x7fc00000u);
    for (int r = tid; r < k; r += FUSE_NT) {
        const unsigned long long key = r < m ? sm.key[r] : 0ull;
        const long long o = (long long)q * k + r;
        if (key) {
            const uint32_t pay = sm.pay[r];
            const int ds = (int)(pay & 0xffffu) - 1, ks = (int)(pay >> 16) - 1;
            out_f[o] = __longlong_as_double((long long)(key - 1ull));
            out_i[o] = sm.id[r];
            out_d[o] = ds >= 0 ? dense_s[ds] : nan32;
            out_k[o] = ks >= 0 ? kw_s[ks] : nan32;
        } else {
            out_f[o] = -(double)INFINITY; out_i[o] = -1ll; out_d[o] = nan32; out_k[o] = nan32;
        }
    }
}

}  // namespace

extern "C" int32_t arx_hybrid_fuse(const float* dense_scores, const int64_t* dense_ids, int32_t n_dense, const float* kw_scores,
                                   const int64_t* kw_ids, int32_t n_kw, int32_t n_queries, double alpha, int32_t k, double* out_fused,
                                   int64_t* out_ids, float* out_dense, float* out_kw, void* stream) {
    ARX_REQUIRE(dense_scores && dense_ids && kw_scores && kw_ids && out_fused && out_ids && out_dense && out_kw, "null pointer argument");
    ARX_REQUIRE(n_dense >= 1 && n_dense <= FUSE_MAX, "n_dense=%d must be in [1, %d]", n_dense, FUSE_MAX);
    ARX_REQUIRE(n_kw >= 1 && n_kw <= FUSE_MAX, "n_kw=%d must be in [1, %d]", n_kw, FUSE_MAX);
    ARX_REQUIRE(k >= 1 && k <= FUSE_MAX, "k=%d must be in [1, %d]", k, FUSE_MAX);
    ARX_REQUIRE(n_queries > 0, "n_queries=%d must be positive", n_queries);
    ARX_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "alpha=%g must be in [0, 1]", alpha);
    hybrid_fuse_kernel<<<n_queries, FUSE_NT, 0, (hipStream_t)stream>>>(dense_scores, (const long long*)dense_ids, n_dense, kw_scores,
                                                                       (const long long*)kw_ids, n_kw, alpha, k, out_fused,
                                                                       (long long*)out_ids, out_dense, out_kw);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
