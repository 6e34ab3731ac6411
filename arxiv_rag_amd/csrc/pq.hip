// arx_pq_encode / arx_pq_lut / arx_pq_candidates: 8-bit product-quantiser codes of the rows, a query's byte look-up tables, and the
// exact candidate lists by table sum (gfx950; C ABI in include/arx.h; the host layer is arxiv_rag_amd/pq.py; the definition is
// INTEGRATION.md "Product-quantised search").  Compiled without FMA contraction: encode and lut are defined operation by operation.
//
// With M = dim / dsub subspaces and codebooks f32 [M][256][dsub], a row's code is M bytes: byte m names the nearest centroid of
// subspace m to the (centred) row, by a squared distance summed in order, ties to the lower centroid.  A query's table holds, per
// (m, centroid), its inner product with the centroid, mapped to a byte with one scale per query.  s(q, r) = sum_m lut[q][m][codes[r][m]]
// is an integer, so the candidate set is defined exactly: C(q) = the first min(R, visible) visible rows by (s desc, row asc).  The exact
// rescore of C(q) is arx_ivf_search over the candidate lists, as for arx_binary_candidates.
//   encode  block = 256 rows, one lane per row.  Per 64 dimensions a lane reads the 128-byte line of its own row in eight 16-byte
//           loads (every line fetched is used whole, by the lane that fetched it) and keeps the 64 centred values in registers; the
//           64 / dsub subspaces of the chunk follow: the subspace's codebook (1 KiB * dsub) is staged in LDS, and all lanes walk the 256
//           centroids together, so every LDS read is a broadcast of one address.  The block's code bytes collect in LDS [256][M] and
//           leave as one contiguous span (the rows of a block are adjacent in the row-major code array) in 4-byte stores.  Every byte
//           is written once, no atomics.
//   lut     one block per query; wave w takes subspaces w, w + 4, ..., a lane four centroids.  Pass 1 finds each subspace's minimum and
//           the largest spread (wave shuffles, then four values through LDS: min and max of finite values are exact in any order);
//           pass 2 computes the same inner products again (the same instructions, so the same bits) and stores the bytes.  Holding
//           the M * 256 floats instead would need 256 KiB at M = 256; up to M = 96 (dim 768 at dsub 8: 96 KiB) they would fit in LDS
//           and the second read of the codebooks (dim KiB per query block, from L2) could be saved: a second kernel path that has not
//           been written; tools/pq_bench.py's lut_event_ms is the cost it would halve at most.
//   keys    s << 32 | (0xffffffff - row): key_lists.h.
//   scan    block (stretch p of rows_per_block rows, tile t of QT queries), four waves.  The tile's byte tables sit in LDS, M * 256
//           bytes per query, behind the tile's key lists (8 KiB per query).  A round gives every lane one row (a wave's 64 rows are one
//           word of `allow`: a zero word costs that one load); the lane reads its M code bytes once, 16 at a time (4 or 1 where M is
//           no multiple of 16), and for every byte gathers one table byte per query of the tile into an integer sum per query.
//           QT IS CHOSEN FROM M SO THAT TWO BLOCKS FIT A CU: the largest of 8, 4, 2, 1 with QT * (M * 256 + 8 KiB lists) inside 80 KiB
//           (QT = 8 for M <= 7, 4 for M <= 47, 2 for M <= 127, e.g. dim 768 at dsub 8, and 1 up to M = 256: 72 KiB).  The scan is a
//           stream of dependent-address LDS byte gathers with a block-wide sort between rounds now and then; with two blocks per CU
//           one block's gathers run under the other's barriers and code loads.  A larger tile (up to 160 KiB, one block per CU) would
//           read the codes fewer times, but the code bytes are one global byte per QT LDS gathers, so the gathers, not the code
//           reads, set the time.  This choice is reasoned, not measured against the one-block layout.
//           Measured with this layout (profiles/pq_bench.json, 10 M rows, M = 96, QT = 2): the scan takes 0.63 ms at one query and
//           9.5 ms at 64, 4x to 66x the 0.15 ms the code bytes cost, so the gathers do set the time, and the batch pays for them
//           query by query.
//   merge   key_lists.h's, one block per query over any number of parts.
// The candidate path is integer work only, with no global atomics; a query's outputs are the R largest of a set of distinct integer
// keys: they depend on its table, codes and allow alone, not on the batch, the tile, rows_per_block or the workspace.  codes, lut and
// allow are device data of which every bit pattern is a legal value: a code byte indexes 256 table bytes, a table byte is added; bits
// of allow at or beyond n_rows are masked off before use.
// WHERE IT LOSES (by construction): codes stay row-major [n_rows][M] so that arx_compact_rows moves them at row_bytes = M and `add`
// appends them; a lane-per-row read of M-byte rows is therefore strided (a wave's 16-byte loads touch 64 different lines; the lines are
// reused by the lane's next loads, from cache), and a wave instruction moves 1 KiB from 64 lines, not from 8.
#include "arx_common.h"
#include "key_lists.h"

namespace {
constexpr int PQ_NT = KEY_NT, PQ_NW = PQ_NT / 64;
constexpr int PQ_CODES = 256;                   // centroids of a subspace: one byte
constexpr int PQ_M_MAX = 256;
constexpr int PQ_DIM_MAX = 8192;
constexpr int PQ_LDS_BLOCK = 80 * 1024;         // a scan block's LDS: two blocks per CU
constexpr int PQ_BLOCKS_TARGET = 1024;          // the default rows_per_block aims at this many scan blocks
constexpr int PQ_RPB_MIN_DEFAULT = 2048;
constexpr int PQ_RPB_LIMIT = 1 << 20;

// ---- encode -------------------------------------------------------------------------------------------------------------------------------
template <int DS>
__global__ __launch_bounds__(PQ_NT) void pq_encode_kernel(const f16_t* __restrict__ x, int64_t n_rows, int dim, const float* __restrict__ centre,
                                                          const float* __restrict__ cb, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* cbs = reinterpret_cast<float*>(smem);                                          // [256][DS]: the subspace's codebook
    uint8_t* cs = reinterpret_cast<uint8_t*>(smem + PQ_CODES * DS * 4);                   // [PQ_NT][M]: the block's codes
    const int M = dim / DS, tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PQ_NT;                                      // < n_rows
    const int64_t row = row0 + tid;
    const f16_t* xr = x + (row < n_rows ? row : row0) * dim;                               // (a lane without a row encodes the block's first)
    for (int c0 = 0; c0 < dim; c0 += 64) {
        float v[64];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f16x8 h = *reinterpret_cast<const f16x8*>(xr + c0 + 8 * i);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * i + e] = (float)h[e];
        }
        if (centre) {
#pragma unroll
            for (int t = 0; t < 64; ++t) v[t] = v[t] - centre[c0 + t];                    // block-uniform addresses
        }
#pragma unroll
        for (int s = 0; s < 64 / DS; ++s) {
            const int m = c0 / DS + s;
            __syncthreads();                                                               // the previous subspace's codebook has been read
            const float4* src = reinterpret_cast<const float4*>(cb + (int64_t)m * PQ_CODES * DS);
            for (int t = tid; t < PQ_CODES * DS / 4; t += PQ_NT) reinterpret_cast<float4*>(cbs)[t] = src[t];
            __syncthreads();
            float best = 0.f;
            int code = 0;
            for (int j = 0; j < PQ_CODES; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int t4 = 0; t4 < DS; t4 += 4) {
                    const float4 c = *reinterpret_cast<const float4*>(cbs + j * DS + t4);  // one address for the whole wave
                    const float e0 = v[s * DS + t4] - c.x, e1 = v[s * DS + t4 + 1] - c.y, e2 = v[s * DS + t4 + 2] - c.z,
                                e3 = v[s * DS + t4 + 3] - c.w;
                    acc = acc + e0 * e0;
                    acc = acc + e1 * e1;
                    acc = acc + e2 * e2;
                    acc = acc + e3 * e3;
                }
                if (j == 0) best = acc;
                else if (acc < best) { best = acc; code = j; }                             // strict: ties to the lower j, NaN never wins
            }
            cs[tid * M + m] = (uint8_t)code;
        }
    }
    __syncthreads();
    const int64_t left = n_rows - row0;
    const int nbytes = (int)(left < PQ_NT ? left : PQ_NT) * M;                             // the block's span of the code array
    uint8_t* dst = out + row0 * M;                                                         // 16-byte aligned: row0 * M is a multiple of 256
    for (int t = tid; t < nbytes / 4; t += PQ_NT) reinterpret_cast<uint32_t*>(dst)[t] = reinterpret_cast<const uint32_t*>(cs)[t];
    if (tid < (nbytes & 3)) dst[(nbytes & ~3) + tid] = cs[(nbytes & ~3) + tid];
}

// ---- lut ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pq_dot(const float* __restrict__ qf, const float* __restrict__ c, int dsub) {
    float acc = 0.f;
    for (int t = 0; t < dsub; t += 4) {
        const float4 cv = *reinterpret_cast<const float4*>(c + t);
        acc = acc + qf[t] * cv.x;
        acc = acc + qf[t + 1] * cv.y;
        acc = acc + qf[t + 2] * cv.z;
        acc = acc + qf[t + 3] * cv.w;
    }
    return acc;
}

__global__ __launch_bounds__(PQ_NT) void pq_lut_kernel(const f16_t* __restrict__ q, int dim, int dsub, const float* __restrict__ cb,
                                                       uint8_t* __restrict__ out) {
    __shared__ float qs[PQ_DIM_MAX];
    __shared__ float lo_s[PQ_M_MAX];
    __shared__ float span_w[PQ_NW];
    __shared__ int bad_w[PQ_NW];
    const int M = dim / dsub, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t qi = blockIdx.x;
    for (int t = tid; t < dim; t += PQ_NT) qs[t] = (float)q[qi * dim + t];
    __syncthreads();
    float span = 0.f;
    int bad = 0;
    for (int m = w; m < M; m += PQ_NW) {                                                   // wave-uniform
        float lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int i = 0; i < PQ_CODES / 64; ++i) {
            const float f = pq_dot(qs + m * dsub, cb + ((int64_t)m * PQ_CODES + lane + 64 * i) * dsub, dsub);
            bad |= !isfinite(f);
            lo = fminf(lo, f);
            hi = fmaxf(hi, f);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o));
            hi = fmaxf(hi, __shfl_xor(hi, o));
        }
        if (lane == 0) lo_s[m] = lo;
        span = fmaxf(span, hi - lo);
    }
    bad = __any(bad);
    if (lane == 0) { span_w[w] = span; bad_w[w] = bad; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PQ_NW; ++i) { span = fmaxf(span, span_w[i]); bad |= bad_w[i]; }
    const bool zero = bad || !(span > 0.f) || !isfinite(span);
    const float inv = 255.f / span;
    for (int m = w; m < M; m += PQ_NW) {
        const float lo = lo_s[m];
#pragma unroll
        for (int i = 0; i < PQ_CODES / 64; ++i) {
            const int j = lane + 64 * i;
            const float f = pq_dot(qs + m * dsub, cb + ((int64_t)m * PQ_CODES + j) * dsub, dsub);
            const float u = zero ? 0.f : fminf(255.f, rintf((f - lo) * inv));               // in 0..255
            out[(qi * M + m) * PQ_CODES + j] = (uint8_t)(int)u;
        }
    }
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------------------
template <int QT>
constexpr int pq_lists_bytes() { return (int)((sizeof(KeyLists<QT>) + 15) / 16 * 16); }

// V: code bytes per load (16: M % 16 == 0; 4: M % 4 == 0; 1: any M)
template <int QT, int V>
__global__ __launch_bounds__(PQ_NT) void pq_scan_kernel(const uint8_t* __restrict__ codes, int64_t n_rows, int M, const uint8_t* __restrict__ lut,
                                                        int nq, const uint64_t* __restrict__ allow, int R, int64_t rpb,
                                                        unsigned long long* __restrict__ part_k) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    KeyLists<QT>& sm = *reinterpret_cast<KeyLists<QT>*>(smem);
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(smem + pq_lists_bytes<QT>());    // [QT][M][256]
    const int TB = M * PQ_CODES;                                                           // a query's table, a multiple of 256 bytes
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = blockIdx.y * QT;
    const int nl = nq - q0 < QT ? nq - q0 : QT;               // the tile's queries
    for (int t = tid; t < QT * (TB / 16); t += PQ_NT) {
        const int l = t / (TB / 16), o = t % (TB / 16);
        uint4 val = {0u, 0u, 0u, 0u};
        if (l < nl) val = reinterpret_cast<const uint4*>(lut + (int64_t)(q0 + l) * TB)[o];
        reinterpret_cast<uint4*>(smem + pq_lists_bytes<QT>())[t] = val;
    }
    if (tid < QT) { sm.cnt[tid] = 0; sm.thr[tid] = 0ull; }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * rpb;             // a multiple of 64
    const int64_t hi = lo + rpb < n_rows ? lo + rpb : n_rows;
    for (int64_t base = lo; base < hi; base += PQ_NT) {       // block-uniform
        const unsigned full = key_full_mask(sm, nl);
        __syncthreads();                                       // everyone has read cnt before anyone appends or cuts
        if (full) key_cut(sm, full, R);
        const int64_t r0 = base + (int64_t)w * 64;             // the wave's 64 rows: one word of allow
        uint64_t vis = 0ull;
        if (r0 < hi) {
            const int64_t left = hi - r0;
            vis = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
            if (allow) vis &= allow[r0 >> 6];
        }
        if (vis != 0ull) {                                     // wave-uniform
            const int64_t row = r0 + lane;
            const bool on = (vis >> lane) & 1ull;
            const uint8_t* c = codes + (on ? row : r0) * M;    // (a lane without a row reads the wave's first row: inside the array)
            int s[QT];
#pragma unroll
            for (int l = 0; l < QT; ++l) s[l] = 0;
            for (int mm = 0; mm < M; mm += V) {
                uint32_t xw[V >= 4 ? V / 4 : 1];
                if constexpr (V == 16) {
                    const uint4 v = *reinterpret_cast<const uint4*>(c + mm);
                    xw[0] = v.x; xw[1] = v.y; xw[2] = v.z; xw[3] = v.w;
                } else if constexpr (V == 4) {
                    xw[0] = *reinterpret_cast<const uint32_t*>(c + mm);
                } else {
                    xw[0] = c[mm];
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const uint8_t* t = tab + (mm + e) * PQ_CODES + ((xw[e >> 2] >> (8 * (e & 3))) & 255u);
#pragma unroll
                    for (int l = 0; l < QT; ++l) s[l] += t[l * TB];
                }
            }
            if (on) {
                const unsigned long long low = (unsigned long long)(0xffffffffu - (uint32_t)row);
#pragma unroll
                for (int l = 0; l < QT; ++l)
                    if (l < nl) key_append(sm, l, ((unsigned long long)(uint32_t)s[l] << 32) | low);
            }
        }
        __syncthreads();
    }
    key_cut(sm, (1u << nl) - 1u, R);
    for (int t = tid; t < nl * R; t += PQ_NT) {
        const int l = t / R, r = t % R;
        part_k[((int64_t)blockIdx.x * nq + q0 + l) * R + r] = r < sm.cnt[l] ? sm.keys[l][r] : 0ull;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
bool pq_dim_ok(int32_t dim) { return dim >= 64 && dim % 64 == 0 && dim <= PQ_DIM_MAX; }
bool pq_dsub_ok(int32_t dsub) { return dsub >= 4 && dsub <= 64 && (dsub & (dsub - 1)) == 0; }
bool pq_m_ok(int32_t dim, int32_t dsub) { return dim / dsub >= 1 && dim / dsub <= PQ_M_MAX; }
template <int QT>
constexpr int64_t pq_scan_smem(int M) { return pq_lists_bytes<QT>() + (int64_t)QT * M * PQ_CODES; }  // the kernel's layout: lists, then tables
int pq_tile(int M) {                                           // queries of a scan tile: two blocks per CU
    if (pq_scan_smem<8>(M) <= PQ_LDS_BLOCK) return 8;
    if (pq_scan_smem<4>(M) <= PQ_LDS_BLOCK) return 4;
    if (pq_scan_smem<2>(M) <= PQ_LDS_BLOCK) return 2;
    return 1;                                                  // M = 256: 8 KiB of lists + 64 KiB of tables
}
static_assert(pq_scan_smem<1>(PQ_M_MAX) <= PQ_LDS_BLOCK, "one query's lists and tables must fit a scan block at the largest M");

#define PQ_REQUIRE_SHAPE(dim, dsub)                                                                                          \
    ARX_REQUIRE(pq_dim_ok(dim), "dim=%d must be a multiple of 64 in 64..%d", dim, PQ_DIM_MAX);                               \
    ARX_REQUIRE(pq_dsub_ok(dsub), "dsub=%d must be a power of two in 4..64", dsub);                                          \
    ARX_REQUIRE(pq_m_ok(dim, dsub), "M=%d (dim / dsub) must be in 1..%d: the look-up tables must fit in LDS", dim / dsub, PQ_M_MAX)

template <int QT, int V>
int32_t pq_launch_scan(dim3 grid, hipStream_t st, const uint8_t* codes, int64_t n_rows, int M, const uint8_t* lut, int nq, const uint64_t* allow,
                       int R, int64_t rpb, unsigned long long* part_k) {
    const int smem = (int)pq_scan_smem<QT>(M);                 // <= PQ_LDS_BLOCK by pq_tile
    ARX_HIP_CHECK(arx_func_smem((const void*)pq_scan_kernel<QT, V>, smem));
    pq_scan_kernel<QT, V><<<grid, PQ_NT, smem, st>>>(codes, n_rows, M, lut, nq, allow, R, rpb, part_k);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
template <int QT, typename... A>
int32_t pq_launch_scan_v(int M, A... a) {
    if (M % 16 == 0) return pq_launch_scan<QT, 16>(a...);
    if (M % 4 == 0) return pq_launch_scan<QT, 4>(a...);
    return pq_launch_scan<QT, 1>(a...);
}
}      // namespace

extern "C" int32_t arx_pq_encode(const void* rows, int64_t n_rows, int32_t dim, int32_t dsub, const float* centre, const float* codebooks,
                                 uint8_t* out_codes, void* stream) {
    PQ_REQUIRE_SHAPE(dim, dsub);
    ARX_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 0..2^31-1", (long long)n_rows);
    if (n_rows == 0) return ARX_OK;
    ARX_REQUIRE(rows && codebooks && out_codes, "null pointer argument");
    ARX_REQUIRE(((uintptr_t)rows | (uintptr_t)codebooks | (uintptr_t)out_codes) % 16 == 0 && (uintptr_t)centre % 4 == 0,
                "rows, codebooks and out_codes must be 16-byte and centre 4-byte aligned");
    const int M = dim / dsub;
    const int smem = PQ_CODES * dsub * 4 + PQ_NT * M;         // at most 96 KiB
    const unsigned blocks = (unsigned)((n_rows + PQ_NT - 1) / PQ_NT);
    hipStream_t st = (hipStream_t)stream;
#define PQ_ENCODE(DS)                                                                                                        \
    case DS:                                                                                                                 \
        ARX_HIP_CHECK(arx_func_smem((const void*)pq_encode_kernel<DS>, smem));                                               \
        pq_encode_kernel<DS><<<blocks, PQ_NT, smem, st>>>((const f16_t*)rows, n_rows, dim, centre, codebooks, out_codes);    \
        break
    switch (dsub) {
        PQ_ENCODE(4);
        PQ_ENCODE(8);
        PQ_ENCODE(16);
        PQ_ENCODE(32);
        PQ_ENCODE(64);
    }
#undef PQ_ENCODE
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_pq_lut(const void* queries, int32_t n_queries, int32_t dim, int32_t dsub, const float* codebooks, uint8_t* out_lut,
                              void* stream) {
    PQ_REQUIRE_SHAPE(dim, dsub);
    ARX_REQUIRE(n_queries >= 0, "n_queries=%d is negative", n_queries);
    if (n_queries == 0) return ARX_OK;
    ARX_REQUIRE(queries && codebooks && out_lut, "null pointer argument");
    ARX_REQUIRE((uintptr_t)queries % 2 == 0 && (uintptr_t)codebooks % 16 == 0, "queries must be 2-byte and codebooks 16-byte aligned");
    pq_lut_kernel<<<(unsigned)n_queries, PQ_NT, 0, (hipStream_t)stream>>>((const f16_t*)queries, dim, dsub, codebooks, out_lut);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int64_t arx_pq_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t dsub, int32_t n_candidates) {
    if (!(n_rows >= 0 && n_rows < (1ll << 31) && n_queries >= 1 && pq_dim_ok(dim) && pq_dsub_ok(dsub) && pq_m_ok(dim, dsub) &&
          n_candidates >= 1 && n_candidates <= KEY_R_MAX))
        return -1;
    return key_layout(n_rows, n_queries, n_candidates).total;
}

extern "C" int32_t arx_pq_candidates_tuned(const uint8_t* codes, int64_t n_rows, int32_t dim, int32_t dsub, const uint8_t* lut,
                                           int32_t n_queries, const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_sum,
                                           int64_t* out_count, void* ws, int64_t ws_bytes, int32_t rows_per_block, void* stream) {
    const int R = n_candidates;
    ARX_REQUIRE(R >= 1 && R <= KEY_R_MAX, "n_candidates=%d out of range 1..%d", R, KEY_R_MAX);
    PQ_REQUIRE_SHAPE(dim, dsub);
    ARX_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 0..2^31-1", (long long)n_rows);
    ARX_REQUIRE(n_queries >= 0, "n_queries=%d is negative", n_queries);
    ARX_REQUIRE(rows_per_block == 0 || (rows_per_block >= 64 && rows_per_block % 64 == 0 && rows_per_block <= PQ_RPB_LIMIT),
                "rows_per_block=%d: 0 (default) or a multiple of 64 in 64..%d", rows_per_block, PQ_RPB_LIMIT);
    if (n_queries == 0) return ARX_OK;
    ARX_REQUIRE(lut && out_cand && out_count && ws && (codes || n_rows == 0), "null pointer argument");
    ARX_REQUIRE(((uintptr_t)codes | (uintptr_t)lut | (uintptr_t)ws) % 16 == 0, "codes, lut and ws must be 16-byte aligned");
    ARX_REQUIRE(((uintptr_t)allow | (uintptr_t)out_count) % 8 == 0, "allow and out_count must be 8-byte aligned");
    ARX_REQUIRE(((uintptr_t)out_cand | (uintptr_t)out_sum) % 4 == 0, "out_cand and out_sum must be 4-byte aligned");
    const KeyWs L = key_layout(n_rows, n_queries, R);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (arx_pq_workspace_bytes)", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    const int M = dim / dsub, QT = pq_tile(M);
    unsigned long long* part_k = (unsigned long long*)ws;
    for (int q0 = 0; q0 < n_queries; q0 += KEY_QBATCH) {
        const int nq = (n_queries - q0) < KEY_QBATCH ? (n_queries - q0) : KEY_QBATCH;
        const int tiles = (nq + QT - 1) / QT;
        int64_t parts = 0;                                     // an empty shard launches no scan: the merge of no parts writes -1 and 0
        if (n_rows > 0) {
            int64_t rpb = rows_per_block;
            if (rpb == 0) {
                const int64_t want = PQ_BLOCKS_TARGET / tiles > 0 ? PQ_BLOCKS_TARGET / tiles : 1;
                rpb = round_up64((n_rows + want - 1) / want, 256);
                if (rpb < PQ_RPB_MIN_DEFAULT) rpb = PQ_RPB_MIN_DEFAULT;
            }
            const int64_t max_parts = L.slots / nq;             // >= 1: the partial lists the workspace holds per query
            if ((n_rows + rpb - 1) / rpb > max_parts) rpb = round_up64((n_rows + max_parts - 1) / max_parts, 64);
            parts = (n_rows + rpb - 1) / rpb;
            ARX_REQUIRE(parts <= max_parts && parts < (1ll << 31), "grid too large");
            const dim3 grid((unsigned)parts, (unsigned)tiles);
            const uint8_t* T = lut + (int64_t)q0 * M * PQ_CODES;
            int32_t rc;
            switch (QT) {
                case 8: rc = pq_launch_scan_v<8>(M, grid, st, codes, n_rows, M, T, nq, allow, R, rpb, part_k); break;
                case 4: rc = pq_launch_scan_v<4>(M, grid, st, codes, n_rows, M, T, nq, allow, R, rpb, part_k); break;
                case 2: rc = pq_launch_scan_v<2>(M, grid, st, codes, n_rows, M, T, nq, allow, R, rpb, part_k); break;
                default: rc = pq_launch_scan_v<1>(M, grid, st, codes, n_rows, M, T, nq, allow, R, rpb, part_k); break;
            }
            if (rc != ARX_OK) return rc;
        }
        key_merge_kernel<true><<<nq, PQ_NT, 0, st>>>(part_k, parts, nq, R, out_cand + (int64_t)q0 * R,
                                                     out_sum ? out_sum + (int64_t)q0 * R : nullptr, out_count + q0);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}

extern "C" int32_t arx_pq_candidates(const uint8_t* codes, int64_t n_rows, int32_t dim, int32_t dsub, const uint8_t* lut, int32_t n_queries,
                                     const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_sum, int64_t* out_count,
                                     void* ws, int64_t ws_bytes, void* stream) {
    return arx_pq_candidates_tuned(codes, n_rows, dim, dsub, lut, n_queries, allow, n_candidates, out_cand, out_sum, out_count, ws, ws_bytes, 0,
                                   stream);
}
