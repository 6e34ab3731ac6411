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
//   scan    key_lists.h's key_scan_kernel (shared with binary.hip) over tiles of QT queries.  The tile's byte tables sit in LDS, M * 256
//           bytes per query, behind the tile's key lists (8 KiB per query).  A lane reads its row's M code bytes once, 16 at a time (4 or
//           1 where M is no multiple of 16), and for every byte gathers one table byte per query of the tile into that query's sum.
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
constexpr int PQ_BLOCKS_TARGET = 1024, PQ_RPB_MIN_DEFAULT = 2048, PQ_RPB_LIMIT = 1 << 20;   // key_scan's, as tests/test_gpu_pq_long.py reads them
static_assert(PQ_BLOCKS_TARGET == KEY_BLOCKS_TARGET && PQ_RPB_MIN_DEFAULT == KEY_RPB_MIN_DEFAULT && PQ_RPB_LIMIT == KEY_RPB_LIMIT, "one set");

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

// The PQ code as key_scan_kernel sees it.  V: code bytes per load (16: M % 16 == 0; 4: M % 4 == 0; 1: any M)
template <int QT_, int V>
struct PqCode {
    using Word = uint8_t;
    static constexpr int QT = QT_;
    const uint8_t* codes; int M; const uint8_t* lut;            // [n_rows][M]; the slice's [nq][M][256]
    struct Lds { KeyLists<QT>& lists; uint8_t* tab; };          // tab: [QT][M][256], behind the lists
    __device__ __forceinline__ Lds lds() const {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        return {*reinterpret_cast<KeyLists<QT>*>(smem), reinterpret_cast<uint8_t*>(smem + pq_lists_bytes<QT>())};
    }
    __device__ __forceinline__ void stage(const Lds s, int q0, int nl) const {
        const int TB = M * PQ_CODES;                            // a query's table, a multiple of 256 bytes
        for (int t = threadIdx.x; t < QT * (TB / 16); t += PQ_NT) {
            const int l = t / (TB / 16), o = t % (TB / 16);
            uint4 val = {0u, 0u, 0u, 0u};
            if (l < nl) val = reinterpret_cast<const uint4*>(lut + (int64_t)(q0 + l) * TB)[o];
            reinterpret_cast<uint4*>(s.tab)[t] = val;
        }
    }
    __device__ __forceinline__ void gather(const Lds s, const uint8_t* c, int mm, int (&sum)[QT]) const {
        const int TB = M * PQ_CODES;                            // (the V code bytes at c[mm]: a table byte per query for each)
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
            const uint8_t* t = s.tab + (mm + e) * PQ_CODES + ((xw[e >> 2] >> (8 * (e & 3))) & 255u);
#pragma unroll
            for (int l = 0; l < QT; ++l) sum[l] += t[l * TB];
        }
    }
    __device__ __forceinline__ void high_words(const Lds s, int64_t row, uint32_t (&h)[QT]) const {
        const uint8_t* c = codes + row * M;
        int sum[QT] = {};                                                                 // the sums, in registers
        if constexpr (V == 16) {                               // one 16-byte load a trip: unrolled further, <1, 16> takes 16 more VGPRs
#pragma unroll 1
            for (int mm = 0; mm < M; mm += V) gather(s, c, mm, sum);
        } else {
            for (int mm = 0; mm < M; mm += V) gather(s, c, mm, sum);
        }
#pragma unroll
        for (int l = 0; l < QT; ++l) h[l] = (uint32_t)sum[l];
    }
};

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

struct PqScan {                                                // the host side of the code, for key_scan
    static constexpr bool HI_DIRECT = true;                    // out_sum is the high word
    static constexpr const char* WORKSPACE_FN = "arx_pq_workspace_bytes";
    const uint8_t *codes, *lut; int M;
    int tile() const { return pq_tile(M); }
    int32_t launch(const KeyScanArgs& a, int q0) const {
        const uint8_t* T = lut + (int64_t)q0 * M * PQ_CODES;
        const int QT = tile(), V = M % 16 == 0 ? 16 : M % 4 == 0 ? 4 : 1;
#define PQ_SCAN(QT_, V_) /* smem <= PQ_LDS_BLOCK by pq_tile */ \
    if (QT == QT_ && V == V_) return key_scan_launch<PqCode<QT_, V_>>(a, codes, M, T, (int)pq_scan_smem<QT_>(M))
        PQ_SCAN(8, 16); PQ_SCAN(8, 4); PQ_SCAN(8, 1); PQ_SCAN(4, 16); PQ_SCAN(4, 4); PQ_SCAN(4, 1);
        PQ_SCAN(2, 16); PQ_SCAN(2, 4); PQ_SCAN(2, 1); PQ_SCAN(1, 16); PQ_SCAN(1, 4);
#undef PQ_SCAN
        return key_scan_launch<PqCode<1, 1>>(a, codes, M, T, (int)pq_scan_smem<1>(M));
    }
};
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
    KEY_REQUIRE_ROWS_PER_BLOCK(rows_per_block);
    if (n_queries == 0) return ARX_OK;
    ARX_REQUIRE(lut && out_cand && out_count && ws && (codes || n_rows == 0), "null pointer argument");
    ARX_REQUIRE(((uintptr_t)codes | (uintptr_t)lut | (uintptr_t)ws) % 16 == 0, "codes, lut and ws must be 16-byte aligned");
    ARX_REQUIRE(((uintptr_t)allow | (uintptr_t)out_count) % 8 == 0, "allow and out_count must be 8-byte aligned");
    ARX_REQUIRE(((uintptr_t)out_cand | (uintptr_t)out_sum) % 4 == 0, "out_cand and out_sum must be 4-byte aligned");
    return key_scan(PqScan{codes, lut, dim / dsub}, n_rows, n_queries, allow, R, rows_per_block, ws, ws_bytes, out_cand, out_sum, out_count,
                    (hipStream_t)stream);
}

extern "C" int32_t arx_pq_candidates(const uint8_t* codes, int64_t n_rows, int32_t dim, int32_t dsub, const uint8_t* lut, int32_t n_queries,
                                     const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_sum, int64_t* out_count,
                                     void* ws, int64_t ws_bytes, void* stream) {
    return arx_pq_candidates_tuned(codes, n_rows, dim, dsub, lut, n_queries, allow, n_candidates, out_cand, out_sum, out_count, ws, ws_bytes, 0,
                                   stream);
}
