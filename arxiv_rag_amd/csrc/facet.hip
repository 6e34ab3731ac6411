// arx_facet_count: facet counts of metadata keys under row bitmaps (C ABI in include/arx.h; the host layer is arxiv_rag_amd/facets.py).
// The consumer of what arx_where_eval, the text scans and the keep-bitmap produce: "how many allowed rows per value of this key".
//
// One launch counts every (filter, key) pair of the call: grid (row chunks, filters, keys).  A wave walks the 64-row words of its
// filter's bitmap in a grid stride, a lane owning one row of the word.  The word is wave-uniform: a zero word costs its one load and
// neither column is read for it.  For a set bit the lane reads kind[r] (1 B) and val[r] (8 B), both coalesced, and maps them to one
// counter index in [0, n_bins + 2) with a single bin function (`facet_bin`): the bin, n_bins = "missing" (another kind), n_bins + 1 =
// "unbinned" (the right kind and no bin).  Only f64 comparisons and conversions touch the values, never arithmetic.
//
// Two counting paths stand behind that function.  A key whose n_bins + 2 counters fit `lds_bins` is counted into an LDS histogram of the
// block (integer LDS atomics) and, after a barrier, every non-zero counter is added to `out` with one integer global atomic; a larger
// key adds to `out` directly.  Rows arrive in paper and section order, so the 64 rows of a word mostly share one or two bins: up to
// FC_ROUNDS times the wave takes the bin of its first remaining lane, ballots who shares it and lets that lane add the popcount; what
// is left after that adds one by one.
//
// Why the launch shape cannot change the result: every counter is a sum of integers, each (row, filter, key) triple contributes exactly
// one 1 to exactly one counter (the grid stride visits every word once, the ballot rounds partition a word's set bits), and integer
// addition is associative and commutative, so the order in which waves, blocks and atomics arrive is immaterial.  `out` is zeroed on
// the stream before the launch; nothing else is written and there is no workspace, no float atomic and no waiting between blocks.
//
// Device data that breaks the contract (a wild code, unsorted cuts) gives wrong counts but no access out of range: a CODE bin is
// range-checked before it is used, both searches keep their index inside the cuts by construction, and the counter index is clamped.
#include "arx_common.h"

namespace {
constexpr int FC_MAX_KEYS = 16, FC_MAX_FILTERS = 64, FC_MAX_BINS = 1 << 20, FC_MAX_LDS_BINS = 32768;
constexpr int FC_DEFAULT_THREADS = 256, FC_DEFAULT_LDS_BINS = 8192;
constexpr int FC_WORDS_PER_WAVE = 16;                         // default grid: a wave gets about this many words, a block at least 4 K rows
constexpr int FC_ROUNDS = 2;                                  // wave-combined adds per word before the lanes add singly
constexpr int64_t FC_MAX_OUT = (int64_t)1 << 27;

struct FacetKeys { arx_facet_key k[FC_MAX_KEYS]; };           // by value in the kernel arguments (768 B): the host array holds device pointers

// the counter of a row of kind k and value v: [0, nb) a bin, nb missing, nb + 1 unbinned
__device__ __forceinline__ int facet_bin(const arx_facet_key& K, int k, double v) {
    const int nb = K.n_bins;
    if (k != K.want_kind) return nb;
    if (K.mode == ARX_FACET_CODE) {
        if (v >= 0.0 && v < (double)nb) {                     // (a NaN fails both)
            const int i = (int)v;
            if ((double)i == v) return i;
        }
        return nb + 1;
    }
    const double* __restrict__ s = K.cuts;
    if (K.mode == ARX_FACET_EXACT) {                          // lower bound over cuts[0, nb): n is uniform, only `base` differs between lanes
        int base = 0;
        for (int n = nb; n > 1;) {
            const int half = n >> 1;
            base = (s[base + half - 1] < v) ? base + half : base;
            n -= half;
        }
        const int idx = base + ((s[base] < v) ? 1 : 0);       // in [0, nb]
        return (idx < nb && s[idx] == v) ? idx : nb + 1;      // by value: -0.0 finds 0.0, a NaN finds nothing
    }
    // ARX_FACET_INTERVAL: edges cuts[0, nb]; the edges <= v, counted by an upper bound, less one
    if (!(v >= s[0] && v <= s[nb])) return nb + 1;
    int base = 0;
    for (int n = nb + 1; n > 1;) {
        const int half = n >> 1;
        base = (s[base + half - 1] <= v) ? base + half : base;
        n -= half;
    }
    const int b = base + ((s[base] <= v) ? 1 : 0) - 1;        // in [-1, nb]; nb when v == cuts[nb]: the last bin is closed
    return b < 0 ? 0 : (b >= nb ? nb - 1 : b);
}

__global__ __launch_bounds__(1024) void facet_count_kernel(const FacetKeys keys, int64_t n_rows, int64_t n_words,
                                                            const unsigned long long* __restrict__ allow, int64_t allow_stride,
                                                            unsigned int* __restrict__ out, int64_t out_stride, int lds_bins) {
    extern __shared__ unsigned int s_hist[];
    const arx_facet_key K = keys.k[blockIdx.z];
    const int n_ctr = K.n_bins + 2;
    const bool in_lds = n_ctr <= lds_bins;                    // (block-uniform)
    const int waves = (int)(blockDim.x >> 6);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * waves;
    if (first >= n_words) return;                             // (block-uniform, before any barrier)
    unsigned int* __restrict__ mine = out + (int64_t)blockIdx.y * out_stride + K.out_off;
    if (in_lds) {
        for (int i = threadIdx.x; i < n_ctr; i += blockDim.x) s_hist[i] = 0u;
        __syncthreads();
    }
    unsigned int* dst = in_lds ? s_hist : mine;
    const unsigned long long* __restrict__ bitmap = allow ? allow + (int64_t)blockIdx.y * allow_stride : nullptr;
    const uint8_t* __restrict__ kind = K.kind;
    const double* __restrict__ val = K.val;
    const int tail = (int)(n_rows & 63);
    for (int64_t w = first + wave; w < n_words; w += (int64_t)gridDim.x * waves) {
        unsigned long long bits = bitmap ? bitmap[w] : ~0ull;
        if (w == n_words - 1 && tail) bits &= (1ull << tail) - 1ull;     // bits at or beyond n_rows are not trusted
        if (bits == 0ull) continue;                           // (wave-uniform)
        const bool active = (bits >> lane) & 1ull;
        int b = -1;
        if (active) {
            const int64_t r = w * 64 + lane;                  // < n_rows: the tail was masked
            b = facet_bin(K, (int)kind[r], val[r]);
            b = b < 0 ? 0 : (b >= n_ctr ? n_ctr - 1 : b);
        }
        unsigned long long rem = bits;
        for (int round = 0; round < FC_ROUNDS && rem; ++round) {
            const int lead = __ffsll((long long)rem) - 1;
            const int b0 = __shfl(b, lead);
            const unsigned long long same = __ballot((((rem >> lane) & 1ull) && b == b0) ? 1 : 0);
            if (lane == lead) atomicAdd(&dst[b0], (unsigned int)__popcll(same));
            rem &= ~same;
        }
        if ((rem >> lane) & 1ull) atomicAdd(&dst[b], 1u);
    }
    if (in_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_ctr; i += blockDim.x) {
            const unsigned int c = s_hist[i];
            if (c) atomicAdd(&mine[i], c);
        }
    }
}

int32_t facet_launch(const arx_facet_key* keys, int32_t n_keys, int64_t n_rows, const uint64_t* allow, int64_t allow_stride, int32_t n_filters,
                     int32_t* out, int64_t out_stride, int32_t block_threads, int32_t blocks_x, int32_t lds_bins, void* stream) {
    static_assert(sizeof(arx_facet_key) == 48, "arx_facet_key is 48 bytes (include/arx.h, _lib.FacetKeyC)");
    ARX_REQUIRE(keys, "null pointer argument: keys");
    ARX_REQUIRE(out, "null pointer argument: out");
    ARX_REQUIRE(n_keys >= 1 && n_keys <= FC_MAX_KEYS, "n_keys=%d out of range 1..%d", n_keys, FC_MAX_KEYS);
    ARX_REQUIRE(n_filters >= 1 && n_filters <= FC_MAX_FILTERS, "n_filters=%d out of range 1..%d", n_filters, FC_MAX_FILTERS);
    ARX_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows=%lld must be in 0..2^31-1", (long long)n_rows);
    ARX_REQUIRE(allow_stride >= 0, "allow_stride=%lld must not be negative", (long long)allow_stride);
    ARX_REQUIRE(out_stride >= 1 && (int64_t)n_filters * out_stride <= FC_MAX_OUT && out_stride <= FC_MAX_OUT,
                "out_stride=%lld: n_filters * out_stride must be in 1..2^27", (long long)out_stride);
    ARX_REQUIRE(block_threads >= 64 && block_threads <= 1024 && block_threads % 64 == 0,
                "block_threads=%d must be a multiple of 64 in 64..1024", block_threads);
    ARX_REQUIRE(blocks_x >= 0, "blocks_x=%d must be at least 1", blocks_x);
    ARX_REQUIRE(lds_bins >= 0 && lds_bins <= FC_MAX_LDS_BINS, "lds_bins=%d out of range 0..%d", lds_bins, FC_MAX_LDS_BINS);
    FacetKeys args;
    int lds_counters = 0;
    for (int j = 0; j < n_keys; ++j) {
        const arx_facet_key& K = keys[j];
        ARX_REQUIRE(K.mode == ARX_FACET_CODE || K.mode == ARX_FACET_EXACT || K.mode == ARX_FACET_INTERVAL, "keys[%d].mode=%d is not 0, 1 or 2", j, K.mode);
        ARX_REQUIRE(K.want_kind >= 1 && K.want_kind <= 3, "keys[%d].want_kind=%d is not 1, 2 or 3", j, K.want_kind);
        ARX_REQUIRE(K.n_bins >= 1 && K.n_bins <= FC_MAX_BINS, "keys[%d].n_bins=%d out of range 1..2^20", j, K.n_bins);
        ARX_REQUIRE(K.kind && K.val, "null pointer argument: keys[%d].%s", j, K.kind ? "val" : "kind");
        ARX_REQUIRE(K.cuts || K.mode == ARX_FACET_CODE, "null pointer argument: keys[%d].cuts (mode %d)", j, K.mode);
        ARX_REQUIRE(K.out_off >= 0 && K.out_off + K.n_bins + 2 <= out_stride, "keys[%d].out_off=%lld: its %d counters must lie inside out_stride=%lld",
                    j, (long long)K.out_off, K.n_bins + 2, (long long)out_stride);
        for (int i = 0; i < j; ++i)
            ARX_REQUIRE(K.out_off >= keys[i].out_off + keys[i].n_bins + 2 || keys[i].out_off >= K.out_off + K.n_bins + 2,
                        "keys[%d].out_off=%lld overlaps the counters of keys[%d]", j, (long long)K.out_off, i);
        args.k[j] = K;
        if (K.n_bins + 2 <= lds_bins && K.n_bins + 2 > lds_counters) lds_counters = K.n_bins + 2;
    }
    for (int j = n_keys; j < FC_MAX_KEYS; ++j) args.k[j] = keys[0];
    hipStream_t st = (hipStream_t)stream;
    ARX_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_filters * (size_t)out_stride * sizeof(int32_t), st));
    if (n_rows == 0) return ARX_OK;
    const int64_t n_words = (n_rows + 63) >> 6;
    const int waves = block_threads / 64;
    const int64_t most = (n_words + waves - 1) / waves;       // blocks beyond this have no word
    int64_t bx = blocks_x;
    if (bx == 0) {
        bx = (n_words + (int64_t)waves * FC_WORDS_PER_WAVE - 1) / ((int64_t)waves * FC_WORDS_PER_WAVE);
        const int64_t cap = 2 * (int64_t)arx_device_cus();
        if (bx > cap) bx = cap;
    }
    if (bx > most) bx = most;
    const int smem = lds_counters * (int)sizeof(unsigned int);
    if (smem > 32 * 1024) ARX_HIP_CHECK(arx_func_smem((const void*)facet_count_kernel, smem));
    const dim3 grid((unsigned)bx, (unsigned)n_filters, (unsigned)n_keys);
    facet_count_kernel<<<grid, block_threads, smem, st>>>(args, n_rows, n_words, (const unsigned long long*)allow, allow_stride,
                                                          (unsigned int*)out, out_stride, lds_bins);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
}      // namespace

extern "C" int32_t arx_facet_count(const arx_facet_key* keys, int32_t n_keys, int64_t n_rows, const uint64_t* allow, int64_t allow_stride,
                                   int32_t n_filters, int32_t* out, int64_t out_stride, void* stream) {
    return facet_launch(keys, n_keys, n_rows, allow, allow_stride, n_filters, out, out_stride, FC_DEFAULT_THREADS, 0, FC_DEFAULT_LDS_BINS, stream);
}

extern "C" int32_t arx_facet_count_tuned(const arx_facet_key* keys, int32_t n_keys, int64_t n_rows, const uint64_t* allow, int64_t allow_stride,
                                         int32_t n_filters, int32_t* out, int64_t out_stride, int32_t block_threads, int32_t blocks_x,
                                         int32_t lds_bins, void* stream) {
    ARX_REQUIRE(blocks_x >= 1, "blocks_x=%d must be at least 1", blocks_x);
    return facet_launch(keys, n_keys, n_rows, allow, allow_stride, n_filters, out, out_stride, block_threads, blocks_x, lds_bins, stream);
}
