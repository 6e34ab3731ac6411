/*
 * arx.h — C ABI of the MI355X-native embed + retrieve hot path (libarx_hip.so).
 *
 * This is the replacement surface for the arithmetic the reference reaches through
 * `SentenceTransformer.encode(...)`
 *   /root/reference/4-embed/generation/generate_embeddings_parallel.py:146-153 (batch encode)
 *   /root/reference/4-embed/generation/generate_embeddings_parallel.py:160-165 (per-item retry)
 *   /root/reference/3-chunks/pipeline/src/processors/text_processor.py:1383-1396 (semantic chunker)
 * plus the cosine top-k step the reference configures but never implements
 *   /root/reference/3-chunks/pipeline/config.yaml:63-64 (`retrieval.top_k: 10`)
 *   /root/reference/3-chunks/pipeline/src/processors/text_processor.py:1601-1605 (cosine helper).
 * The reference has no FFI of its own (it is pure Python); INTEGRATION.md shows the ctypes stub a
 * maintainer would add at those call sites.
 *
 * Conventions
 *   - plain C types only; every pointer marked "device" is a HIP device pointer owned by the CALLER
 *     (e.g. a PyTorch-ROCm tensor's data_ptr); the library never allocates outputs.
 *   - an opaque handle owns only its private workspace (create/destroy).
 *   - every launch goes on the caller's hipStream_t (passed as void*); no hidden synchronisation.
 *   - return 0 on success, negative on error; arx_last_error() gives the thread-local message.
 *   - one host thread per handle.  The library keeps NO process-wide policy and reads no environment variable: what a search does is
 *     in its arguments (arx_topk_options) and its workspace, what an encoder handle runs is fixed by the arguments of its create call
 *     (arx_encoder_options), so different host threads may search different (or the same) shards at once, each with its own workspace
 *     and stream.  The only process-wide state in the library is the opt-in arx_prof_* timing facility.  (A -DARX_DEV_VARIANTS build
 *     additionally reads a few ARX_DEV_* / ARX_STAMP_* measurement switches.)
 */
#ifndef ARX_H
#define ARX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARX_VERSION 112            /* 0.1.1: search policy per call (arx_topk_options), no process-wide search state; 111: the int8 index is centred (layout + 4 dim bytes);
                                      112: encoder schedules per handle (arx_encoder_options), no environment variable is read */

#define ARX_OK            0
#define ARX_ERR_ARG      -1        /* bad argument / unsupported shape */
#define ARX_ERR_HIP      -2        /* HIP runtime error */
#define ARX_ERR_CAPACITY -3        /* batch exceeds the handle's workspace */

#define ARX_ARCH_MPNET 0           /* relative-position bias, pad-aware position ids */
#define ARX_ARCH_BERT  1           /* absolute positions + token type 0 */
#define ARX_POOL_MEAN  0
#define ARX_POOL_CLS   1

typedef struct {
    int32_t arch;                  /* ARX_ARCH_* */
    int32_t vocab_size;
    int32_t hidden;                /* H: multiple of 64 */
    int32_t layers;
    int32_t heads;                 /* H / heads must be 32 or 64 */
    int32_t ffn;                   /* F: multiple of 64 */
    int32_t max_pos;               /* rows of the position table */
    int32_t pool;                  /* ARX_POOL_* */
    int32_t pad_id;                /* MPNet 1, BERT 0 */
    int32_t rel_buckets;           /* MPNet: 32 */
    int32_t rel_max_distance;      /* MPNet: 128 */
    float   ln_eps;
} arx_encoder_config;

/* All weight pointers: device memory, caller-owned, must outlive the handle.
 * Matrices are nn.Linear layout [out, in] row-major, bf16 (uint16 storage).  Vectors are f32. */
typedef struct {
    const void*  w_qkv;            /* [3H, H] bf16: rows 0..H-1 = q, H..2H-1 = k, 2H..3H-1 = v */
    const float* b_qkv;            /* [3H] */
    const void*  w_o;              /* [H, H] bf16 */
    const float* b_o;              /* [H] */
    const float* ln1_g; const float* ln1_b;   /* attention output LayerNorm [H] */
    const void*  w_fc1;            /* [F, H] bf16 */
    const float* b_fc1;            /* [F] */
    const void*  w_fc2;            /* [H, F] bf16 */
    const float* b_fc2;            /* [H] */
    const float* ln2_g; const float* ln2_b;   /* output LayerNorm [H] */
} arx_layer_weights;

typedef struct {
    const float* word_emb;         /* [vocab, H] f32 */
    const float* pos_emb;          /* [max_pos, H] f32 */
    const float* type_emb;         /* [H] f32: BERT token_type row 0; NULL for MPNet */
    const float* emb_ln_g; const float* emb_ln_b;   /* [H] */
    const float* rel_bias;         /* [rel_buckets, heads] f32 (HF encoder.relative_attention_bias.weight); NULL for BERT */
    const arx_layer_weights* layers;   /* host array of `layers` entries */
} arx_encoder_weights;

typedef struct arx_encoder arx_encoder;

int32_t     arx_version(void);
const char* arx_last_error(void);

/* MPNet relative-position bucket of (key_pos - query_pos) — host function, exported so the table
 * the kernels consume can be checked against the golden vectors without a GPU. */
int32_t arx_mpnet_bucket(int32_t relative_position, int32_t num_buckets, int32_t max_distance);

/* Workspace bytes a handle for (cfg, max_tokens, max_seqs) allocates. */
int64_t arx_encoder_workspace_bytes(const arx_encoder_config* cfg, int32_t max_tokens, int32_t max_seqs);

/* Build a handle: validates shapes, allocates the private workspace (activations for up to
 * max_tokens packed tokens / max_seqs sequences), precomputes the relative-position table. */
int32_t arx_encoder_create(const arx_encoder_config* cfg, const arx_encoder_weights* w,
                           int32_t max_tokens, int32_t max_seqs, arx_encoder** out);
void    arx_encoder_destroy(arx_encoder* h);

/* Which kernels a handle runs, fixed for its life at create (round <= 4: environment variables).  Zero-initialise, set struct_bytes =
 * sizeof(arx_encoder_options), fill what differs from the defaults.  The schedules agree to rounding, not bit for bit. */
/* GEMM main-loop schedules: gemm_schedule here, `variant` of arx_gemm_bf16 and of arx_gemm_epilogue; dispatch in csrc/encoder.hip */
#define ARX_GEMM_DEFAULT    89     /* the persistent 4-phase kernel for K <= 1024, the per-tile 4-phase kernel above */
#define ARX_GEMM_PER_TILE    8     /* 4-phase kernel, one 256 x 256 tile per block, wherever it applies */
#define ARX_GEMM_PERSISTENT  9     /* 4-phase kernel, one block per CU walking the tiles, wherever it applies */
#define ARX_GEMM_2STAGE     13     /* 2-stage loop, 64-bit offsets, any N % 8 == 0: what the 4-phase kernels fall back to */
#define ARX_GEMM_SPLIT_K    70     /* split-K wave tiles for <= 256 rows; in a handle only through arx_encoder_set_low_latency */
#define ARX_GEMM_TILE_128   71     /* 2-stage loop on 128 x 128 tiles: the medium-batch half of arx_encoder_set_low_latency */
/* (a -DARX_DEV_VARIANTS build also holds the round-1 A/B schedules 1, 2, 3, 4, 15, 33, 34 of DESIGN.md's negative-result tables) */
#define ARX_ATTN_TRANSPOSED  1     /* default: the transposing-read kernel, 4-wave blocks up to 128 tokens and 8-wave blocks above */
#define ARX_ATTN_RING        2     /* -DARX_DEV_VARIANTS builds only: the streaming ring kernel, batches of 129..256 tokens */
#define ARX_ATTN_RING16      4     /* -DARX_DEV_VARIANTS builds only: the 16-wave ring kernel, head dim 64, batches of 129..256 tokens */
#define ARX_ATTN_STAGED      8     /* the first kernel: V transposed while it is staged into LDS, a running maximum in every tile */
#define ARX_ENC_EXPLICIT_LAYERNORM 1   /* flags: the two-pass LayerNorm kernels between the GEMMs instead of the LayerNorm-fold epilogues */
typedef struct {
    int32_t struct_bytes;          /* sizeof(arx_encoder_options) */
    int32_t gemm_schedule;         /* 0 = ARX_GEMM_DEFAULT; else ARX_GEMM_PER_TILE, _PERSISTENT, _2STAGE or _TILE_128 (or a dev schedule) */
    int32_t attn_kernel;           /* 0 = ARX_ATTN_TRANSPOSED; else an ARX_ATTN_* id */
    int32_t flags;                 /* ARX_ENC_* */
} arx_encoder_options;
/* arx_encoder_create with an explicit choice; opt == NULL = defaults (what arx_encoder_create passes).  A wrong struct_bytes, an id this
 * build does not contain or an unknown flag is ARX_ERR_ARG naming the field and its value: nothing is allocated, *out is not written. */
int32_t arx_encoder_create_opt(const arx_encoder_config* cfg, const arx_encoder_weights* w, int32_t max_tokens, int32_t max_seqs,
                               const arx_encoder_options* opt, arx_encoder** out);

/* Encode one batch of token sequences -> unit-norm sentence embeddings.
 *   ids   device int32 [n_seqs, seq_stride]: right-padded token ids (pad beyond lens[i] is ignored)
 *   lens  device int32 [n_seqs]: valid tokens per row (0 <= lens[i] <= max_len <= 512)
 *   total_tokens  host-side upper bound on sum(lens) (exact sum is best; n_seqs*max_len always valid)
 *   out_f32  device float  [n_seqs, out_stride] or NULL
 *   out_f16  device fp16   [n_seqs, out16_stride] or NULL   (corpus-shard row, written in place)
 *   normalize  1: x / max(||x||, 1e-12)   0: raw pooled vector
 * Semantics = SentenceTransformer.encode(..., normalize_embeddings=True) on the same token ids:
 * encoder forward, masked mean (or CLS) pool, L2 normalise.  Rows with lens[i] == 0 give zeros. */
int32_t arx_encoder_forward(arx_encoder* h, const int32_t* ids, int32_t seq_stride,
                            const int32_t* lens, int32_t n_seqs, int32_t max_len, int32_t total_tokens,
                            float* out_f32, int64_t out_stride,
                            void* out_f16, int64_t out16_stride,
                            int32_t normalize, void* stream);

/* The fused attention block alone, on caller-provided packed qkv [sum(lens), 3H] bf16 -> ctx [sum(lens), H] bf16
 * (parity tap: lets a test drive the online-softmax rescale path with crafted scores). */
int32_t arx_encoder_attention(arx_encoder* h, const void* qkv, const int32_t* lens, int32_t n_seqs, int32_t max_len,
                              void* ctx, void* stream);

/* Debug / parity tap: copy the packed hidden state after `layer` (0 = embeddings, L = last) as f32
 * [total_tokens, H] into dst (device).  Valid after a forward on the same stream. */
int32_t arx_encoder_debug_hidden(arx_encoder* h, int32_t layer_slot, float* dst, int32_t n_tokens, void* stream);

/* Opt-in small-batch schedule for QUERY batches (no reference counterpart: the reference encodes its queries with the same
 * `model.encode` as the corpus, GEN:146-153).  With on != 0, a forward of at most 256 packed token rows runs its linear layers as
 * split-K wave tiles (csrc/gemm_small.h: every CU takes part and each weight byte is read once) instead of 256 x 256 tiles that
 * leave all but a few CUs idle; forwards of up to 8 192 rows take 128 x 128 tiles; longer forwards are unaffected.  Rows agree with the default schedule to rounding (another
 * summation order), not bit for bit: leave it off for corpus rows if their bits must not depend on the batch they were in.
 * Allocates the handle's 64-MiB partial-sum workspace on first use (freed by arx_encoder_destroy). */
int32_t arx_encoder_set_low_latency(arx_encoder* h, int32_t on);

/* Ask the next forward() to snapshot the hidden state after `layer` (-1 = off). */
int32_t arx_encoder_set_tap(arx_encoder* h, int32_t layer);

/* ---- cross-encoder reranking (BertForSequenceClassification, e.g. cross-encoder/ms-marco-MiniLM-L-6-v2) ----------------------
 * logits = W_c tanh(W_p h + b_p) + b_c on the final CLS row h of "[CLS] A [SEP] B [SEP]", segment B with token type 1.
 * All pointers: device memory, caller-owned, f32, must outlive the handle. */
typedef struct {
    int32_t struct_bytes;          /* sizeof(arx_pair_head) */
    int32_t n_labels;              /* 1..16 */
    const float* type_emb;         /* [2, H] token-type table (row 0 should be the handle's arx_encoder_weights.type_emb) */
    const float* pooler_w; const float* pooler_b;   /* [H, H], [H] (bert.pooler.dense) */
    const float* cls_w;    const float* cls_b;      /* [n_labels, H], [n_labels] (classifier) */
} arx_pair_head;

/* Attach a pair head to a BERT handle with CLS pooling (else ARX_ERR_ARG).  Allocates the handle's [max_seqs, H] f32 CLS scratch on
 * first use (freed by arx_encoder_destroy); arx_encoder_workspace_bytes does not count it. */
int32_t arx_encoder_set_pair_head(arx_encoder* h, const arx_pair_head* head);
/* Score sentence pairs: arguments as arx_encoder_forward, plus seg_b device int32 [n_seqs] (first token of segment B; any value is
 * valid: seg_b[i] >= lens[i] = all type 0; NULL = all type 0) -> out_logits device f32 [n_seqs, out_stride >= n_labels].
 * A pair's logits are bitwise independent of the other pairs of the call (unless arx_encoder_set_low_latency is on).  The tap of
 * arx_encoder_set_tap works across this call as across a forward. */
int32_t arx_encoder_score_pairs(arx_encoder* h, const int32_t* ids, int32_t seq_stride, const int32_t* lens, const int32_t* seg_b,
                                int32_t n_seqs, int32_t max_len, int32_t total_tokens, float* out_logits, int64_t out_stride,
                                void* stream);
/* Parity tap: copy the f32 CLS rows [n, H] the head read in the last arx_encoder_score_pairs call into dst (device; same stream). */
int32_t arx_encoder_debug_cls(arx_encoder* h, float* dst, int32_t n, void* stream);
/* The head alone on caller-provided CLS rows f32 [n, ld >= hidden] (parity tap); hidden <= 1024; head->type_emb is not read. */
int32_t arx_pair_head_forward(const float* cls_rows, int64_t ld, int32_t n, int32_t hidden, const arx_pair_head* head,
                              float* out_logits, int64_t out_stride, void* stream);

/* Build flags of the loaded library: bit 0 = built with -DARX_DEV_VARIANTS (the A/B schedules of DESIGN.md's negative-result
 * tables are compiled in and arx_encoder_options accepts their ids); 0 for the shipped build. */
int32_t arx_build_info(void);

/* ---- brute-force cosine top-k over an HBM-resident fp16 shard ------------------------------------
 *   corpus  device fp16 [n_rows, dim] row-major, dim % 64 == 0.  Scores are DOT PRODUCTS (cosine when rows and queries are unit
 *           vectors, as the encoder writes them); the answer is the exact top-k of those for rows of ANY norm, provided
 *           arx_topk_options.max_row_norm bounds the rows' L2 norms (default: unit rows; arx_rows_max_norm_f16 measures it).
 *   queries device fp16 [n_queries, dim]
 *   out_scores device f32 [n_queries, k]; out_ids device int64 [n_queries, k] = local row + idx_base
 *   order: score descending, ties -> lower row index; if k > n_rows the tail is (-inf, -1)
 *   ws: device workspace of arx_topk_workspace_bytes(...) bytes, caller-owned.  k <= 32. */
int64_t arx_topk_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k);
int32_t arx_topk_search(const void* corpus, int64_t n_rows, const void* queries, int32_t n_queries,
                        int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                        void* ws, int64_t ws_bytes, void* stream);

/* Optional int8 PRE-FILTER (no reference counterpart; same exact answers, fewer bytes).  arx_topk_build_i8 writes a second, int8
 * representation of the shard (int8 values of the rows MINUS a vector mu the build samples from them — their mean, so that rows sharing a large
 * common component are told apart by what distinguishes them —, row-wise scale, the row's L1 norm, mu: dim + 8 bytes per row + 4 dim, caller-owned device buffer of
 * arx_topk_i8_index_bytes(...) bytes); arx_topk_search_i8 then runs its first pass over THAT — half the bytes where the pass is
 * HBM-bound, twice the MFMA rate where it is matrix-bound — computing for every (query, 64-row group) a rigorous UPPER BOUND on the
 * true fp16 score of the group's rows (quantisation error bounded analytically, csrc/search_pass_a.h).  Selection, the fp32 rescoring
 * of the fp16 rows and the exactness certificate are those of arx_topk_search, so out_scores / out_ids are the same exact top-k
 * (the certificate's exhaustive-by-threshold step absorbs the bound's slack: a few hundred 64-row groups per query on unit rows).
 * dim % 128 == 0, dim <= 1024.  `corpus` is still needed (the rescoring reads it).  The int8 pass needs the LARGER workspace of
 * arx_topk_workspace_bytes_i8 (candidate lists, a second word per (query, group)); the fp16 pass does not pay for it. */
int64_t arx_topk_i8_index_bytes(int64_t n_rows, int32_t dim);
int64_t arx_topk_workspace_bytes_i8(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k);
int32_t arx_topk_build_i8(const void* corpus, int64_t n_rows, int32_t dim, void* index_i8, void* stream);
/* {|mu|, max |t_c|, max sum |c'_i m^_i|} of a built index -> host_out[3] (synchronises the stream): |mu| is what a caller needs to decide on
 * ARX_TOPK_I8_CENTRE_QUERY. */
int32_t arx_topk_i8_index_info(const void* index_i8, int64_t n_rows, int32_t dim, float* host_out, void* stream);
int32_t arx_topk_search_i8(const void* corpus, const void* index_i8, int64_t n_rows, const void* queries, int32_t n_queries,
                           int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                           void* ws, int64_t ws_bytes, void* stream);

/* Per-CALL policy of a search (nothing here is remembered by the library: two indices with different policies can be searched from two
 * host threads at once).  Zero-initialise, set struct_bytes = sizeof(arx_topk_options), fill what differs from the defaults. */
#define ARX_TOPK_NO_PERSISTENT 1   /* flags: take the per-tile pass-A kernel even where the persistent one applies (A/B measurements) */
#define ARX_TOPK_NO_SINGLE_ROW_TAIL 8 /* flags: take the select + rescore kernel pair (all 64 rows of each selected group) where the library would take the
                                      single-kernel tail that rescoring only the arg-max 4-row block (fp16 pass: batches of <= 256 queries, k <= 10, shards
                                      of <= 1 M rows) or the arg-max row (int8 pipeline's first step) of each selected group — A/B measurements, tests */
#define ARX_TOPK_I8_CENTRE_QUERY 16 /* flags (int8 pass): quantise the QUERY minus its component along the index's mean direction as well, the rank-one term
                                      that leaves added exactly in pass A (one more instruction per value of its epilogue).  For indexes whose rows share a large
                                      common component (arx_topk_i8_index_info: |mu|^2 = the mean pairwise cosine of unit rows); same exact answers either way */
#define ARX_TOPK_SCAN_ONLY     2   /* flags: run only pass A (the scan of the shard: every CU, HBM-bound) and leave its result in the workspace */
#define ARX_TOPK_TAIL_ONLY     4   /* flags: run only what follows pass A (select, exact rescoring, certificate) on a workspace a SCAN_ONLY call
                                      with the same arguments filled; the caller orders the two calls (possibly on two streams with different
                                      CU masks: the pipelined search).  Split calls take at most 1 024 queries. */
typedef struct {
    int32_t struct_bytes;          /* sizeof(arx_topk_options) of the caller's header */
    int32_t i8_max_queries;        /* with an int8 index: internal query batches of more than this many queries take the fp16 first pass;
                                      0 = library default (every batch size: the measured crossover), negative = never int8 */
    float   max_row_norm;          /* upper bound on the L2 norm of every corpus row; 0 = unit rows (<= 1 + 2^-9, what the encoder
                                      writes).  The exactness certificate's rounding tolerance scales with it: a bound that is too
                                      SMALL voids the proof (answers could then differ among ~1e-5-level near-ties), too large only
                                      sends more queries through the slow path.  arx_rows_max_norm_f16 computes it. */
    int32_t cu_limit;              /* compute units the launch stream may use (a stream created with a CU mask); 0 = the whole device.
                                      Sizes the persistent pass-A grid (one block per CU). */
    int32_t flags;                 /* ARX_TOPK_* */
    float   debug_tau_mult;        /* TEST HOOK: multiplies the certificate tolerance; 0 = 1; values in (0, 1) would SHRINK the tolerance
                                      and void the guarantee, so they are refused (1e9 = every group rescored: an exhaustive exact scan) */
    int32_t debug_drop_best;       /* TEST HOOK: the selection forgets its best group, as a rounding accident at the boundary would;
                                      the certificate must recover it */
} arx_topk_options;
/* arx_topk_search (index_i8 == NULL) / arx_topk_search_i8 with an explicit policy; opt == NULL = defaults. */
int32_t arx_topk_search_opt(const void* corpus, const void* index_i8, int64_t n_rows, const void* queries, int32_t n_queries,
                            int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                            void* ws, int64_t ws_bytes, const arx_topk_options* opt, void* stream);

/* max over rows of the L2 norm of fp16 rows [n_rows, dim] -> *out_max (ONE device float, written by the kernels on `stream`; fp32
 * accumulation, rounded up).  What arx_topk_options.max_row_norm wants for a shard that was not written by the encoder (rows loaded
 * from a user's .npy).  A non-finite row gives +inf/NaN: refuse to index such a shard. */
int32_t arx_rows_max_norm_f16(const void* rows, int64_t n_rows, int32_t dim, float* out_max, void* stream);

/* Exactness certificate of the LAST arx_topk_search on this workspace (csrc/search_tail.h, rescore_kernel step 5): the number of
 * queries whose first selection could not be certified (an unscored 64-row group reached the k-th exact score minus the
 * rounding tolerance) and the number of extra groups that were then rescored for them.  Every answer is exact either way; the
 * counters say how often the slow path ran (near-duplicate chunks).  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_topk_stats(const void* ws, int64_t* flagged_queries, int64_t* extra_groups, void* stream);

/* A HIP stream restricted to a subset of the compute units (hipExtStreamCreateWithCUMask): bit i of cu_mask = CU i in the driver's
 * enumeration, which deals consecutive bits round-robin to the 8 XCDs — a contiguous run of 8 n bits is n CUs on every XCD.  The
 * pipelined search (ShardIndex.search_many) runs pass A of batch b + 1 on most CUs and the select / rescore / merge tail of batch b on a
 * few, so that the tail's whole-CU blocks never wait for pass-A blocks to drain.  *out is a hipStream_t. */
int32_t arx_stream_create_cu_mask(const uint32_t* cu_mask, int32_t n_words, void** out);
int32_t arx_stream_destroy(void* stream);
/* compute units of the current device */
int32_t arx_device_cu_count(void);
/* Debug: out[b] (device uint32 [n_blocks]) = (XCC_ID << 16) | (HW_ID & 0xffff) of the CU that ran block b of a grid of one-wave blocks that
 * each idle for spin_cycles — which compute units the stream's queue really uses (HW_ID: bits 8-11 CU, 12 shader array, 13-15 engine). */
int32_t arx_debug_cu_census(uint32_t* out, int32_t n_blocks, int32_t spin_cycles, void* stream);

/* Merge P partial top-k lists (e.g. the all-gathered per-shard results) into the global top-k.
 *   scores f32 [P, n_queries, k], ids int64 [P, n_queries, k] (device) -> out [n_queries, k]. */
int32_t arx_topk_merge(const float* scores, const int64_t* ids, int32_t n_parts, int32_t n_queries,
                       int32_t k, float* out_scores, int64_t* out_ids, void* stream);

/* ---- Filtered exact top-k (Chroma's `where`): arx_topk_search over the sub-corpus of ALLOWED rows ------------------------------
 * allow: device uint64 [ceil(n_rows / 64)], bit (r & 63) of word (r >> 6) set = row r may be returned; bits at or beyond n_rows are
 * ignored.  One filter per call, shared by its queries.  Semantics exactly those of arx_topk_search over the allowed rows with ids of
 * the ORIGINAL rows (idx_base + r): score descending, ties to the lower row, (-inf, -1) padding when fewer than k rows are allowed.
 * n_allowed: the number of set bits below n_rows if the caller knows it, -1 if not.  max_row_norm: what arx_topk_options.max_row_norm is, 0 = unit
 * rows.  dim % 64 == 0, k <= 32, any n_queries.  Two device paths with the same bits (csrc/filter.hip): the masked scan (pass A with
 * the filter in front of the group maximum; tiles without an allowed row are not read) and the exhaustive scoring of the compacted
 * list of allowed rows, which the library takes by itself for small n_allowed * n_queries and for any query whose candidate list
 * overflows.  ws: device workspace of arx_topk_filtered_workspace_bytes(...) bytes, caller-owned. */
int64_t arx_topk_filtered_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k);
int32_t arx_topk_search_filtered(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                 int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                                 float max_row_norm, void* ws, int64_t ws_bytes, void* stream);
/* The same with the path and the candidate capacity chosen by the caller (tests, tuning): path 0 = library's choice, 1 = masked scan,
 * 2 = exhaustive over the allowed rows; cand_cap = candidate groups a query may list before it goes to the exhaustive path (0 =
 * default, at most 8192).  Same bits for every choice. */
int32_t arx_topk_search_filtered_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                                       int32_t n_queries, int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                                       float max_row_norm, void* ws, int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream);
/* {queries sent to the exhaustive path because their candidate list overflowed, candidate groups rescored} of the LAST filtered
 * search on this workspace.  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_topk_filtered_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream);

/* ---- Filtered exact top-k with a different filter per query in one call (csrc/filter_multi.hip) ---------------------------------------
 * allow: device uint64 [n_filters][ceil(n_rows / 64)], each row a bitmap in the convention of arx_topk_search_filtered (bits at or
 * beyond n_rows are ignored and may be garbage); 1 <= n_filters <= 64.  filter_of: device int32 [n_queries]; query q may return only
 * the rows of allow[filter_of[q]].  A filter_of[q] outside [0, n_filters) means query q sees no row: its output is all (-inf, -1), and
 * nothing is read out of range (the kernels test the index; the host never sees it).  n_allowed: HOST int64 [n_filters], the number of
 * set bits below n_rows of each bitmap, -1 where unknown, or NULL = all unknown; it only steers path 0.
 * Query q's scores and ids are those of arx_topk_search_filtered called with that query alone and allow[filter_of[q]], bit for bit: a
 * query's output depends on the query, its own bitmap and the corpus alone - not on the other queries, their filters, the order of the
 * batch, n_filters, the path or cand_cap.  The shard is read once per call, not once per filter: a 256-row tile is skipped only when
 * no filter used by the block's 64 / 128 / 256 queries has a bit in it.  max_row_norm, dim % 64 == 0, k <= 32, any n_queries (sliced
 * above 1 024), output conventions and the two device paths as for arx_topk_search_filtered; the exhaustive path computes a query's row
 * list from per-filter popcount offsets instead of storing it, and path 0 takes it only when every n_allowed[f] is given and
 * max_f n_allowed[f] * n_queries < 2^18.  n_filters outside 1..64 or a null pointer: ARX_ERR_ARG before any launch.
 * ws: device workspace of arx_topk_filtered_multi_workspace_bytes(...) bytes, caller-owned; with qb = min(n_queries, 1 024), ldg = qb
 * rounded up to 64, G = ceil(n_rows / 64) and P = min(ceil(n_rows / 256), 128) it is the sum, each term rounded up to 256 bytes, of
 * 64 + 4 G ldg + (4 ldg + 12 ldg / 64) + 8 * 64 (G + 1) + 4 qb + 4 P qb k + 8 P qb k: the offsets are laid out for 64 filters
 * whatever n_filters is (n_filters outside 1..64 returns -1). */
int64_t arx_topk_filtered_multi_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n_filters, int32_t dim, int32_t k);
int32_t arx_topk_search_filtered_multi(const void* corpus, int64_t n_rows, const uint64_t* allow, int32_t n_filters,
                                       const int64_t* n_allowed, const int32_t* filter_of, const void* queries, int32_t n_queries,
                                       int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm,
                                       void* ws, int64_t ws_bytes, void* stream);
/* The same with the path and the candidate capacity chosen by the caller (tests, tuning), as arx_topk_search_filtered_tuned.  Same
 * bits for every choice. */
int32_t arx_topk_search_filtered_multi_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int32_t n_filters,
                                             const int64_t* n_allowed, const int32_t* filter_of, const void* queries, int32_t n_queries,
                                             int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base,
                                             float max_row_norm, void* ws, int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream);
/* {queries sent to the exhaustive path because their candidate list overflowed, candidate groups rescored} of the LAST multi-filter
 * search on this workspace.  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_topk_filtered_multi_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream);

/* ---- Exact top-k with a row limit per query (the self-join of near-duplicate detection) ----------------------------------------------
 * row_limit: device int64 [n_queries]; query q may return only the local rows r < row_limit[q] (clamped to [0, n_rows]).  The answer is
 * the exact top-k of those rows, score descending, ties to the lower row, ids = local row + idx_base, (-inf, -1) padding when fewer than
 * k rows lie below the limit (limit 0 included).  A (query, row) score has the bits it has in arx_topk_search and
 * arx_topk_search_filtered.  `queries` may point into `corpus` itself: with row_limit[q] = the query's own row number that is "the
 * nearest earlier rows of every row".  A query's output depends on the query, its limit and the corpus alone — not on the batch, the
 * other limits, the path or cand_cap.  max_row_norm as for the filtered search, 0 = unit rows.  dim % 64 == 0, k <= 32, any n_queries
 * (batches above 1 024 queries are processed in slices).  Two device paths with the same bits (csrc/prefix.hip): the masked scan (pass A
 * with `row < limit` in front of the group maximum; tiles at or beyond the largest limit of a query tile are not read) and the
 * exhaustive scoring of rows [0, limit), which also answers any query whose candidate list overflows.
 * ws: device workspace of arx_topk_prefix_workspace_bytes(...) bytes, caller-owned. */
int64_t arx_topk_prefix_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k);
int32_t arx_topk_search_prefix(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit, int32_t n_queries,
                               int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm,
                               void* ws, int64_t ws_bytes, void* stream);
/* The same with the path and the candidate capacity chosen by the caller (tests, tuning): path 0 = library's choice, 1 = masked scan,
 * 2 = exhaustive; cand_cap = candidate groups a query may list before it goes to the exhaustive path (0 = default 1 024, at most
 * 8192).  Same bits for every choice. */
int32_t arx_topk_search_prefix_tuned(const void* corpus, int64_t n_rows, const void* queries, const int64_t* row_limit, int32_t n_queries,
                                     int32_t dim, int32_t k, float* out_scores, int64_t* out_ids, int64_t idx_base, float max_row_norm,
                                     void* ws, int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream);
/* {queries sent to the exhaustive path because their candidate list overflowed, candidate groups rescored} of the LAST prefix search
 * on this workspace.  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_topk_prefix_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream);

/* ---- Grouped exact search: the top papers with their best chunks (field collapsing; csrc/grouped.hip) --------------------------------
 * group_of: device int32 [n_rows], non-decreasing and non-negative, not necessarily dense: a group (a paper) is a contiguous run of
 * rows.  allow: a row bitmap in the convention of arx_topk_search_filtered, NULL = every row; n_allowed as there (-1 = unknown).
 * For query q, score(q, r) has the bits it has in arx_topk_search and arx_topk_search_filtered.  A group's score is the maximum of
 * score(q, r) over its visible rows; a group with no visible row does not exist for the query.  The answer is the n_groups best groups
 * by (group score desc, row of the best chunk asc) and, for each, its chunks_per_group best visible chunks by (score desc, row asc): the
 * first chunk is the one that gave the group its score.
 *   out_scores f32 [n_queries, n_groups, chunks_per_group], out_ids int64 (same shape) = idx_base + row,
 *   out_groups int32 [n_queries, n_groups] = the group_of value;
 * padding (-inf, -1) for chunks and -1 for groups when fewer than n_groups groups are visible or a group has fewer than
 * chunks_per_group visible rows.  1 <= n_groups <= 32, 1 <= chunks_per_group <= 8, dim % 64 == 0, any n_queries (sliced above 1 024).
 * max_run_rows: an upper bound on the rows of any run, the caller's contract as max_row_norm is (arx_group_runs_info measures it): too
 * small voids the exactness proof, too large only raises K = n_groups * (floor((max_run_rows + 62) / 64) + 1), the number of 64-row
 * group maxima the scan selects among (the proof is in csrc/grouped.hip).  K > 512: the whole call takes the exhaustive path.
 * A query's output depends on the query, the mask, group_of and the corpus alone - not on the batch, its order, the path or cand_cap.
 * A null pointer, n_groups or chunks_per_group out of range, max_run_rows < 1 or dim % 64 != 0: ARX_ERR_ARG before any launch, the
 * message naming the field and its value.
 * ws: device workspace of arx_topk_grouped_workspace_bytes(...) bytes, caller-owned; with qb = min(n_queries, 1 024), ldg = qb rounded
 * up to 64, G = ceil(n_rows / 64), P = n_groups and T = min(ceil(n_rows / 256), 128) it is the sum, each term rounded up to 256 bytes,
 * of 64 + 4 G ldg + 8 G + 4 qb + 4 qb P + 8 qb P + 4 T qb P + 8 T qb P (chunks_per_group does not enter; -1 for an unsupported
 * shape: n_rows outside 1 .. 2^36 - 1, n_queries < 1, dim not a multiple of 64 in 64 .. 8192, n_groups or chunks_per_group out of
 * range). */
int64_t arx_topk_grouped_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t n_groups, int32_t chunks_per_group);
int32_t arx_topk_search_grouped(const void* corpus, int64_t n_rows, const int32_t* group_of, int64_t max_run_rows, const uint64_t* allow,
                                int64_t n_allowed, const void* queries, int32_t n_queries, int32_t dim, int32_t n_groups,
                                int32_t chunks_per_group, float* out_scores, int64_t* out_ids, int32_t* out_groups, int64_t idx_base,
                                float max_row_norm, void* ws, int64_t ws_bytes, void* stream);
/* The same with the path and the candidate capacity chosen by the caller (tests, tuning): path 0 = library's choice, 1 = the scan,
 * 2 = exhaustive over the visible rows; cand_cap = candidate groups a query may list before it goes to the exhaustive path (0 =
 * default 1 024, at most 8192).  Same bits for every choice. */
int32_t arx_topk_search_grouped_tuned(const void* corpus, int64_t n_rows, const int32_t* group_of, int64_t max_run_rows,
                                      const uint64_t* allow, int64_t n_allowed, const void* queries, int32_t n_queries, int32_t dim,
                                      int32_t n_groups, int32_t chunks_per_group, float* out_scores, int64_t* out_ids, int32_t* out_groups,
                                      int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, int32_t path, int32_t cand_cap,
                                      void* stream);
/* {queries sent to the exhaustive path because their candidate list overflowed, candidate groups rescored} of the LAST grouped search
 * on this workspace.  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_topk_grouped_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream);
/* out (device int64 [2], written by the kernels on `stream`) = {rows of the longest run of group_of, number of runs}; the longest run is
 * -1 when group_of decreases somewhere or holds a negative value.  What max_run_rows wants, as arx_rows_max_norm_f16 is what
 * max_row_norm wants. */
int32_t arx_group_runs_info(const int32_t* group_of, int64_t n_rows, int64_t* out, void* stream);

/* ---- Boosted exact search: top-k of cosine plus a weighted row prior (score boosting, a rank profile; csrc/boosted.hip) ---------------
 * prior: device f32 [n_rows], 16-byte aligned, one value per row.  weight: device f32 [n_queries], one per query.  allow: a row bitmap
 * in the convention of arx_topk_search_filtered, NULL = every row; n_allowed as there (-1 = unknown).
 * Row r is visible to query q when its bit is set (or allow is NULL) and p(q, r) = fl32(weight[q] * prior[r]) is finite: a NaN or +-inf
 * prior hides the row from every query, a non-finite weight gives its query no rows, and no NaN is ever ranked or returned.
 *   base(q, r)    = the f32 score arx_topk_search and arx_topk_search_filtered give the pair, bit for bit
 *   boosted(q, r) = fl32(base(q, r) + p(q, r)): two separately rounded f32 operations, no FMA (numpy: base + np.float32(w) * prior)
 * The answer is the k best visible rows by (boosted desc, row asc):
 *   out_scores f32 [n_queries, k] = boosted, out_base f32 [n_queries, k] = base of the same rows, out_ids int64 [n_queries, k] =
 *   idx_base + row; padding (-inf, -inf, -1).  weight[q] == 0: the ids and base bits of arx_topk_search_filtered.
 * max_abs_prior: an upper bound on |prior[r]| over the finite values, the caller's contract as max_row_norm is (arx_prior_info measures
 * it): too small voids the exactness proof (csrc/boosted.hip), too large only widens the candidate set.  max_row_norm as for the
 * filtered search, 0 = unit rows.  1 <= k <= 32, dim % 64 == 0 up to 8192, any n_queries (sliced above 1 024).
 * path: 0 = library's choice, 1 = the scan, 2 = exhaustive over the visible rows; cand_cap = candidate groups a query may list before it
 * goes to the exhaustive path (0 = default 1 024, at most 8192): test hooks, same bits for every choice.  A query's output depends on
 * its row of `queries`, its weight, the prior, the bitmap and the corpus alone - not on the batch, its order, the path or cand_cap.
 * A null or misaligned pointer, a negative size, k or dim out of range, a max_abs_prior that is negative or not finite, a workspace
 * that is too small: ARX_ERR_ARG before any launch, the message naming the part.
 * ws: device workspace of arx_topk_search_boosted_workspace_bytes(...) bytes, caller-owned (-1 for an unsupported shape); the stats
 * counters sit at its start as the siblings' do. */
int64_t arx_topk_search_boosted_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t k);
int32_t arx_topk_search_boosted(const void* corpus, int64_t n_rows, const float* prior, float max_abs_prior, const float* weight,
                                const uint64_t* allow, int64_t n_allowed, const void* queries, int32_t n_queries, int32_t dim, int32_t k,
                                float* out_scores, float* out_base, int64_t* out_ids, int64_t idx_base, float max_row_norm, void* ws,
                                int64_t ws_bytes, int32_t path, int32_t cand_cap, void* stream);
/* {queries sent to the exhaustive path because their candidate list overflowed, candidate groups rescored} of the LAST boosted search
 * on this workspace.  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_topk_boosted_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream);
/* out (device int64 [2], written by the kernels on `stream`): out[0] = the f32 bits (in the low word) of the largest |finite value| of
 * prior[0 .. n_rows), 0 when there is none; out[1] = the number of non-finite values (NaN, +-inf).  One pass.  What max_abs_prior wants. */
int32_t arx_prior_info(const float* prior, int64_t n_rows, int64_t* out, void* stream);

/* ---- Score threshold (`min_score`): every row at or above a cosine, up to 1 024 exact rows per query (csrc/range.hip) ------------------
 * min_score: device f32 [n_queries], one threshold per query.  allow: a row bitmap in the convention of arx_topk_search_filtered, NULL =
 * every row; n_allowed as there (-1 = unknown).  For query q a visible row r QUALIFIES when score(q, r) >= min_score[q], compared in
 * f32; score(q, r) has the bits arx_topk_search and arx_topk_search_filtered give the pair.  min_score[q] = -inf: every visible row
 * qualifies; +inf or NaN: none does.  The answer is the best min(count, M) qualifying rows by (score desc, row asc), M = max_results,
 * 1 <= M <= 1024:
 *   out_scores f32 [n_queries, M], out_ids int64 [n_queries, M] = idx_base + row, (-inf, -1) padding;
 *   out_counts int32 [n_queries] = the number of qualifying rows when that is <= M, and exactly M + 1 when more than M rows qualify.
 * M + 1 means "the list is truncated: it holds the best M".  An exact total above M is deliberately not offered: it would make a loose
 * threshold cost a full exact scan of the shard.  Every element of the three outputs is written.
 * A query's outputs depend on the query, its threshold, the bitmap and the corpus alone - not on the batch, its order, the path or
 * cand_cap.  dim % 64 == 0, 64 .. 8192; any n_queries (sliced above 1 024); n_rows < 2^32 (a row is 32 bits of a sort key; a larger
 * shard: ARX_ERR_ARG naming n_rows).  max_row_norm as for the filtered search, 0 = unit rows.  Two device paths with the same bits: the
 * scan (pass A of the filtered search, then a tail that rescores the groups a proved bound selects; the proof is in csrc/range.hip) and
 * the exhaustive scoring of every visible row, which also answers any query whose candidate list overflows.
 * A null pointer, max_results outside 1 .. 1024, dim % 64 != 0 or a non-finite max_row_norm: ARX_ERR_ARG before any launch, the message
 * naming the field and its value.
 * ws: device workspace of arx_range_workspace_bytes(...) bytes, caller-owned; with qb = min(n_queries, 1 024), ldg = qb rounded up to 64,
 * G = ceil(n_rows / 64), M = max_results and T = min(ceil(n_rows / 256), 128, floor(4096 / M)) it is the sum, each term rounded up to 256
 * bytes, of 64 + 4 G ldg + 8 G + 4 qb + 8 T qb M + 4 T qb (-1 for an unsupported shape: n_rows outside 1 .. 2^32 - 1, n_queries < 1,
 * dim not a multiple of 64 in 64 .. 8192, max_results outside 1 .. 1024). */
int64_t arx_range_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t max_results);
int32_t arx_range_search(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                         const float* min_score, int32_t n_queries, int32_t dim, int32_t max_results, float* out_scores, int64_t* out_ids,
                         int32_t* out_counts, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes, void* stream);
/* The same with the path and the candidate capacity chosen by the caller (tests, tuning): path 0 = library's choice, 1 = the scan,
 * 2 = exhaustive over the visible rows; cand_cap = candidate groups a query may list before it goes to the exhaustive path (0 =
 * default 2 (max_results + 1) + 1 024, at most 8192).  Same bits for every choice. */
int32_t arx_range_search_tuned(const void* corpus, int64_t n_rows, const uint64_t* allow, int64_t n_allowed, const void* queries,
                               const float* min_score, int32_t n_queries, int32_t dim, int32_t max_results, float* out_scores,
                               int64_t* out_ids, int32_t* out_counts, int64_t idx_base, float max_row_norm, void* ws, int64_t ws_bytes,
                               int32_t path, int32_t cand_cap, void* stream);
/* {queries sent to the exhaustive path because their candidate list overflowed, candidate groups rescored} of the LAST range search on
 * this workspace.  Copies 16 bytes to the host and waits on `stream`. */
int32_t arx_range_stats(const void* ws, int64_t* overflowed_queries, int64_t* candidate_groups, void* stream);

/* ---- Substring scan over the chunk texts (Chroma's `where_document`: `$contains` / `$not_contains`) -----------------------------
 * The producer of the row bitmaps arx_topk_search_filtered takes (csrc/textscan.hip).
 * out_bits[p][w] bit (r & 63) of word w = r >> 6  <=>  pattern p occurs in row r, entirely inside
 * [row_off[r], row_off[r+1]).  Bits at or beyond n_rows are written as 0.  Every word of out_bits is written:
 * the result does not depend on what the buffer held before.  Bytes compare as bytes (case-sensitive; on well-formed UTF-8 a byte
 * substring is a code-point substring).
 *   blob     device uint8 [row_off[n_rows]]       the shard's texts, concatenated, no separators (a valid pointer even if empty)
 *   row_off  device int64 [n_rows + 1]            ascending, row_off[0] == 0; empty rows allowed
 *   pat_blob device uint8, pat_off device int32 [n_pat + 1]; every pattern 1..256 bytes; 1 <= n_pat <= 32
 *   out_bits device uint64 [n_pat, ceil(n_rows / 64)]
 * Pattern lengths are device data and the caller's contract (a length outside 1..256 matches no row); a pattern longer than a row
 * cannot match it.  One launch on `stream`, no atomics, no workspace. */
int32_t arx_text_contains(const uint8_t* blob, const int64_t* row_off, int64_t n_rows,
                          const uint8_t* pat_blob, const int32_t* pat_off, int32_t n_pat,
                          uint64_t* out_bits, void* stream);
/* Regular-expression scan over the same texts (`$regex` / `$not_regex`; csrc/textscan.hip).  The output contract is that of
 * arx_text_contains: out_bits[p][w] bit (r & 63) of word w = r >> 6  <=>  regex p matches somewhere inside [row_off[r], row_off[r+1])
 * (`^` / `$` are that row's start and end); bits at or beyond n_rows are 0; every word is written with a plain store.
 * The host compiles each regex to a byte-level DFA (arxiv_rag_amd/regex_dfa.py: compile_regex, pack_tables); the kernel walks tables.
 *   tables    device uint8, table_off device int32 [n_re + 1]; 1 <= n_re <= 8.  Table p = tables[table_off[p], table_off[p+1]):
 *             uint16 n_states, uint16 n_classes (little-endian, each 1..256), class_of[256], flags[n_states],
 *             trans[n_states][n_classes].  The start state is 0; after byte b in state s the state is trans[s][class_of[b]].
 *             flags: 1 = matched (absorbing: the row matches whatever follows), 2 = the row matches if it ends in this state,
 *             4 = dead (absorbing, no accepting state reachable).  A row matches when the state at its end has flag 1 or 2.
 *   out_bits  device uint64 [n_re, ceil(n_rows / 64)]
 * The tables are device data and the caller's contract.  A header outside 1..256, or a table shorter than its header says, makes that
 * regex match no row; a class or transition outside its range is read as 0: a malformed table gives wrong bits, never an access
 * outside the kernel's LDS copy of it.  One launch on `stream` (a block holds one regex's table in LDS; the regex is the grid's y),
 * no atomics, no workspace. */
int32_t arx_text_regex(const uint8_t* blob, const int64_t* row_off, int64_t n_rows,
                       const uint8_t* tables, const int32_t* table_off, int32_t n_re,
                       uint64_t* out_bits, void* stream);
/* The same with the launch shape chosen: waves_per_block = 64-row groups (output words) a block of that many waves covers with one
 * staged table; 0 = default (8), else 1, 2, 4, 8 or 16.  Same bits for every choice. */
int32_t arx_text_regex_tuned(const uint8_t* blob, const int64_t* row_off, int64_t n_rows,
                             const uint8_t* tables, const int32_t* table_off, int32_t n_re,
                             uint64_t* out_bits, int32_t waves_per_block, void* stream);
/* *out_count (ONE device int64) = set bits of bits[0 .. ceil(n_rows/64)) that name rows below n_rows. */
int32_t arx_bitmap_count(const uint64_t* bits, int64_t n_rows, int64_t* out_count, void* stream);

/* ---- Stable compaction under a row bitmap (csrc/compact.hip; `HipCollection.compact()`) ---------------------------------------------
 * Dropping rows from what a shard keeps in HBM without a round trip through the host.  `keep` is a row bitmap in the convention of
 * arx_topk_search_filtered: device uint64 [ceil(n_rows / 64)], bit (r & 63) of word r >> 6 set = row r stays; bits at or beyond n_rows
 * are ignored and may be garbage.  The three calls are stream-ordered on `stream`, work on caller-owned memory only (no workspace), use
 * no atomics and no float arithmetic, and return ARX_ERR_ARG, naming the argument, before any launch on a null pointer, an n_rows
 * outside [0, 2^36) or a row_bytes outside [1, 16384].
 *
 * The plan:  word_rank device int64 [ceil(n_rows / 64) + 1] receives the exclusive prefix sum of the words' popcounts, the total in
 * its last entry and in *out_count (ONE device int64).  The new position of a kept row r is
 *     word_rank[r >> 6] + popcount(keep[r >> 6] & ((1 << (r & 63)) - 1)).
 * Every entry is written; n_rows == 0 writes word_rank[0] = 0 and a count of 0 (keep may then be null).  Three launches (per-block
 * sums, one scan of the block totals, one pass that adds them): no block waits for another. */
int32_t arx_compact_plan(const uint64_t* keep, int64_t n_rows, int64_t* word_rank, int64_t* out_count, void* stream);
/* Fixed-size rows, out of place: kept row r of src [n_rows, row_bytes] goes to row new(r) of dst.  `word_rank` is the plan of the same
 * `keep`.  dst must not overlap src (the caller's contract).  Rows [0, count) of dst are written and nothing else: a byte beyond
 * count * row_bytes keeps what it held.  Only kept rows are read; a 64-row word of `keep` that is zero costs its one load.  Rows move
 * in 16-byte units when row_bytes and both pointers are multiples of 16, byte by byte otherwise, with the same result.  A plan that
 * is not this bitmap's (a word's rows would land beyond the plan's own total) moves nothing for that word.  One launch. */
int32_t arx_compact_rows(const void* src, void* dst, int64_t row_bytes, int64_t n_rows, const uint64_t* keep, const int64_t* word_rank,
                         void* stream);
/* The same for variable-length rows: blob / row_off as for arx_text_contains.  new_row_off device int64 [count + 1] receives the
 * exclusive prefix sum of the kept rows' lengths, starting at 0 (scanned in three launches like the plan); new_blob receives their
 * bytes, back to back.  new_blob must hold the kept bytes (row_off[n_rows] always suffices) and must not overlap blob; nothing is
 * written beyond new_row_off[count].  Empty rows, an empty blob and count == 0 are legal; n_rows == 0 writes new_row_off[0] = 0.
 * Offsets are device data and the caller's contract: a row is clamped into [0, row_off[n_rows]] as the text scans clamp it, and a row
 * whose bytes would end beyond row_off[n_rows] in new_blob is skipped, so offsets outside the contract give wrong bytes, never an
 * access out of range.  Four launches. */
int32_t arx_compact_text(const uint8_t* blob, const int64_t* row_off, int64_t n_rows, const uint64_t* keep, const int64_t* word_rank,
                         uint8_t* new_blob, int64_t* new_row_off, void* stream);

/* ---- Chroma `where` filters over metadata columns in HBM (csrc/where_eval.hip; the lowering is arxiv_rag_amd/where_device.py) ----
 * A column is one metadata key over the shard's rows: kind uint8 [n_rows] (0 = absent or another type, 1 = number, 2 = string,
 * 3 = bool) and val f64 [n_rows] (the number; a string's rank in the sorted distinct strings of the key; 0.0 / 1.0 for a bool; 0.0
 * otherwise): 9 bytes per row and key.  col_table holds the two device addresses of every column of the call.
 * A filter is a postfix program over its own leaves.  Token = (arg << 2) | code, int32:
 *   code 0  LEAF i   push leaf i of this filter (i counts from the filter's first leaf)
 *   code 1  AND n    pop n entries, push 1 if all are 1          (1 <= n <= 32)
 *   code 2  OR n     pop n entries, push 1 if any is 1
 * The stack never holds more than 32 entries and ends with one, the row's result: the CALLER's contract (the arrays are device data).
 * A leaf is true for row r when  (kind[r] == want_kind && cmp(val[r], operand)) != (negate != 0), compared in f64:
 *   op 0 EQ ==   1 GT >   2 GE >=   3 LT <   4 LE <=   5 IN val[r] is one of set_vals[set_off, set_off + set_len)   6 NEVER false
 * A set slice is ascending, distinct and NaN-free; it is searched by value (-0.0 finds 0.0).
 * The layout of a leaf, 32 bytes, no padding: */
typedef struct {
    double  operand;      /* offset  0: the right-hand side of EQ..LE; unused by IN and NEVER */
    int32_t column;       /* offset  8: index into col_table, 0 <= column < n_cols */
    int32_t want_kind;    /* offset 12: 1 number, 2 string, 3 bool */
    int32_t op;           /* offset 16 */
    int32_t negate;       /* offset 20: 0 or 1 ($ne, $nin) */
    int32_t set_off;      /* offset 24: IN: first entry of the leaf's slice of set_vals */
    int32_t set_len;      /* offset 28: IN: its length */
} arx_where_leaf;
/*   col_table  device int64 [n_cols][2]            {address of kind, address of val} per column; n_cols >= 1
 *   leaves     device arx_where_leaf [leaf_off[n_filters]];  leaf_off  device int32 [n_filters + 1], ascending from 0
 *   tokens     device int32 [token_off[n_filters]];          token_off device int32 [n_filters + 1], ascending from 0
 *   set_vals   device f64 [n_set_vals], 0 <= n_set_vals <= 2^20 (may be NULL when 0)
 *   and_with   NULL, or device uint64 bitmaps and-ed into the result: filter f uses the words at and_with + f * and_stride
 *              (and_stride in words; 0 = one bitmap for all filters)
 *   out_bits   device uint64 [n_filters][ceil(n_rows / 64)]: bit (r & 63) of word r >> 6 of bitmap f <=> row r satisfies filter f
 *              (and and_with allows it).  Bits at or beyond n_rows are written as 0.  The layout arx_topk_search_filtered_multi takes.
 *   out_counts device int64 [n_filters]: the set bits of each bitmap, written by the kernels on `stream`.
 * Every word of out_bits and every count is written: neither depends on what the buffers held before.  Two launches on `stream` (all
 * bitmaps, then the counts), no atomics, no workspace, no host synchronisation.  1 <= n_filters <= 64, 1 <= n_rows < 2^36.
 * A null pointer, n_filters, n_rows, n_cols or n_set_vals out of range or a negative and_stride: ARX_ERR_ARG before any launch, the
 * message names the field.  What the leaves and offsets hold is device data: where_device.py validates it on the host before the
 * upload (a column index outside [0, n_cols) is refused there), and the kernel clamps leaf, column and set indices to the ranges the
 * call declares, so a damaged program yields wrong bits but reads nothing out of range. */
int32_t arx_where_eval(const int64_t* col_table, int32_t n_cols, int64_t n_rows,
                       const arx_where_leaf* leaves, const int32_t* leaf_off,
                       const int32_t* tokens, const int32_t* token_off,
                       const double* set_vals, int64_t n_set_vals, int32_t n_filters,
                       const uint64_t* and_with, int64_t and_stride,
                       uint64_t* out_bits, int64_t* out_counts, void* stream);

/* ---- Facet counts of metadata keys under row bitmaps (csrc/facet.hip; the host layer is arxiv_rag_amd/facets.py) ---------------------
 * "How many allowed rows per value of this key": the columns are those of arx_where_eval (kind uint8 + val f64 per row), the bitmaps
 * those every filter here produces (bit (r & 63) of word r >> 6 = row r is allowed).  A key describes one column and how a row's value
 * becomes a bin.  The bin applies only to a row whose bit is set and whose kind[r] == want_kind:
 *   mode 0 ARX_FACET_CODE      the bin is val[r], if it is an integer in [0, n_bins) (strings by their code, bools as 0 / 1)
 *   mode 1 ARX_FACET_EXACT     the bin is i with cuts[i] == val[r]; cuts holds n_bins values, ascends strictly and holds no NaN; the
 *                              lookup is a binary search with the IEEE compare, so -0.0 finds 0.0
 *   mode 2 ARX_FACET_INTERVAL  the bin is i with cuts[i] <= val[r] < cuts[i + 1]; cuts holds n_bins + 1 ascending edges and
 *                              val[r] == cuts[n_bins] falls into the last bin (numpy.histogram's convention)
 * Comparisons are in f64; no arithmetic touches the values.  The layout of a key, 48 bytes, no padding; the array of keys is a HOST
 * array whose pointers are DEVICE pointers: */
#define ARX_FACET_CODE     0
#define ARX_FACET_EXACT    1
#define ARX_FACET_INTERVAL 2
typedef struct arx_facet_key {
    const uint8_t* kind;  /* offset  0: device uint8 [n_rows] */
    const double*  val;   /* offset  8: device f64 [n_rows] */
    const double*  cuts;  /* offset 16: device f64; mode 1: n_bins values, mode 2: n_bins + 1 edges, mode 0: unused, may be NULL */
    int32_t mode;         /* offset 24 */
    int32_t want_kind;    /* offset 28: 1 number, 2 string, 3 bool */
    int32_t n_bins;       /* offset 32: 1 .. 2^20 */
    int32_t reserved;     /* offset 36: 0 */
    int64_t out_off;      /* offset 40: where this key's n_bins + 2 counters start within a filter's slice of out */
} arx_facet_key;
/*   allow   NULL (every row), or device uint64 bitmaps of ceil(n_rows / 64) words: filter f reads the words at allow + f * allow_stride
 *           (allow_stride in words; 0 = one bitmap for all filters).  Bits of the last word at or beyond n_rows are not trusted and
 *           not counted.
 *   out     device int32 [n_filters][out_stride].  Filter f and key j own out[f * out_stride + out_off_j + b]:  b < n_bins the bins,
 *           b == n_bins "missing" (an allowed row whose kind is not want_kind), b == n_bins + 1 "unbinned" (the right kind, no bin: a
 *           NaN, a value outside the edges or not among the cuts, a code out of range or not integral).  Every key's counters sum to
 *           the allowed rows below n_rows.
 * The call zeroes all n_filters * out_stride counters on `stream` and launches once: grid (row chunks, filters, keys); a zero bitmap
 * word costs its one load.  A key with n_bins + 2 <= 8192 is counted in an LDS histogram per block and flushed with one integer atomic
 * per non-zero counter, a larger one adds to `out` directly; a wave whose rows agree on the bin issues one add of their number.  Only
 * integer atomic adds are used, so the counts do not depend on the launch shape or on the order of arrival.  No workspace, no host
 * synchronisation.
 * ARX_ERR_ARG before anything is launched or zeroed, the message naming the field: a null keys, out, kind, val or (modes 1, 2) cuts;
 * n_keys outside 1..16; n_filters outside 1..64; n_bins outside 1..2^20; n_rows outside [0, 2^31); a mode or want_kind not among its
 * values; a negative allow_stride; a key's counters outside out_stride or overlapping another key's; n_filters * out_stride > 2^27.
 * What the columns and cuts hold is device data: values outside the contract (a wild code, unsorted cuts) may give wrong counts, never
 * a read or write outside the arrays passed. */
int32_t arx_facet_count(const arx_facet_key* keys, int32_t n_keys, int64_t n_rows,
                        const uint64_t* allow, int64_t allow_stride, int32_t n_filters,
                        int32_t* out, int64_t out_stride, void* stream);
/* The same with the launch shape chosen: block_threads a multiple of 64 in 64..1024 (default 256), blocks_x >= 1 row-chunk blocks
 * (blocks without a word exit), lds_bins in 0..32768 counters an LDS histogram may hold (default 8192 = 32 KiB; 0 forces the direct
 * path).  Same counts for every choice. */
int32_t arx_facet_count_tuned(const arx_facet_key* keys, int32_t n_keys, int64_t n_rows,
                              const uint64_t* allow, int64_t allow_stride, int32_t n_filters,
                              int32_t* out, int64_t out_stride,
                              int32_t block_threads, int32_t blocks_x, int32_t lds_bins, void* stream);

/* ---- Spherical k-means update over fp16 rows (csrc/cluster.hip; the host layer is arxiv_rag_amd/topics.py; INTEGRATION.md "Topics") ----
 * The assign half of a Lloyd iteration is arx_cluster_assign below; these calls are the other half.
 *   rows    device fp16 [n_rows, dim], 16-byte aligned
 *   order   device int32 [n_members]: row numbers sorted by (cluster, row)
 *   start   device int64 [C + 1]: cluster c owns order[start[c], start[c + 1])
 *   sums    device f32 [C, dim]: S_c[d]; every element is written
 * A cluster's members are cut into runs of 256 consecutive entries of `order`.  A run's partial starts at 0.0f and adds float(row[d])
 * entry by entry in ascending position; S_c[d] starts at 0.0f and adds the cluster's partials in ascending run order; every add is a
 * plain f32 add made by one thread.  The bits therefore depend on rows, order and start alone, never on the launch shape, and equal
 * topics.sums_host (numpy.cumsum in f32 per run, then over the partials).  Two launches on `stream` (partials, then sums), no atomics,
 * no host synchronisation, no workspace beyond the partials:
 *   partials  device scratch of arx_cluster_sums_workspace_bytes(n_members, C, dim) = (ceil(n_members / 256) + C) * dim * 4 bytes,
 *             16-byte aligned (-1 for arguments outside the contract below).
 * ARX_ERR_ARG before anything is launched, the message naming the field: dim not a multiple of 64 in [64, 8192]; C outside
 * [1, 4096]; n_rows or n_members outside [0, 2^31); a null or misaligned pointer; ws_bytes below the figure above.  n_members == 0 or
 * n_rows == 0 zeroes `sums`.
 * order and start are device data: an order entry outside [0, n_rows) keeps its place in its run and adds nothing; start values are
 * clamped into [0, n_members] and made non-decreasing (a running maximum) before use.  Wrong data gives wrong sums, never a read or
 * write outside the arrays passed. */
int64_t arx_cluster_sums_workspace_bytes(int64_t n_members, int32_t C, int32_t dim);
int32_t arx_cluster_sums(const void* rows, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                         int32_t C, void* partials, int64_t ws_bytes, float* sums, void* stream);
/* The same with the launch shape of the partials chosen: block_threads a multiple of 64 in 64..1024 (default 256), runs_per_block in
 * 1..64 runs a block carries side by side (0 = default: the fewest that fill whole waves, doubled while they fit the block).  Same
 * bits for every choice. */
int32_t arx_cluster_sums_tuned(const void* rows, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                               int32_t C, void* partials, int64_t ws_bytes, float* sums, int32_t block_threads, int32_t runs_per_block,
                               void* stream);
/* The new centroids from the sums: out_f32[c] = S_c / sqrtf(sum_d S_c[d]^2), out_f16 = that rounded to nearest even (device fp16
 * [C, dim]).  The sum of squares has one fixed order: lane l of 64 adds S[d] * S[d] over d = l, l + 64, ... ascending (product rounded,
 * then added), then v_l = v_l + v_(l ^ o) for o = 32, 16, 8, 4, 2, 1; sqrtf and the division are IEEE.  A cluster that is empty
 * (start, clamped below at 0 and made non-decreasing, gives it no entry) or whose norm is 0 or not finite keeps prev[c] (device f32
 * [C, dim]) bit for bit.  One launch, one wave per cluster.  Same contract for dim and C; a null pointer is ARX_ERR_ARG. */
int32_t arx_cluster_finish(const float* sums, const int64_t* start, const float* prev, int32_t C, int32_t dim, float* out_f32,
                           void* out_f16, void* stream);

/* ---- Nearest centroid of every row (csrc/cluster_assign.hip; the host layer is arxiv_rag_amd/topics.py; INTEGRATION.md "Topics") ----
 * The assign half of a Lloyd iteration, and "label rows against given centroids":
 *   out_labels[i] = the lowest c that maximises score(centroid c, row i)        out_scores[i] = that f32 value
 * where score is exact_row_score (csrc/exact_score.h), the score of arx_topk_search: 8 lanes per pair, lane l taking the 16-byte
 * chunks l, l + 8, ... in ascending order, two fmaf chains per lane over even and odd elements, a0 + a1, then the butterfly xor 4, 2,
 * 1.  For finite inputs and a valid norm bound the result equals arx_topk_search(k = 1) over the centroids bit for bit, labels and
 * scores (and topics.assign_exact_host).
 *   rows               device fp16 [n_rows, dim], 16-byte aligned
 *   centroids_f16      device fp16 [C, dim], 16-byte aligned
 *   max_centroid_norm  a bound on the centroids' 2-norms, positive and finite (0 = 1 + 2^-9, as max_row_norm)
 *   out_labels         device int32 [n_rows];  out_scores device f32 [n_rows]; 16-byte aligned, every element written once by a plain store
 *   stats              device int64 [2] or NULL: {rows flagged, exact scores computed on the slow path}, set by the call
 *   ws                 device scratch of arx_cluster_assign_workspace_bytes(n_rows, C, dim) = 16 + 4 n_rows (rounded up to 16) bytes,
 *                      16-byte aligned (-1 for arguments outside the contract below)
 * Fast pass: an fp16 MFMA GEMM of row tiles against centroid tiles with f32 accumulation whose epilogue keeps, per row, the best
 * approximate score with its centroid (ties to the lower one) and the second best.  Certificate: with
 *   tau_i = tau_mult * (1.0625 * dim + 4) * 2^-24 * |x_i|_2 * max_centroid_norm
 * (dim * 2^-24 for the MFMA sum in any order, (dim / 16 + 4) * 2^-24 for the exact score; |x_i|_2 computed in the kernel and rounded
 * up) a row with a_best - a_second > 2 tau_i has a unique exact winner, and one exact score of that pair is its score.  Every other row
 * (near ties, NaN or inf rows; none when C == 1) is FLAGGED: listed behind an integer counter and scored against every centroid by
 * the second launch, which reads the count on the device.  Two identical centroids flag every row: n_rows * C * dim FMAs, what the
 * search pays.  Two launches and one 16-byte memset on `stream`, no host synchronisation, no float atomics; the results do not depend
 * on the launch shape.
 * ARX_ERR_ARG before anything is launched, the message naming the field: dim not a multiple of 64 in [64, 8192]; C outside [1, 4096];
 * n_rows outside [0, 2^31); a null or misaligned pointer; ws_bytes below the figure above; max_centroid_norm negative or not finite.
 * n_rows == 0 launches nothing (stats are zeroed).  Rows and centroids are device data: values that are not finite lie outside the
 * equality above and give some label in [0, C), never a read or write outside the arrays passed. */
int64_t arx_cluster_assign_workspace_bytes(int64_t n_rows, int32_t C, int32_t dim);
int32_t arx_cluster_assign(const void* rows, int64_t n_rows, int32_t dim, const void* centroids_f16, int32_t C, float max_centroid_norm,
                           int32_t* out_labels, float* out_scores, int64_t* stats, void* ws, int64_t ws_bytes, void* stream);
/* The same with the certificate's margin and the launch shape chosen: tau_mult 0 (= 1) or a finite value >= 1 (values in (0, 1) are
 * refused; 1e9 sends every row of a C >= 2 call down the slow path); rows_per_block 0 (default), 32 or 64 rows a block stages.  Same
 * bits for every choice. */
int32_t arx_cluster_assign_tuned(const void* rows, int64_t n_rows, int32_t dim, const void* centroids_f16, int32_t C,
                                 float max_centroid_norm, int32_t* out_labels, float* out_scores, int64_t* stats, void* ws,
                                 int64_t ws_bytes, float tau_mult, int32_t rows_per_block, void* stream);

/* ---- IVF probe search: exact top-k over the rows of the lists a query probes (csrc/ivf.hip; the host layer is arxiv_rag_amd/ivf.py;
 * the definition is INTEGRATION.md "IVF probe search") ------------------------------------------------------------------------------
 * The lists are the member lists of a clustering (topics.members): order[start[c] .. start[c + 1]) are the rows of list c.  The rows
 * query q SEES are order[j] for j in [start[c], start[c + 1]) over the distinct c in probes[q] that lie in [0, n_lists), restricted to
 * [0, n_rows) and, when `allow` is given, to rows whose bit is set.  Per query the call returns the best k visible rows by
 * (exact_row_score desc, row asc), padded with (-inf, -1); ids are row + idx_base; out_scanned[q] is the number of visible rows, each
 * scored once.  A (query, row) score is exact_row_score (csrc/exact_score.h), the bits of arx_topk_search; the answer equals
 * arx_topk_search_filtered over the bitmap of the visible rows bit for bit.  Which lists to probe is the caller's choice (the nearest
 * centroids: ivf.IvfIndex.probe) and the only approximation.
 *   corpus        device fp16 [n_rows, dim], 16-byte aligned; queries device fp16 [n_queries, dim], 16-byte aligned
 *   order         device int32 [n_members] (NULL only when n_members == 0); start device int64 [n_lists + 1]
 *   max_list_rows a bound on the lists' lengths the HOST knows (it sizes the grid: no host read inside the call); a list is read up to
 *                 its first max_list_rows entries
 *   probes        device int32 [n_queries, n_probe]
 *   allow         device uint64 [ceil(n_rows / 64)] or NULL: arx_topk_search_filtered's convention (bit r & 63 of word r >> 6)
 *   out_scores    device f32 [n_queries, k]; out_ids device int64 [n_queries, k]; out_scanned device int64 [n_queries] or NULL
 *   ws            device scratch of arx_ivf_workspace_bytes(n_members, n_lists, n_queries, n_probe, dim, k) bytes, 16-byte aligned
 *                 (-1 for arguments outside the limits below); at most about 50 MB
 * Three launches per 1024 queries on `stream` (prepare: dedupe the probes, cumulative list lengths; scan: blocks of rows_per_block list
 * positions x query, 8 lanes per row; merge: any number of partial lists per query), no host synchronisation, no float atomics.  A
 * query's answer depends on its row of queries, its row of probes, the lists, `allow` and the corpus; not on the batch, its order or
 * the launch shape.
 * ARX_ERR_ARG before anything is launched, the message naming the field: k outside 1..32; n_probe outside 1..128; dim not a multiple of
 * 64 or above 8192; n_lists outside 1..4096; n_rows outside 1..2^31-1; n_members outside 0..2^31-1; max_list_rows outside
 * 0..n_members; n_queries < 1; a null or misaligned pointer; ws_bytes below the figure above.
 * order, start and probes are device data.  Bad values give a defined answer and never an access out of range: a probe outside
 * [0, n_lists) is ignored; a repeated probe counts once; start is read clamped into [0, n_members] and made non-decreasing
 * (topics.clamp_starts); an order entry outside [0, n_rows) keeps its place and is skipped.  order should name a row at most once; if
 * it does not, a row may come back twice. */
int64_t arx_ivf_workspace_bytes(int64_t n_members, int32_t n_lists, int32_t n_queries, int32_t n_probe, int32_t dim, int32_t k);
int32_t arx_ivf_search(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                       int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries, const int32_t* probes,
                       int32_t n_probe, const uint64_t* allow, int32_t k, float* out_scores, int64_t* out_ids, int64_t* out_scanned,
                       int64_t idx_base, void* ws, int64_t ws_bytes, void* stream);
/* The same with the scan's launch shape chosen: rows_per_block list positions per block, 0 (default: 128, growing to 1024 while the
 * grid holds more than 2048 blocks) or a multiple of 64 in 64..2^20; raised where the workspace could not hold the partial lists.  Same
 * bits for every choice. */
int32_t arx_ivf_search_tuned(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                             int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries, const int32_t* probes,
                             int32_t n_probe, const uint64_t* allow, int32_t k, float* out_scores, int64_t* out_ids,
                             int64_t* out_scanned, int64_t idx_base, void* ws, int64_t ws_bytes, int32_t rows_per_block, void* stream);
/* arx_ivf_search_multi: arx_ivf_search with a row filter per query and a score threshold per query, in the same three launches (a scan
 * block serves one query, so both are values the block loads once).  The arguments of arx_ivf_search, with after `allow`:
 *   allow         device uint64 [n_filters][ceil(n_rows / 64)] or NULL; n_filters >= 1 (any number: there is no limit of 64)
 *   filter_of     device int32 [n_queries]: the bitmap of query q is allow + filter_of[q] * ceil(n_rows / 64)
 *   min_score     device f32 [n_queries] or NULL (4-byte aligned)
 * and after out_scanned:
 *   out_hits      device int64 [n_queries] or NULL
 * Visible rows: query q sees the rows arx_ivf_search sees with `allow` replaced by its own bitmap.  filter_of is device data: a value
 * outside [0, n_filters) means the query sees no row (all (-inf, -1), scanned = 0, hits = 0) and nothing is read through it, the
 * convention of arx_topk_search_filtered_multi and arx_bm25_search_filtered.  allow == NULL means no filter: filter_of is ignored and
 * may be NULL.  out_scanned[q] is the number of visible rows, each scored once.
 * With min_score a visible row QUALIFIES when score >= min_score[q], a plain f32 compare on the exact_row_score bits: a NaN score never
 * qualifies, a NaN threshold qualifies nothing, -inf qualifies every visible row whose score is not NaN.  With min_score == NULL every
 * visible row qualifies and is ranked as arx_ivf_search ranks it.  (There a NaN score, which needs inf or NaN in the rows or the query,
 * never starts a merge of the running top-k, and inside one it wins or loses by comparisons that are all false: the rank of such a row
 * is not defined.  It is whatever arx_ivf_search gives: the code is the same.)
 * Result: the best k qualifying rows by (score desc, row asc), padded with (-inf, -1), ids + idx_base.  out_hits[q] is the exact number
 * of qualifying rows, an int64 sum of integer per-block counts with no cap; with min_score == NULL out_hits[q] = out_scanned[q].
 * With n_filters = 1, filter_of all zero and min_score = NULL the outputs equal arx_ivf_search's with that bitmap bit for bit, for every
 * rows_per_block.  Query by query the outputs equal those of a call with that query alone: the batch, its order, the other queries'
 * filters and thresholds and the launch shape do not matter.  No float atomics.
 *   ws            device scratch of arx_ivf_multi_workspace_bytes(...) bytes, 16-byte aligned: arx_ivf_workspace_bytes of the same
 *                 arguments + 4 bytes per (partial list, query) slot, rounded up to 256 (the blocks' counts of qualifying rows), where
 *                 slots = clamp(ceil(n_members / 64) * min(n_queries, 1024), min(n_queries, 1024), 2^17); -1 outside the limits
 * ARX_ERR_ARG, the message naming the field: everything arx_ivf_search_tuned refuses; with allow given, n_filters < 1 or a null
 * filter_of; a filter_of or min_score that is not 4-byte aligned; ws_bytes below the figure above. */
int64_t arx_ivf_multi_workspace_bytes(int64_t n_members, int32_t n_lists, int32_t n_queries, int32_t n_probe, int32_t dim, int32_t k);
int32_t arx_ivf_search_multi(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members, const int64_t* start,
                             int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries, const int32_t* probes,
                             int32_t n_probe, const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const float* min_score,
                             int32_t k, float* out_scores, int64_t* out_ids, int64_t* out_scanned, int64_t* out_hits, int64_t idx_base,
                             void* ws, int64_t ws_bytes, void* stream);
int32_t arx_ivf_search_multi_tuned(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* order, int64_t n_members,
                                   const int64_t* start, int32_t n_lists, int64_t max_list_rows, const void* queries, int32_t n_queries,
                                   const int32_t* probes, int32_t n_probe, const uint64_t* allow, int32_t n_filters,
                                   const int32_t* filter_of, const float* min_score, int32_t k, float* out_scores, int64_t* out_ids,
                                   int64_t* out_scanned, int64_t* out_hits, int64_t idx_base, void* ws, int64_t ws_bytes,
                                   int32_t rows_per_block, void* stream);

/* ---- Binary-code search: sign-bit codes, exact Hamming candidate lists (csrc/binary.hip; the host layer is arxiv_rag_amd/binary.py;
 * the definition is INTEGRATION.md "Binary-code search") -----------------------------------------------------------------------------
 * arx_binary_pack: rows device fp16 [n_rows, dim] -> out_codes device uint64 [n_rows, dim / 64].  Bit j & 63 of word j >> 6 is set iff
 * (float)x[j] > centre[j]: a strict f32 compare, so NaN gives 0, +inf gives 1 (against a finite centre), -0 and a value equal to the
 * centre give 0.  centre is device f32 [dim] or NULL (NULL: 0).  This is the bit convention of the row bitmaps, on the host
 * np.packbits(bits, bitorder="little").view(np.uint64).  One launch on `stream`, every word written once with a plain store, no atomics,
 * no float arithmetic beyond the convert and the compare.  The same call packs the queries.  n_rows = 0 is legal and launches nothing.
 * ARX_ERR_ARG before the launch, the message naming the field: dim not a multiple of 64 in 64..8192; n_rows outside 0..2^31-1; a null
 * rows or out_codes with n_rows > 0; rows not 2-byte, centre not 4-byte or out_codes not 8-byte aligned. */
int32_t arx_binary_pack(const void* rows, int64_t n_rows, int32_t dim, const float* centre, uint64_t* out_codes, void* stream);
/* arx_binary_candidates: with W = dim / 64, d(q, r) = sum over w of popcount(codes[r][w] ^ qcodes[q][w]), an integer.  The VISIBLE rows
 * are [0, n_rows), restricted to the rows whose bit of `allow` is set when it is given.  C(q) is the first min(R, visible) visible rows
 * by (d ascending, row ascending), R = n_candidates: distances are integers, so C(q) is defined exactly, ties to the lower row.
 *   codes         device uint64 [n_rows, W], 16-byte aligned (NULL only when n_rows == 0); qcodes device uint64 [n_queries, W]
 *   allow         device uint64 [ceil(n_rows / 64)] or NULL: arx_topk_search_filtered's convention (bit r & 63 of word r >> 6); bits at
 *                 or beyond n_rows may hold anything
 *   out_cand      device int32 [n_queries, R]: C(q) in that order, padded with -1.  Rows are local (there is no idx_base)
 *   out_dist      device int32 [n_queries, R] or NULL: their distances, padded with -1
 *   out_count     device int64 [n_queries]: |C(q)|
 *   ws            device scratch of arx_binary_workspace_bytes(n_rows, n_queries, dim, n_candidates) bytes, 16-byte aligned (-1 for
 *                 arguments outside the limits below); at most 64 MiB
 * Two launches per 256 queries on `stream` (scan: blocks of rows_per_block rows x tile of 8 queries, so the code array is read once per
 * query tile, not once per query; a 64-row word of `allow` that is zero costs its one load; merge: one block per query over any number
 * of partial lists), no host synchronisation, integer work only, no global atomics.  A query's outputs depend on its own row of qcodes,
 * codes and allow; not on the batch, its order, the tile it lands in or the launch shape.  n_rows = 0 is legal: all -1, counts 0.
 * ARX_ERR_ARG before anything is launched, the message naming the field: n_candidates outside 1..256; dim not a multiple of 64 in
 * 64..8192; n_rows outside 0..2^31-1; n_queries < 1; a null or misaligned pointer; ws_bytes below the figure above.
 * codes, qcodes and allow are device data of which every bit pattern is legal: nothing read from them addresses anything.
 * THE EXACT RESCORE needs no call of its own.  The candidate lists are lists in arx_ivf_search's layout: order = out_cand flattened
 * (an entry of -1 keeps its place and is skipped), n_members = n_queries * R, start[q] = q * R (int64 [n_queries + 1]), n_lists =
 * n_queries, max_list_rows = R, probes[q] = {q}, n_probe = 1, allow = NULL (it has been applied).  arx_ivf_search then returns the best
 * k <= 32 of C(q) by (exact_row_score desc, row asc), with the score bits of every other search; out_scanned[q] = |C(q)|.  n_lists is at
 * most 4096 there, so the queries go in slices of at most 4096 (binary.py uses 1024).  Both calls are stream-ordered. */
int64_t arx_binary_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t n_candidates);
int32_t arx_binary_candidates(const uint64_t* codes, int64_t n_rows, int32_t dim, const uint64_t* qcodes, int32_t n_queries,
                              const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_dist, int64_t* out_count,
                              void* ws, int64_t ws_bytes, void* stream);
/* The same with the scan's launch shape chosen: rows_per_block rows per block, 0 (default: about 1024 blocks over the shard and the
 * query tiles, at least 2048 rows each) or a multiple of 64 in 64..2^20; raised where the workspace could not hold the partial lists.
 * Same bits for every choice. */
int32_t arx_binary_candidates_tuned(const uint64_t* codes, int64_t n_rows, int32_t dim, const uint64_t* qcodes, int32_t n_queries,
                                    const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_dist,
                                    int64_t* out_count, void* ws, int64_t ws_bytes, int32_t rows_per_block, void* stream);

/* ---- Product-quantised search: 8-bit PQ codes, byte look-up tables, exact candidate lists by table sum (csrc/pq.hip; the host layer
 * is arxiv_rag_amd/pq.py; the definition is INTEGRATION.md "Product-quantised search") --------------------------------------------
 * Shapes: dim a multiple of 64 in 64..8192; dsub a power of two in 4..64; M = dim / dsub in 1..256 (the look-up tables must fit in
 * LDS).  codebooks: device f32 [M, 256, dsub], 16-byte aligned, every value finite (the host layer checks that; the library reads them
 * as they are).  centre: device f32 [dim] or NULL.  fl32() below is one rounding to f32; no product is fused with a sum.
 * arx_pq_encode: rows device fp16 [n_rows, dim] (16-byte aligned) -> out_codes device uint8 [n_rows, M] (16-byte aligned).  For row r
 * and subspace m: v_t = fl32((float)x[m dsub + t] - centre[m dsub + t]) (the exact widened value without a centre); d_j starts from
 * acc = 0 and takes, t ascending, e = fl32(v_t - c[m][j][t]), acc = fl32(acc + fl32(e e)); the code starts as (best = d_0, code = 0)
 * and j = 1..255 wins iff d_j < best (strict): ties go to the lowest j, a NaN distance never wins, a row of NaN gets code 0.  One
 * launch on `stream`, every byte written once with a plain store, no atomics.  n_rows = 0 is legal and launches nothing.
 * ARX_ERR_ARG before the launch, the message naming the field: dim, dsub or M outside the shapes above; n_rows outside 0..2^31-1; a
 * null rows, codebooks or out_codes with n_rows > 0; a misaligned pointer. */
int32_t arx_pq_encode(const void* rows, int64_t n_rows, int32_t dim, int32_t dsub, const float* centre, const float* codebooks,
                      uint8_t* out_codes, void* stream);
/* arx_pq_lut: queries device fp16 [n_queries, dim] -> out_lut device uint8 [n_queries, M, 256].  f[m][j] starts from acc = 0 and takes,
 * t ascending, acc = fl32(acc + fl32((float)q[m dsub + t] c[m][j][t])): the query is NOT centred (<q, centre> is one constant per
 * query and does not change the order).  lo_m = min_j f[m][j]; span = max_m fl32(max_j f[m][j] - lo_m).  If any f is not finite, or
 * span is not a finite value > 0, the query's whole table is 0.  Otherwise inv = fl32(255.f / span) and
 * u[m][j] = (uint8) min(255, rintf(fl32(fl32(f - lo_m) inv))).  One launch, one block per query; n_queries = 0 launches nothing. */
int32_t arx_pq_lut(const void* queries, int32_t n_queries, int32_t dim, int32_t dsub, const float* codebooks, uint8_t* out_lut,
                   void* stream);
/* arx_pq_candidates: s(q, r) = sum over m of lut[q][m][codes[r][m]], an integer <= 65280.  The VISIBLE rows are [0, n_rows), restricted
 * to the rows whose bit of `allow` is set when it is given.  C(q) is the first min(R, visible) visible rows by (s descending, row
 * ascending), R = n_candidates: sums are integers, so C(q) is defined exactly, ties to the lower row.
 *   codes         device uint8 [n_rows, M], row-major, 16-byte aligned (NULL only when n_rows == 0); lut device uint8 [n_queries, M, 256],
 *                 16-byte aligned
 *   allow         device uint64 [ceil(n_rows / 64)] or NULL: arx_topk_search_filtered's convention; bits at or beyond n_rows may hold
 *                 anything
 *   out_cand      device int32 [n_queries, R]: C(q) in that order, padded with -1.  Rows are local (there is no idx_base)
 *   out_sum       device int32 [n_queries, R] or NULL: their sums, padded with -1
 *   out_count     device int64 [n_queries]: |C(q)|
 *   ws            device scratch of arx_pq_workspace_bytes(n_rows, n_queries, dim, dsub, n_candidates) bytes, 16-byte aligned (-1 for
 *                 arguments outside the limits, n_queries < 1 among them); at most 64 MiB
 * Two launches per 256 queries on `stream` (scan: blocks of rows_per_block rows x tile of 8, 4, 2 or 1 queries, chosen from M so that a
 * tile's tables and key lists take at most 80 KiB of LDS; merge: one block per query over any number of partial lists), no host
 * synchronisation, integer work only, no global atomics.  A query's outputs depend on its own table, codes and allow; not on the batch,
 * its order, the tile it lands in, the launch shape or the workspace.  n_rows = 0 is legal (all -1, counts 0; the scan is not
 * launched) and so is n_queries = 0 (nothing is launched).
 * ARX_ERR_ARG before anything is launched, the message naming the field: n_candidates outside 1..256; dim, dsub or M outside the
 * shapes above; n_rows outside 0..2^31-1; n_queries < 0; a null or misaligned pointer; ws_bytes below the figure above.
 * codes, lut and allow are device data of which every bit pattern is legal: nothing read from them addresses anything out of range.
 * THE EXACT RESCORE is arx_ivf_search over the candidate lists, composed exactly as for arx_binary_candidates above. */
int64_t arx_pq_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t dsub, int32_t n_candidates);
int32_t arx_pq_candidates(const uint8_t* codes, int64_t n_rows, int32_t dim, int32_t dsub, const uint8_t* lut, int32_t n_queries,
                          const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_sum, int64_t* out_count, void* ws,
                          int64_t ws_bytes, void* stream);
/* The same with the scan's launch shape chosen: rows_per_block as for arx_binary_candidates_tuned.  Same bits for every choice. */
int32_t arx_pq_candidates_tuned(const uint8_t* codes, int64_t n_rows, int32_t dim, int32_t dsub, const uint8_t* lut, int32_t n_queries,
                                const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_sum, int64_t* out_count,
                                void* ws, int64_t ws_bytes, int32_t rows_per_block, void* stream);

/* ---- Graph search: beam search over a fixed-degree k-NN graph, exact scores (csrc/graph.hip; the host layer and the numpy restatement
 * `search_host` are arxiv_rag_amd/graph.py; the definition is INTEGRATION.md "Graph search") --------------------------------------------
 *   corpus        device fp16 [n_rows, dim], 16-byte aligned; queries device fp16 [n_queries, dim], 16-byte aligned
 *   neighbors     device int32 [n_rows, degree], degree a multiple of 8 in 8..64; an entry outside [0, n_rows) is "no edge"
 *   entries       device int32 [n_queries, n_entries], n_entries in 1..64; an entry outside [0, n_rows) is skipped
 *   allow         device uint64 [ceil(n_rows / 64)] or NULL: arx_topk_search_filtered's convention (bit r & 63 of word r >> 6)
 *   k in 1..32, ef in k..512, max_iters in 1..1024
 *   out_scores    device f32 [n_queries, k]; out_ids device int64 [n_queries, k]; out_scored, out_expanded device int64 [n_queries] or NULL
 *   ws            device scratch of arx_graph_workspace_bytes(...) bytes (-1 for arguments outside the limits below)
 * Per query, with a visited set (exact set semantics), a beam of at most ef (score, row) pairs ordered by (score desc, row asc) and an
 * "expanded" mark per beam row.  A row's score is exact_row_score (csrc/exact_score.h) against the query, the bits of arx_topk_search; a
 * NaN score ranks below every number (among NaNs: row asc) and comes back as the quiet NaN 0x7fc00000.
 *   start    the distinct valid entry rows become visited, are scored and merged into the beam, which is cut to its best ef
 *   iterate  at most max_iters times: the parent is the best beam row not yet expanded (none: stop); it is marked expanded; each of its
 *            neighbours that is valid and not yet visited becomes visited and is scored; the new pairs are merged into the beam, which
 *            is cut to ef.  A row that falls off the beam stays visited and is never scored again.
 *   answer   without allow the first k of the beam; with allow the best k by (score desc, row asc) among ALL rows scored whose bit is
 *            set (the walk ignores the bitmap: hidden rows stay bridges).  Missing places are (-inf, -1); ids are row + idx_base.
 *   out_scored[q] the rows scored, out_expanded[q] the iterations run.
 * One launch on `stream`, one block per query, all state in LDS (the workspace is not written): a query's outputs depend on its row of
 * queries and entries, the graph, allow and the corpus; not on the batch or the launch shape.  The visited set is an open-addressing
 * table of 16384 slots filled by integer LDS compare-and-swap, the only atomics; it holds at most 8192 rows, and a call whose
 * n_entries + max_iters * degree exceeds 8192 is refused: the table never drops a row.
 * ARX_ERR_ARG before the launch, the message naming the field: any of the ranges above; n_entries + max_iters * degree > 8192; dim not a
 * multiple of 64 or above 8192; n_rows outside 1..2^31-1; n_queries < 1; a null or misaligned pointer; ws_bytes below the figure above.
 * neighbors, entries and allow are device data: bad values give the defined answer above and never an access out of range. */
int64_t arx_graph_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t degree, int32_t k, int32_t ef, int32_t max_iters,
                                  int32_t n_entries);
int32_t arx_graph_search(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* neighbors, int32_t degree, const void* queries,
                         int32_t n_queries, const int32_t* entries, int32_t n_entries, const uint64_t* allow, int32_t k, int32_t ef,
                         int32_t max_iters, float* out_scores, int64_t* out_ids, int64_t* out_scored, int64_t* out_expanded, int64_t idx_base,
                         void* ws, int64_t ws_bytes, void* stream);
/* The same with the block size chosen: threads 0 (default: 256, or 128 for degree <= 16), 64, 128 or 256; a block scores threads / 8
 * rows per pass.  Same bits for every choice. */
int32_t arx_graph_search_tuned(const void* corpus, int64_t n_rows, int32_t dim, const int32_t* neighbors, int32_t degree, const void* queries,
                               int32_t n_queries, const int32_t* entries, int32_t n_entries, const uint64_t* allow, int32_t k, int32_t ef,
                               int32_t max_iters, float* out_scores, int64_t* out_ids, int64_t* out_scored, int64_t* out_expanded,
                               int64_t idx_base, void* ws, int64_t ws_bytes, int32_t threads, void* stream);

/* ---- Graph maintenance: link new rows into a built graph, renumber it after a compaction (csrc/graph.hip; the host layer and the numpy
 * restatements `link_host`, `remap_host`, `insert_host` are arxiv_rag_amd/graph.py; INTEGRATION.md "Graph search", "Keeping the graph") ---
 * arx_graph_link offers rows to the tails of other rows' neighbour lists.
 *   corpus        device fp16 [n_rows, dim], 16-byte aligned; dim a multiple of 64, at most 8192
 *   neighbors     device int32 [n_rows, degree], read and written; degree a multiple of 8 in 8..64
 *   targets       device int32 [n_targets]; offer_start device int32 [n_targets + 1]; offers device int32 [n_offers], n_offers < 2^31 - 64:
 *                 slot s offers the rows offers[offer_start[s] .. offer_start[s + 1]) to row targets[s]
 * With H = degree / 2, an entry being valid when it lies in [0, n_rows), for every slot s with t = targets[s]:
 *   head     neighbors[t][0 .. H) is left exactly as it is
 *   pool     the valid entries of neighbors[t][H .. degree) and the valid rows among the slot's offers, without t and without the head's
 *            valid entries; a row named several times is in the pool once
 *   key      of pool row c:  order word of exact_row_score(row c, query = row t) << 32 | (0xffffffff - c), the keys of arx_graph_search:
 *            score desc, row asc, a NaN score below every number
 *   tail     neighbors[t][H .. degree) becomes the rows of the pool's degree - H largest keys in descending order, padded with -1
 * A slot is skipped, its row left untouched, when t lies outside [0, n_rows), when t is not strictly greater than every t inside
 * [0, n_rows) of the slots before it (with ascending targets: the previous slot's; so no two blocks ever write one row), or when its
 * offer_start pair is negative, decreasing or beyond n_offers.  targets, offer_start, offers and neighbors are device data: bad values give the answer
 * above and never an access out of range.
 * One launch on `stream`, one block per slot, plain stores only: no atomics, no workspace.  A target's new tail depends on the corpus,
 * its own old row and its own offers alone; the offers are taken 64 at a time and merged into the running tail, and because the tail is
 * the top of a SET the result depends neither on that chunking nor on the launch shape.
 * ARX_ERR_ARG before the launch, the message naming the field: degree, dim, n_rows outside 1..2^31-1, n_targets < 0 (0: nothing to do),
 * n_offers outside the range above, a null or misaligned pointer. */
int32_t arx_graph_link(const void* corpus, int64_t n_rows, int32_t dim, int32_t* neighbors, int32_t degree, const int32_t* targets,
                       int32_t n_targets, const int32_t* offer_start, const int32_t* offers, int64_t n_offers, void* stream);
/* The same with the block size chosen: threads as for arx_graph_search_tuned.  Same bits for every choice. */
int32_t arx_graph_link_tuned(const void* corpus, int64_t n_rows, int32_t dim, int32_t* neighbors, int32_t degree, const int32_t* targets,
                             int32_t n_targets, const int32_t* offer_start, const int32_t* offers, int64_t n_offers, int32_t threads,
                             void* stream);
/* arx_graph_remap renumbers a graph after a stable compaction.  neighbors: device int32 [count, degree], the kept rows already moved by
 * arx_compact_rows (rows of 4 * degree bytes); keep, word_rank: the bitmap and the plan of arx_compact_plan over the n_old rows there
 * were (n_old < 2^31, count <= n_old).  Every entry e is rewritten in place: a valid one (in [0, n_old)) whose keep bit is set becomes
 * word_rank[e >> 6] + popcount(keep[e >> 6] & the bits below e & 63); any other is dropped (as is one whose new number would not lie in
 * [0, count): a plan that is not this bitmap's).  A row's surviving entries move to its front in their old order, the rest become -1.
 * One launch on `stream`, a wave per row, plain stores; any bit pattern in the rows is legal.  ARX_ERR_ARG: degree, n_old, count, a null
 * pointer (count = 0: nothing to do). */
int32_t arx_graph_remap(int32_t* neighbors, int64_t count, int32_t degree, const uint64_t* keep, const int64_t* word_rank, int64_t n_old,
                        void* stream);

/* ---- MMR diversified re-ordering of a query's search candidates (csrc/mmr.hip; the definition is INTEGRATION.md "MMR") -----------
 * arx_gather_rows: out[s] (device fp16 [count, dim]) = shard row ids[s] - idx_base where that row lies in [0, n_rows), all zeros
 * otherwise (id -1, a row another rank owns: the ranks' buffers then add up to the rows, arxiv_rag_amd/mmr.py).  shard device fp16
 * [n_rows, dim], ids device int64 [count] (the [Q, n] list of a search, global ids), dim % 8 == 0.  Every output element is written once
 * with a plain 16-byte store: the result does not depend on what the buffer held before.  One launch on `stream`, no atomics. */
int32_t arx_gather_rows(const void* shard, int64_t n_rows, int32_t dim, int64_t idx_base, const int64_t* ids, int64_t count,
                        void* out, void* stream);
/* arx_mmr_select: per query, greedy maximal marginal relevance over its n <= 32 candidate slots (in search order).
 *   q device fp16 [n_queries, dim]; cand device fp16 [n_queries, n, dim] (what arx_gather_rows wrote); ids device int64 [n_queries, n]:
 *   a slot with id < 0 is never picked and counts as a zero row.  dim % 64 == 0, dim <= 8192, 1 <= m <= n <= 32, lambda in [0, 1].
 *   rel[i] = cos(q, c_i), sim[i][j] = cos(c_i, c_j): true cosines (rows of any norm; 0 where a norm is 0), every dot product an f32 sum
 *   of exact fp16 products.  Pick 0 = argmax lambda rel[i]; pick t = argmax over valid unpicked i of
 *   lambda rel[i] - (1 - lambda) max_{j picked} sim[i][j]; ties to the lower slot.
 *   order device int32 [n_queries, m]: the picked SLOT positions; mmr device f32 [n_queries, m]: the objective at the time of the pick;
 *   (-1, -inf) in the tail when fewer than m slots are valid.
 * One block per query, no atomics, no workspace: a query's outputs depend on its own row of q, cand and ids alone, bit for bit. */
int32_t arx_mmr_select(const void* q, const void* cand, const int64_t* ids, int32_t n_queries, int32_t n, int32_t dim, int32_t m,
                       float lambda, int32_t* order, float* mmr, void* stream);

/* ---- BM25 keyword top-n (hybrid search: `retrieval.use_hybrid_search`, 3-chunks/pipeline/config.yaml:67-68) ----------------
 * Index of one shard, device memory, built by the caller (arxiv_rag_amd/keyword.py):
 *   term_ptr int64 [vocab + 1]   CSR by term: postings of term t are [term_ptr[t], term_ptr[t + 1])
 *   post_row uint32 [P]          shard-local row of the posting, strictly ascending within a term
 *   post_w   f32 [P]             its impact idf(t) * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl)) > 0 (float64 on the host, rounded once)
 * A query is its distinct term ids: q_terms device int32 [n_queries, 64], strictly ascending, -1 padded; q_nterms device int32
 * [n_queries], each in 0..64 (ascending order and ids inside [0, vocab) are the caller's contract; a term outside the vocabulary has
 * no postings).  bm25(q, d) = sum of the impacts of q's terms in d, added in ascending term order in f32 without atomics: a row's
 * score depends on the index and the query's terms only, never on the tile size, the block count or the other queries of the call.
 * Output, per query: the n <= 32 rows with the largest (score desc, row asc) among rows holding at least one query term, as
 * (f32 score, int64 idx_base + row); unused slots are (-inf, -1), the convention of arx_topk_search, so per-shard lists merge
 * through arx_topk_merge.
 * One kernel serves this call, the filtered calls and arx_bm25_search_wide below (csrc/bm25.hip): a block walks row tiles, keeps its
 * candidates as 64-bit keys (score bits, then the inverted row) in a 4096-key LDS list that one cut function brings back to its n
 * largest (rounds of a block-wide maximum for n <= 32, a block-wide sort beyond), and with more than one block per query (blocks = min(tiles, 512, 4096 / n[, max_blocks])) the blocks' sorted lists are
 * merged by one kernel of the call's own, one block per query.  The keys are distinct, so the answer is one set in one order.
 * ws: device scratch of arx_bm25_workspace_bytes(n_rows, n_queries, n) bytes
 *   = round_up(min(ceil(n_rows / 1024), 512, 4096 / n) * n_queries * n * 8, 256)   (the per-block lists as 64-bit keys, sized for the
 * smallest tile); may be NULL when the call runs one block per query.  The function returns -1 for n_rows <= 0, n_queries <= 0,
 * n < 1 or n > 32. */
int64_t arx_bm25_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n);
int32_t arx_bm25_search(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                        const int32_t* q_terms, const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores,
                        int64_t* out_ids, int64_t idx_base, void* ws, int64_t ws_bytes, void* stream);
/* The same search with the launch shape chosen by the caller (tests, tuning): tile_rows = accumulator rows per LDS tile (a multiple
 * of 1024 in [1024, 12288]; 0 = default), max_blocks = cap on the blocks per query (0 = default).  Same bits for every choice. */
int32_t arx_bm25_search_tuned(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                              const int32_t* q_terms, const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores,
                              int64_t* out_ids, int64_t idx_base, void* ws, int64_t ws_bytes, int32_t tile_rows, int32_t max_blocks,
                              void* stream);
/* Filtered BM25 top-n (hybrid search under `where` / `where_document` / the dedup keep-bitmap; opt-in: `hybrid_filters=True`,
 * --hybrid-filters).  arx_bm25_search restricted to allowed rows, with a filter per query:
 *   allow     device uint64 [n_filters][ceil(n_rows / 64)], the bitmap convention of arx_topk_search_filtered (bit r & 63 of word
 *             r >> 6 = row r allowed); bits at or beyond n_rows may be garbage and are ignored.  n_filters >= 1, and the 64-filter
 *             limit of arx_topk_search_filtered_multi does not apply: each block of the kernel serves one query.
 *   filter_of device int32 [n_queries]: the bitmap of each query; NULL = every query uses bitmap 0.  A query whose filter_of lies
 *             outside [0, n_filters) sees no row: its output is all (-inf, -1) and nothing is read out of range (tested on the device).
 * Output, per query q: the n <= 32 rows with the largest (score desc, row asc) among rows that hold at least one query term AND are
 * allowed by allow[filter_of[q]].  A row's score has exactly the bits arx_bm25_search / arx_bm25_scores give it: the impacts are
 * untouched, so idf and avgdl stay statistics of the WHOLE corpus, as a Lucene filter clause leaves them.  A query's output depends
 * on the query, its own bitmap and the index only: not on the other queries, their filters, n_filters, tile_rows or max_blocks.
 * Kernel, cut, merge, padding and workspace (arx_bm25_workspace_bytes) are those of arx_bm25_search; the bitmap words of a tile are
 * staged in LDS and a key is appended only when its row's bit is set.  ARX_ERR_ARG before any launch: a null allow, n_filters < 1,
 * and every argument error of arx_bm25_search.
 * Cost: a tile (<= 12288 rows) without an allowed row is skipped, with its binary searches and posting reads; a tile with one is
 * streamed whole.  So a contiguous filter saves bandwidth and a scattered one does not, however selective: a doc-at-a-time path for
 * those is out of scope. */
int32_t arx_bm25_search_filtered(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                                 const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const int32_t* q_terms,
                                 const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores, int64_t* out_ids,
                                 int64_t idx_base, void* ws, int64_t ws_bytes, void* stream);
int32_t arx_bm25_search_filtered_tuned(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab,
                                       int64_t n_rows, const uint64_t* allow, int32_t n_filters, const int32_t* filter_of,
                                       const int32_t* q_terms, const int32_t* q_nterms, int32_t n_queries, int32_t n,
                                       float* out_scores, int64_t* out_ids, int64_t idx_base, void* ws, int64_t ws_bytes,
                                       int32_t tile_rows, int32_t max_blocks, void* stream);
/* Wide BM25 top-n: n in [1, 1024], with an optional row filter (hybrid search with candidate lists longer than 32; opt-in:
 * `hybrid_on_device=True`, --hybrid-on-device).  The kernel, cut and merge of arx_bm25_search and arx_bm25_search_filtered with two
 * other limits: n <= 1024, and blocks * n <= 65536 instead of 4096.  Index, queries, scores and filter are theirs:
 *   allow == NULL   the unfiltered search (n_filters is ignored and filter_of must be NULL);
 *   allow != NULL   device uint64 [n_filters][ceil(n_rows / 64)] with filter_of device int32 [n_queries] or NULL (= bitmap 0), in the
 *                   convention of arx_bm25_search_filtered: an index outside [0, n_filters) gives that query no row and reads nothing,
 *                   bits at or beyond n_rows are ignored, a tile without an allowed row is skipped before its binary searches.
 * Scores: the impacts of the query's terms added in ascending term order in f32, no float atomics: a row's score has the bits
 * arx_bm25_search and arx_bm25_scores give it, whatever tile_rows, max_blocks and the other queries of the call are.
 * Output, per query: the n rows with the largest (score desc, row asc) among the (allowed) rows holding a query term, as (f32 score,
 * int64 idx_base + row); unused slots are (-inf, -1).  For n <= 32 the output equals arx_bm25_search / arx_bm25_search_filtered bit
 * for bit, and for m < n the first m entries of the n-list are the m-list.
 * blocks = min(tiles, 512, 65536 / n[, max_blocks]), 64 blocks at n = 1024.
 * tile_rows: accumulator rows per LDS tile, a multiple of 1024 in [1024, 12288]; 0 = default (min(round_up(n_rows, 1024), 10240): two
 * blocks per CU; the default of every BM25 call).  max_blocks: cap on the blocks per query (0 = default).
 * ws: device scratch of arx_bm25_wide_workspace_bytes(n_rows, n_queries, n) bytes
 *   = round_up(min(ceil(n_rows / 1024), 512, 65536 / n) * n_queries * n * 8, 256)   (the per-block lists as 64-bit keys);
 * may be NULL when the call runs one block per query.  The function returns -1 for n_rows <= 0, n_queries <= 0, n < 1 or n > 1024.
 * ARX_ERR_ARG before any launch: a null pointer, filter_of without allow, n_filters < 1 with allow, vocab <= 0, n_rows outside
 * [1, 2^31), n_queries outside [1, 65535], n outside [1, 1024], idx_base < 0, max_blocks < 0, a tile_rows that is not as above, a
 * workspace that is too small. */
int64_t arx_bm25_wide_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n);
int32_t arx_bm25_search_wide(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                             const uint64_t* allow, int32_t n_filters, const int32_t* filter_of, const int32_t* q_terms,
                             const int32_t* q_nterms, int32_t n_queries, int32_t n, float* out_scores, int64_t* out_ids,
                             int64_t idx_base, void* ws, int64_t ws_bytes, int32_t tile_rows, int32_t max_blocks, void* stream);
/* Relative-score fusion of a dense and a keyword candidate list per query, on the device: arxiv_rag_amd/keyword.py `fuse`, bit for bit.
 *   dense_scores f32 / dense_ids int64 [n_queries, n_dense], kw_scores f32 / kw_ids int64 [n_queries, n_kw] (device); a slot with
 *   id < 0 is unused.  n_dense, n_kw and k each in [1, 1024]; alpha in [0, 1]; no workspace.
 *   PRECONDITION: the ids >= 0 of one list of one query are distinct (every search of this library returns such lists), and below
 *   2^63 - 1.  Ids are compared as int64: they may exceed 2^32.
 * Per list, in float64, norm = (s - min) / (max - min) over its used slots, 1.0 for every one of them when max == min; a row absent
 * from a list gets 0.0 from that side; fused = alpha * normD + (1.0 - alpha) * normK as two separately rounded products and one sum
 * (no FMA contraction).  Output, per query: the best k rows of the union by (fused desc, id asc) as out_fused f64, out_ids int64,
 * out_dense f32, out_kw f32 [n_queries, k]; out_dense / out_kw are NaN where the row was not in that list; unused slots are
 * (-inf, -1, NaN, NaN).  Every output element is written.  One block per query, no atomics: a query's output depends on its own two
 * lists, alpha and k alone. */
int32_t arx_hybrid_fuse(const float* dense_scores, const int64_t* dense_ids, int32_t n_dense, const float* kw_scores,
                        const int64_t* kw_ids, int32_t n_kw, int32_t n_queries, double alpha, int32_t k, double* out_fused,
                        int64_t* out_ids, float* out_dense, float* out_kw, void* stream);
/* Debug tap: out (device f32 [row_hi - row_lo]) = the score of ONE query (q_terms device int32 [n_terms], ascending) for every row of
 * [row_lo, row_hi), 0 where the row holds none of its terms; the accumulation is the search's own. */
int32_t arx_bm25_scores(const int64_t* term_ptr, const uint32_t* post_row, const float* post_w, int32_t vocab, int64_t n_rows,
                        const int32_t* q_terms, int32_t n_terms, int64_t row_lo, int64_t row_hi, int32_t tile_rows, float* out,
                        void* stream);
/* The BM25 index built on the device (opt-in: `KeywordIndex(build_on_device=True)`, `keyword_build_on_device=True`,
 * --keyword-build-on-device; csrc/bm25_build.hip).  arx_bm25_build_postings computes keyword.py `build_postings`, bit for bit:
 *   pieces   device int32 [n_tokens]: the word-piece ids of every document, concatenated in row order
 *   doc_ptr  device int64 [n_docs + 1], non-decreasing, doc_ptr[0] = 0, doc_ptr[n_docs] = n_tokens: document r is pieces[doc_ptr[r] ..
 *            doc_ptr[r + 1]) (the caller's contract)
 *   term_ptr device int64 [vocab + 1], post_row device uint32 and post_tf device int32, each with room for n_tokens entries: the
 *            layout above, rows strictly ascending within a term, post_tf = occurrences of the term in the row; the first *n_postings
 *            entries are written and nothing beyond them
 *   n_postings device int64: P, the number of postings;  bad_id device int32: non-zero when any id lies outside [0, vocab).  Such an
 *            id is sorted as term 0, so nothing is read or written out of range; the other outputs then mean nothing.
 * A stable LSD radix sort by term id (8-bit digits, the row as payload; tokens arrive in row order), then the heads of equal
 * (term, row) runs are numbered.  Integer LDS atomics in the digit histograms only; no global and no float atomics; bad_id is a plain
 * store.  The output is one defined array set: it does not depend on tile_tokens or max_blocks.
 * n_tokens == 0 or n_docs == 0: term_ptr is all zero, P is 0, and no kernel is launched.
 * ws: device scratch of arx_bm25_build_workspace_bytes(n_tokens, n_docs, vocab) bytes
 *   = 4 * round_up(4 * n_tokens, 256) + 4 * 256 * 2048   (two (key, row) pairs the passes alternate between, and the digit counts of up
 * to 2048 blocks); the function returns -1 outside the limits below.
 * ARX_ERR_ARG before any launch: a null pointer, n_tokens outside [0, 2^31), n_docs outside [0, 2^32), vocab outside [1, 2^24], a
 * workspace that is too small.
 * _tuned: the launch shape is the caller's (tests, tuning).  tile_tokens: a block's chunk of tokens is a whole number of tiles of this
 * size, a multiple of 256 in [256, 65536] (0 = default, 2048); max_blocks: cap on the blocks, at most 2048 (0 = default, 2048). */
int64_t arx_bm25_build_workspace_bytes(int64_t n_tokens, int64_t n_docs, int32_t vocab);
int32_t arx_bm25_build_postings(const int32_t* pieces, int64_t n_tokens, const int64_t* doc_ptr, int64_t n_docs, int32_t vocab,
                                int64_t* term_ptr, uint32_t* post_row, int32_t* post_tf, int64_t* n_postings, int32_t* bad_id,
                                void* ws, int64_t ws_bytes, void* stream);
int32_t arx_bm25_build_postings_tuned(const int32_t* pieces, int64_t n_tokens, const int64_t* doc_ptr, int64_t n_docs, int32_t vocab,
                                      int64_t* term_ptr, uint32_t* post_row, int32_t* post_tf, int64_t* n_postings, int32_t* bad_id,
                                      void* ws, int64_t ws_bytes, int32_t tile_tokens, int32_t max_blocks, void* stream);
/* post_w f32 [n_postings] = keyword.py `impacts_f64(...).astype(float32)`, bit for bit, from the arrays above (n_postings as the host
 * read it), idf device f64 [vocab] (`keyword.idf_f64` of the statistics in force, computed on the host: with global statistics their
 * all-reduce sits between the two calls) and avgdl.  Per posting s of term t (the last t with term_ptr[t] <= s) and row r, in float64
 * and in numpy's operation order, without FMA contraction, rounded once to f32 (k1 = 1.2, b = 0.75):
 *   dl = doc_ptr[r + 1] - doc_ptr[r];  norm = k1 * ((1.0 - b) + (b * dl) / avgdl);  w = ((idf[t] * tf) * (k1 + 1.0)) / (tf + norm)
 * ARX_ERR_ARG before any launch: a null pointer, n_postings outside [0, 2^31), n_docs outside [0, 2^32), vocab outside [1, 2^24], a
 * negative or NaN avgdl.  n_postings == 0 launches nothing. */
int32_t arx_bm25_build_impacts(const int64_t* term_ptr, const uint32_t* post_row, const int32_t* post_tf, int64_t n_postings,
                               const int64_t* doc_ptr, int64_t n_docs, const double* idf, int32_t vocab, double avgdl, float* post_w,
                               void* stream);

/* Raw linear layer of the path: C[M,N] (bf16) = epi(A[M,K] (bf16) x W[N,K]^T (bf16) + bias[N] (f32)),
 * mode 0 = bias, 1 = bias + erf-GELU, 2 = bias + resid[M,N] (bf16).  K % 64 == 0, N % 8 == 0.
 * `variant` selects the main-loop schedule (ARX_GEMM_*); exposed for unit tests and tuning. */
int32_t arx_gemm_bf16(const void* A, const void* W, const float* bias, const void* resid, void* C,
                      int32_t M, int32_t N, int32_t K, int32_t mode, int32_t variant, void* stream);

/* Parity tap: the same linear layer with ANY epilogue mode of the forward (csrc/gemm.h), launched exactly as the encoder launches it:
 *   mode 0-2 as above;
 *   3 = rstd_m (acc - mean_m s_n) + c_n   (LayerNorm folded into the weights; `bias` is the folded c vector);   4 = GELU of mode 3;
 *   5 = acc + b_n + resid, and the output rows' LayerNorm statistics;   6 = acc + b_n + LN(resid), LN rebuilt from (r_mean, r_rstd,
 *   r_gamma, r_beta), and the statistics.
 * Statistics (modes 5/6; N % 64 == 0) are those of the bf16-ROUNDED output.  Tile kernels (variants 89, 8, 9, 13, 71) write per-row
 * partial (sum, sum of squares) of 64-column slice j to part_sum / part_sq [j * part_ld + m], j < N / 64, m < M (nothing else of the slabs
 * is written), then ln_finalize_kernel writes out_mean / out_rstd [m] for m < *n_rows (a device int32, as in the forward) with
 * mean = sum / N, rstd = rsqrt(max(sumsq / N - mean^2, 0) + eps).  Variant 70 (M <= 256; statistics N <= 1024) writes out_mean / out_rstd
 * itself and no slab.  Per-row input vectors hold row_cap floats: >= M, and >= M rounded up to 256 for variants 89, 8, 9, which stage a
 * whole tile's rows at once (rows >= M are read, never used).  A pointer a mode needs and does not get, an unknown mode or variant, or
 * a shape a kernel refuses is ARX_ERR_ARG, before anything is launched.  Device pointers throughout; no host synchronisation. */
typedef struct {
    int32_t struct_bytes;               /* sizeof(arx_gemm_epilogue) */
    int32_t mode;                       /* 0..6 */
    int32_t variant;                    /* ARX_GEMM_*: 89, 8, 9, 13, 70, 71 */
    float eps;                          /* LayerNorm epsilon of the output statistics (modes 5/6) */
    const float* bias;                  /* [N]; modes 3/4: the folded c vector */
    const void* resid;                  /* bf16 [M, N]: modes 2/5/6 */
    const float *a_mean, *a_rstd;       /* [row_cap]: statistics of the A operand's rows (modes 3/4) */
    const float* s_vec;                 /* [N]: s_n = sum_k W'[n][k] (modes 3/4) */
    const float *r_mean, *r_rstd;       /* [row_cap]: statistics of the residual's rows (mode 6) */
    const float *r_gamma, *r_beta;      /* [N]: LayerNorm affine of the residual (mode 6) */
    int64_t row_cap;
    float *part_sum, *part_sq;          /* [N / 64][part_ld] (modes 5/6, tile kernels) */
    int64_t part_ld;                    /* >= M */
    float *out_mean, *out_rstd;         /* [M] (modes 5/6) */
    const int32_t* n_rows;              /* device int32: rows ln_finalize_kernel covers (modes 5/6, tile kernels) */
} arx_gemm_epilogue;
int32_t arx_gemm_bf16_ex(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, const arx_gemm_epilogue* e, void* stream);

/* Parity tap: fold_ln_kernel alone, the fold arx_encoder_create applies to the weights that consume a LayerNorm output.
 * W bf16 [N, K], gamma / beta f32 [K], bias f32 [N] -> Wf bf16 [N, K] = bf16(W[n][k] gamma[k]), s[n] = sum_k Wf[n][k],
 * c[n] = bias[n] + sum_k beta[k] W[n][k]. */
int32_t arx_fold_ln(const void* W, const float* gamma, const float* beta, const float* bias, void* Wf, float* s, float* c,
                    int32_t N, int32_t K, void* stream);

/* out[i] = cos(emb[i], emb[i+1]) for i in [0, n-1): the adjacent-sentence similarity the stage-3 semantic chunker
 * thresholds (/root/reference/3-chunks/pipeline/src/processors/text_processor.py:1555-1561, helper :1601-1605).
 * emb device f32 [n, ld >= dim]; out device f32 [n-1]. */
int32_t arx_adjacent_cosine(const float* emb, int64_t ld, int32_t n, int32_t dim, float* out, void* stream);

/* ---- host-side WordPiece feeder (no device code) ------------------------------------------------------------------------------
 * Replaces, for pure-ASCII texts, the tokenisation sentence-transformers performs inside `model.encode(batch, ...)`
 * (/root/reference/4-embed/generation/generate_embeddings_parallel.py:146-153; HF `tokenizers` pipeline BertNormalizer ->
 * BertPreTokenizer -> WordPiece("##") -> "<bos> $A <eos>" -> truncation, transformers models/mpnet/tokenization_mpnet.py:108-163).
 * Texts containing one of the `triggers` (the tokenizer's added-token strings) are FLAGGED, not tokenised: the caller sends them
 * through the reference pipeline; non-ASCII segments go through a cache of that pipeline's output (below).  Multi-threaded; writes a
 * padded id matrix and lengths directly. */
int32_t arx_wp_create(const char* vocab_blob, const int64_t* vocab_off /* [n_vocab+1] */, int32_t n_vocab, int32_t unk_id,
                      int32_t bos_id, int32_t eos_id, int32_t pad_id, int32_t lowercase, int32_t max_chars_per_word,
                      const char* trigger_blob, const int64_t* trigger_off /* [n_triggers+1] */, int32_t n_triggers, void** out);
void arx_wp_destroy(void* tokenizer);
/* ids: host int32 [n, max_len] (rows padded with pad_id), lens: host int32 [n], fallback: host uint8 [n] (1 = not tokenised here) */
int32_t arx_wp_encode(void* tokenizer, const char* text_blob, const int64_t* text_off /* [n+1] */, int64_t n, int32_t max_len,
                      int32_t* ids, int32_t* lens, uint8_t* fallback, int32_t n_threads);
/* fallback[i]: 0 = tokenised; 1 = send the whole text through the reference pipeline (added-token string present, or a non-ASCII
 * run > 512 bytes); 2 = the text has non-ASCII whitespace-delimited segments the tokenizer has not been taught yet: fetch them
 * (arx_wp_miss_count / arx_wp_miss_fetch), tokenise each ONCE with the reference pipeline (no specials, no truncation), hand the
 * pieces back (arx_wp_cache_add) and encode those texts again.  tokens(text) is the concatenation of tokens(segment) because every
 * stage of the pipeline is local to a whitespace-delimited segment. */
int32_t arx_wp_miss_count(void* tokenizer, int64_t* n_strings, int64_t* n_bytes);
int32_t arx_wp_miss_fetch(void* tokenizer, char* blob, int64_t* off /* [n_strings+1] */);
int32_t arx_wp_cache_add(void* tokenizer, const char* seg_blob, const int64_t* seg_off /* [n+1] */, int64_t n, const int32_t* ids,
                         const int64_t* ids_off /* [n+1] */);
int64_t arx_wp_cache_size(void* tokenizer);
int32_t arx_wp_version(void);

/* ---- small device helpers the host code needs (all on `stream`) -------------------------------- */
/* f32 [n] -> bf16 [n] round-to-nearest-even (weight upload). */
int32_t arx_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* L2-normalised N(0,1) rows in fp16, generated on device from (seed, row index): bench cfg 3. */
int32_t arx_fill_unit_rows_f16(void* dst, int64_t n_rows, int32_t dim, uint64_t seed, void* stream);
/* The same generator for a row RANGE of a larger corpus: dst row j = row (row_base + j) of the corpus arx_fill_unit_rows_f16 would
 * write for this seed — every rank of a sharded bench fills its own slice of ONE corpus (bench cfg 4: 5 M rows cut 8 ways), so that
 * the merged answer can be checked against a single-index search of the same rows. */
int32_t arx_fill_unit_rows_f16_at(void* dst, int64_t n_rows, int32_t dim, uint64_t seed, int64_t row_base, void* stream);
/* EMBEDDING-LIKE synthetic rows (bench: search on something harder than iid Gaussian directions): row r belongs to cluster
 * hash(seed, r) % n_clusters and is centre(cluster) + spread * noise(r), both N(0,1) per dimension times a per-dimension gain that is
 * hot_gain on n_hot_dims dimensions chosen by the seed (outlier dimensions: they set max|x| and with it the int8 scale of every row)
 * and 1 elsewhere; L2-normalised, fp16.  Rows of the same seed share the centres whatever row_base is, so queries drawn with a
 * row_base beyond the corpus are new points of the same mixture.  n_clusters < 0 = TOPIC ORDER: cluster(r) = r / (-n_clusters), i.e.
 * consecutive runs of -n_clusters rows share a centre (the chunks of one paper: neighbours in row order and in embedding space — whole
 * 64-row groups of near-tied rows, the hard layout for group-max selection).  dim % 128 == 0, dim <= 1024. */
int32_t arx_fill_clustered_rows_f16_at(void* dst, int64_t n_rows, int32_t dim, uint64_t seed, int64_t row_base, int32_t n_clusters,
                                       float spread, int32_t n_hot_dims, float hot_gain, void* stream);

/* ---- live per-kernel timing (bench.py roofline leg) ----------------------------------------------
 * When enabled, every launch of a hot kernel class is bracketed by hipEvents recorded on the launch
 * stream; arx_prof_read synchronises on them and returns the summed device time and launch count. */
#define ARX_K_SEARCH_GROUPMAX 0    /* search pass A: f16 MFMA GEMM + max over 64-row groups */
#define ARX_K_GEMM_QKV        1
#define ARX_K_GEMM_OPROJ      2
#define ARX_K_GEMM_FC1        3
#define ARX_K_GEMM_FC2        4
#define ARX_K_ATTENTION       5
#define ARX_K_LAYERNORM       6
#define ARX_K_EMBED           7
#define ARX_K_POOL            8
#define ARX_K_SEARCH_SELECT   9
#define ARX_K_SEARCH_RESCORE 10
#define ARX_K_GEMM_RAW       11    /* arx_gemm_bf16 called directly (unit tests, tuning): whatever its shape */
#define ARX_K_CLASSES        12
int32_t arx_prof_enable(int32_t on);
/* bit c set = kernel class c (ARX_K_*) records its event pair while profiling is on (default: all).  A timed run enables only the
 * class it reports, so that the other ~170 event packets per forward do not sit between the kernels being timed. */
int32_t arx_prof_classes(uint32_t mask);
int32_t arx_prof_reset(void);
int32_t arx_prof_read(int32_t kernel_class, float* total_ms, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* ARX_H */
