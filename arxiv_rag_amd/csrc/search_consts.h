// Constants of arx_topk_* shared by search.hip and the masked searches (filter.hip, prefix.hip): each includes this, then search_pass_a.h and
// search_tail.h (the masked searches also masked_topk.h).
#pragma once

#define GROUP_ROWS 64
#define KMAX 32                      // largest k
#define KSEL_SMALL 12                 // groups rescored when k <= 10 (k + 2: the certificate, not a margin, answers for exactness)
#define KSEL_BIG 36                   // groups rescored when k <= 32
#define SUPER 16                      // groups per super-group in the selection pass
#define SEL_SPLIT_WAVES 4            // waves per select block
#define QBATCH_MAX 1024              // queries per internal pass (bounds the gmax workspace)
#define AUX16_MAX_NQ 256              // fp16 pass: query batches up to this size (one 256-query tile) write aux words and take the single-row tail
#define TAIL_INBLOCK_MAX_SUPER 1024   // ... on shards of up to this many super-groups (1 M rows): there the block also selects for itself
#define SURV_CAP 256                 // int8 pipeline: rows at or above the threshold kept per query
#define CNT_QCOUNT 2                 // layout of the int8 candidate pipeline's counter block: see collect_pairs_kernel
#define CNT_QOVER (2 + QBATCH_MAX)
#define CNT_INTS (2 + 2 * QBATCH_MAX)
