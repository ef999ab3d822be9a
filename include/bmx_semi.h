/* bmx_semi.h — semi-joins: bmx_where_semijoin, bmx_where_in and their sharded forms. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to
 * bmx.h. It brings bmx_where.h (the program: bmx_lit) with it.
 *
 * What it is for: a query that crosses one edge of the graph. "The orders whose userId is the uid of an active user", "the posts whose authorId belongs to
 * nobody who is banned", "the users whose team is one of these 30 000 team codes". Every other query of this library selects nodes by comparing their own
 * fields with constants the caller already holds; a set of 10^5 sparse keys is no range and does not fit the 32 literals of a program. Here one program builds a
 * set S of values on the device and a second program tests a field of its candidates against it; no list leaves the device in between.
 *
 * The set S.
 *   bmx_where_semijoin: the values of key_field on the nodes the INNER program (in_base_field, in_nclauses, in_clause_len, in_lits) selects. The inner program is
 *     a bmx_scan_where program: its universe is the positions of in_base_field's dense index whose row holds data, literal truth as in bmx_where.h. An inner node
 *     whose key row is absent or tombstoned counts in res->n_inner and adds nothing to S. key_field == in_base_field takes the value from the column and costs
 *     no probe; any other key_field costs one probe per selected inner node.
 *   bmx_where_in: the `nvalues` values given (1..BMX_SEMI_MAX_SET; nvalues takes the place of set_cap, so this form never overflows). Duplicates are allowed. A
 *     value outside +-(2^53 - 1) is no value any row can hold: it is skipped and not counted in res->n_inner (INT64_MIN is the table's empty word and is
 *     never inserted).
 * Selection: a node is selected iff the OUTER program (base_field, nclauses, clause_len, lits) selects it — exactly bmx_scan_where — AND its link_field row holds
 *   data whose value is in S. With BMX_SEMI_ANTI in `flags` the second condition is its exact complement (an anti-join): true for a link value outside S and true
 *   for an absent or tombstoned link, as BMX_LIT_NOT is. link_field == base_field reads the column and costs no probe; any other link_field costs one probe per
 *   node the outer program selects, also when the program has probed that field already.
 * The answer: the ids of the selected nodes in position order of base_field's index, at most `cap` of them; nothing is written at or beyond out_ids[cap].
 *   out_ids == NULL with cap == 0 counts only. res->n_match is exact whatever cap is; res->set_size is the number of distinct values in S; res->n_inner is the
 *   number of inner nodes selected, key present or not (bmx_where_in: the number of given values inside the domain, duplicates counted); res->reserved is 0.
 * Overflow: more than set_cap (1..BMX_SEMI_MAX_SET) distinct values. res->flags == BMX_SEMI_OVERFLOW, res->n_match == 0, res->set_size is some number > set_cap
 *   that is a lower bound of the distinct values, res->n_inner is still exact, and nothing is written to out_ids — for the anti form too: the "commit only if it
 *   fits" rule of bmx_watch_poll and bmx_where_group. The caller retries with more room or a narrower inner program.
 *   The context keeps a table of max(64, next power of two >= 2 * set_cap) key words for the largest set_cap asked so far, and set_cap words of staging.
 *
 * mem: BMX_MEM_HOST is synchronous; `values` is then a host array. BMX_MEM_DEVICE takes out_ids, res and values as device pointers and only enqueues: the probe
 *   sweep reads the overflow state on the device, res is written fully by the call's last kernel, in stream order, and no host round trip lies between the build
 *   and the probe. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched
 *   to its int64 column, on either side.
 * Value-ordered views: with a view on base_field or in_base_field (bmx_index_set_ordered) the call still takes the column path and leaves the view's bookkeeping
 *   untouched.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program, for either program (nclauses outside 1..8, a
 *   clause_len of 0 or above 8, more than 32 literals, more than 8 fields besides the base field, unknown literal flag bits, clause_len or lits NULL; the text
 *   says "outer program" or "inner program"); res NULL; set_cap or nvalues outside 1..BMX_SEMI_MAX_SET; values NULL; out_ids NULL with cap > 0; unknown bits in
 *   flags; link_field or key_field == BMX_AGG_NO_FIELD; a bad mem; a NULL context / communicator.
 * The sharded forms (host memory). A node's rows all live on the shard that owns its id, but a key may be held by inner nodes of several shards, and the node
 *   that links to it may live on yet another: S has to be the union. Phase 1 (bmx_comm_where_semijoin alone): every shard builds its own set with the caller's
 *   set_cap and exports it, all shards enqueued before the first list is fetched; the lists are united on the host (sort + unique). BMX_SEMI_OVERFLOW if any
 *   shard overflowed or the union has more than set_cap values; set_size is then the largest lower bound known. Phase 2: the union goes to every shard as
 *   bmx_where_in's values do, every shard's probe sweep is enqueued before the first answer is fetched, and the answers are collected shard after shard as
 *   bmx_comm_scan_where's are: the ids one context holding the same rows gives, in shard order. n_inner and n_match add up over the shards. */
#ifndef BMX_SEMI_H
#define BMX_SEMI_H
#include "bmx.h"
#include "bmx_where.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_semi_res {
  uint64_t n_match;   /* outer nodes selected, however small cap is; 0 on overflow */
  uint64_t set_size;  /* distinct values in the set; on overflow some number > set_cap, a lower bound */
  uint64_t n_inner;   /* semijoin: inner nodes selected (key present or not); where_in: values inside +-(2^53-1) */
  uint32_t flags;     /* BMX_SEMI_OVERFLOW */
  uint32_t reserved;  /* 0 */
} bmx_semi_res;       /* 32 bytes */
#define BMX_SEMI_ANTI      1u          /* select the complement on the link: anti-join */
#define BMX_SEMI_OVERFLOW  1u
#define BMX_SEMI_MAX_SET   (1u << 20)

int bmx_where_semijoin(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                       uint32_t link_field, uint32_t flags,
                       uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits, uint32_t key_field,
                       uint64_t set_cap, uint64_t* out_ids, uint64_t cap, bmx_semi_res* res, int mem);
int bmx_where_in(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                 uint32_t link_field, uint32_t flags, const int64_t* values, uint64_t nvalues,
                 uint64_t* out_ids, uint64_t cap, bmx_semi_res* res, int mem);
int bmx_comm_where_semijoin(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                            uint32_t link_field, uint32_t flags,
                            uint32_t in_base_field, uint32_t in_nclauses, const uint32_t* in_clause_len, const bmx_lit* in_lits, uint32_t key_field,
                            uint64_t set_cap, uint64_t* out_ids, uint64_t cap, bmx_semi_res* res);
int bmx_comm_where_in(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                      uint32_t link_field, uint32_t flags, const int64_t* values, uint64_t nvalues,
                      uint64_t* out_ids, uint64_t cap, bmx_semi_res* res);

#ifdef __cplusplus
}
#endif
#endif
