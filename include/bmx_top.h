/* bmx_top.h — ordered, limited queries: bmx_scan_top and bmx_comm_scan_top. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next to bmx.h.
 *
 * What it replaces in the reference: docs/querying.md names "fields used for sorting" as the first reason to build an index, and "the 20 highest scores", "the
 * next page of products by price between 10 and 50", "the newest 100 posts of this author" are a range() (src/bullet-query.js:221-261) followed by a sort of
 * every match on the host. With the dense scans that is: deliver every matching id (8 bytes per match), fetch their values, sort. bmx_scan_top answers on the
 * device with the k records asked for; no match list exists at any point and nothing proportional to the match count is written anywhere.
 *
 * Selection: exactly bmx_scan_filter's and bmx_scan_aggregate's — an AND of 1..8 inclusive range terms over fields of the same node; term 0 runs on the index of
 *   terms[0].field (built or refreshed like any scan), the other terms are probed in the table; tombstones match no term; lo > hi matches nothing.
 * Order: by the value of terms[0].field, then by node id as an unsigned 64-bit number. The caller picks the order field by putting it first: "top 10 by score
 *   among admins" is [{score, -inf..inf}, {role, 3..3}]. Ascending is (val, id) ascending; BMX_TOP_DESC is val descending with id still ascending. The order is
 *   total (ids are unique per field) and depends on nothing but the rows: not on index positions, rebuilds, views or the shard layout. Pages therefore never
 *   overlap and the shards' answers merge exactly.
 * Cursor: `after` is a HOST pointer in both mem modes, read at call time (16 bytes). NULL: from the beginning. Otherwise a node is ELIGIBLE only if it is
 *   selected and comes strictly after *after in the order; the cursor need not name an existing row. Paging: pass the last record of the previous page. There
 *   is no offset: it would cost O(offset).
 * Answer: out[0 .. min(k, n_eligible)) = the first eligible nodes in order, *n_out = records written, *n_eligible = eligible nodes (with after == NULL the
 *   match count: the caller sees whether another page exists). n_out and n_eligible may be NULL. k is 1..BMX_TOP_MAX_K.
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes out, n_out and n_eligible as device pointers and only enqueues; no host round trip happens between
 *   the passes. An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched
 *   to its int64 column.
 * BMX_ERR_INVALID, before any device work and without writing anything: nterms outside 1..8, terms or out NULL, k == 0 or k > BMX_TOP_MAX_K, unknown flag bits,
 *   a bad mem, a NULL context / communicator.
 * Cost: an exact radix select over the composite key (value, then id) in sweeps of term 0's value column, each about one bmx_scan_count of that column:
 *   pass 0 (count, minimum and maximum of the keys; with more than one term also the probes, whose outcome later passes read from a bit mask), one sweep per
 *   11-bit digit of (max - min) until at most 4096 rows are at or below the boundary, one compaction sweep, one one-workgroup sort. A selection of at most 4096
 *   rows needs no digit sweep; 10^8 uniform values need one or two. WORST CASE: all keys equal — the value digits are skipped, but the boundary lies inside one
 *   tie group that only the ids tell apart: up to six id-digit sweeps (64 bits); with a wide value range in front of such a group, up to five value-digit sweeps
 *   (54 bits) before them.
 * Value-ordered views: a query on an index with a value-ordered view (bmx_index_set_ordered) takes this same column path — the dense columns are kept current
 *   whether or not a view exists — and the view's bookkeeping is untouched. Answering from the view in O(log R + k) is a follow-up: the view is ordered by
 *   (value, POSITION), so id-ordered ties at the boundary need their own select.
 * bmx_comm_scan_top (host memory): the query is enqueued on every shard before the first answer is fetched; the shards' answers (each <= k records, ordered) are
 *   merged on the host into the first k and their n_eligible added up — exact, because a node lives on one shard and the order is total. */
#ifndef BMX_TOP_H
#define BMX_TOP_H
#include "bmx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_top_rec { uint64_t id; int64_t val; } bmx_top_rec;   /* 16 bytes */
#define BMX_TOP_DESC  1u
#define BMX_TOP_MAX_K 4096u

int bmx_scan_top(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint32_t flags, const bmx_top_rec* after, uint32_t k,
                 bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible, int mem);
int bmx_comm_scan_top(bmx_comm* comm, uint32_t nterms, const bmx_term* terms, uint32_t flags, const bmx_top_rec* after, uint32_t k,
                      bmx_top_rec* out, uint64_t* n_out, uint64_t* n_eligible);

#ifdef __cplusplus
}
#endif
#endif
