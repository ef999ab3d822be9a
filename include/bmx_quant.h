/* bmx_quant.h — exact quantiles over boolean filters: bmx_where_quantiles and its sharded form. Additions to the C ABI of bmx.h (ABI 4, unchanged); include
 * it next to bmx.h. It brings bmx_where.h (the program: bmx_lit) with it.
 *
 * What it replaces: order statistics over a filter — "the median order value of active users", "p95 / p99 latency of the requests that are not cached", "the
 * quartiles of age among non-admins" — needed bmx_scan_where with ids, a bmx_get_rows of the measure to the host and a partition there. bmx_where_top cannot
 * stand in: its k is at most BMX_TOP_MAX_K and it orders by the base field only. This call selects on the device: an exact radix select for up to
 * BMX_QUANT_MAX ranks at once, over the base field's column or over a probed field. The answer is a value, so ties need no id digits, no compaction, no sort.
 *
 * Selection: exactly bmx_scan_where's. The program is its `nclauses, clause_len, lits` (disjunctive normal form over range literals; see bmx_where.h for
 *   literal truth, BMX_LIT_NOT, clamping and the limits). The candidates are the positions of base_field's dense index (built or refreshed like any scan) whose
 *   row holds data. res->n_match = selected nodes.
 * Sample: the multiset of measure_field's values of the selected nodes whose measure row holds data; res->n is its size. A selected node whose measure row is
 *   absent or tombstoned counts in n_match but not in n, as in bmx_where_aggregate. measure_field may be base_field (the value comes from the column, no
 *   probe), a field of the program, or a field the program does not name; in the last two cases the field is probed once per selected candidate, in the first
 *   sweep only: that sweep leaves the value in a scratch of 8 bytes per index position, which the context owns and the later sweeps read.
 * Rank rule ("lower" nearest rank, numpy.sort(v)[(num * (n - 1)) // den]): qs[i] is the quantile num / den, 0 <= num <= den, 1 <= den <= BMX_QUANT_MAX_DEN,
 *   and rank = floor(num * (n - 1) / den). The product fits 64 bits: an index has fewer than 2^44 rows and den <= 2^20.
 *     out[i].value   = the sample's element of that 0-based rank in ascending order
 *     out[i].rank    = the rank
 *     out[i].n_below = sample elements strictly smaller than value
 *     out[i].n_equal = sample elements equal to value; n_below <= rank < n_below + n_equal
 *   0/1 is the minimum, 1/1 the maximum, 1/2 the lower median. qs may repeat a quantile and need not be sorted; the records come back in the order of qs.
 *   qs is a HOST pointer in both mem modes and is read at call time, like `after` in bmx_where_top.
 * Empty sample: n == 0 gives every record {0, 0, 0, 0}, res->min = INT64_MAX and res->max = INT64_MIN. Otherwise res->min / res->max are the sample's.
 * Output: out[0 .. nq) and *res are written fully, whatever they held. res may be NULL.
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes out and res as device pointers and only enqueues; nothing comes back to the host between the sweeps.
 *   An ordinary entry point: it orders behind a deferred compaction, sees the last merge, works after a growth and on an index that has switched to its int64
 *   column.
 * Value-ordered views: with a view on base_field (bmx_index_set_ordered) the call still takes the column path and leaves the view's bookkeeping untouched, as
 *   bmx_where_top does.
 * Cost: one sweep of the base column with the program's probes (bmx_where_aggregate's sweep), then one sweep of one bit per position plus the value (the column,
 *   or the 8-byte scratch) per 11 bits of (largest - smallest value of the sample): none when all values are equal, at most 3 for a measure that is the base
 *   field on its 4-byte column, at most 5 otherwise. More quantiles widen the histograms, not the sweeps.
 * BMX_ERR_INVALID, before any device work and without writing anything: every refusal of bmx_scan_where's program; nq == 0 or nq > BMX_QUANT_MAX; qs or out
 *   NULL; a den of 0 or above BMX_QUANT_MAX_DEN, or num > den; a bad mem; a NULL context / communicator. BMX_ERR_NOMEM, with nothing written, when the value
 *   scratch of a probed measure cannot be allocated.
 * bmx_comm_where_quantiles (host memory): the quantiles of the shards do not combine, so the communicator steps the same sweeps itself. The program is checked
 *   and prepared once; the first sweep is enqueued on every shard before anything is fetched; the shards' counts, minima and maxima fold on the host; then per
 *   digit the live prefixes go up to every shard, every shard's sweep is enqueued, the histograms (at most nq x 16 KB per shard) come down and add, and the
 *   host finds the bins with the very code the device uses. Exact, because a node's rows all live on the shard that owns its id; one shard gives the bytes
 *   bmx_where_quantiles gives. */
#ifndef BMX_QUANT_H
#define BMX_QUANT_H
#include "bmx.h"
#include "bmx_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_QUANT_MAX     8u          /* quantiles per call */
#define BMX_QUANT_MAX_DEN (1u << 20)

typedef struct bmx_quant_q   { uint32_t num, den; } bmx_quant_q;                                  /* the quantile num / den */
typedef struct bmx_quant_rec { int64_t value; uint64_t rank, n_below, n_equal; } bmx_quant_rec;   /* 32 bytes */
typedef struct bmx_quant_res { uint64_t n_match, n; int64_t min, max; } bmx_quant_res;            /* 32 bytes */

int bmx_where_quantiles(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                        uint32_t measure_field, uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, int mem);
int bmx_comm_where_quantiles(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits,
                             uint32_t measure_field, uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res);

#ifdef __cplusplus
}
#endif
#endif
