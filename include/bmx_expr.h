/* bmx_expr.h — computed measures: bmx_where_aggregate_expr, bmx_where_group_expr, bmx_where_quantiles_expr and their sharded forms. Additions to the C ABI
 * of bmx.h (ABI 4, unchanged); include it next to bmx.h. It brings bmx_where.h (the program: bmx_lit), bmx_group.h and bmx_quant.h (the records) with it.
 *
 * What it replaces: every aggregate form measured ONE field. "Total inventory value" (sum of price * inventory), "sum of net + tax by status", "p95 of
 * end - start among the requests that are not cached", the variance of a field (which needs the sum of a * a) were answered only when somebody had stored the
 * expression as a field of its own, or by bmx_where_rows of both fields to the host and arithmetic there. These calls compute the measure in the sweep that
 * already probes it: m = value(a) op value(b) of the selected node, op one of + - *. Nothing proportional to the match count leaves the device.
 *
 * Everything except the measure is the plain form's — bmx_where_aggregate (bmx_where_agg.h), bmx_where_group (bmx_group.h), bmx_where_quantiles (bmx_quant.h):
 *   the selection (bmx_scan_where's program and candidates), the records (bmx_agg; bmx_group_rec / bmx_group_res; bmx_quant_rec / bmx_quant_res), the group
 *   window group_lo .. group_lo + ngroups - 1 with its record of everything else, `absent` and `total`, the overflow rule of the discovered groups and the
 *   sorted host output, the rank rule, the mem modes, the ordering behind a deferred compaction, growth, the switch to the int64 column, and a value-ordered view
 *   of base_field, which is neither read nor touched.
 *
 * The measure of a selected node. m->a and m->b name two fields of the node. Every selected node falls into exactly one of three classes:
 *   defined      : the rows of a and of b both hold data, and the EXACT integer result of value(a) op value(b) lies in -(2^53 - 1) .. 2^53 - 1. The node counts
 *                  in n, sum, min and max (in the sample of the quantiles) with that value.
 *   undefined    : the row of a or of b is absent or tombstoned. The node counts in n_match only, as a node without its measure field does in the plain form,
 *                  and in xres->n_undef.
 *   out of range : both rows hold data and the exact result lies outside -(2^53 - 1) .. 2^53 - 1. The node counts in n_match only, and in xres->n_range. Its
 *                  value is never folded in, never wrapped and never clamped. (2^53 - 1 is the engine's value domain and the range in which JavaScript's
 *                  numbers are exact integers; the 128-bit sums, the digits of the select and the shards' merges are built for it. The update by query counts
 *                  its out-of-range results the same way.)
 *   The result is decided exactly: a product is judged beyond its low 64 bits, so 2^32 * (2^32 + 1), whose low 64 bits are 2^32, is out of range.
 *   xres counts over all groups together: total.n_match == total.n + n_undef + n_range for the grouped forms (for bmx_where_aggregate_expr: summed over all
 *   records of the answer), res->n_match == res->n + n_undef + n_range for the quantiles.
 * Operands: either may be base_field (the column value, no probe), a field of the program (probed once more after the match is known, as a plain measure is)
 *   or a field the program does not name. a == b is allowed and is probed once: a * a for a variance, a + a for doubling, a - a = 0 for every node that holds
 *   a. The operands take no slot of the program. BMX_EXPR_SUB is value(a) - value(b), in this order.
 * xres: a HOST pointer with BMX_MEM_HOST, a DEVICE pointer with BMX_MEM_DEVICE, where it is written fully and in stream order, whatever it held. It may be NULL.
 * BMX_ERR_INVALID, before any device work and without writing anything, each with a text of its own: m NULL; m->op outside 1..3; m->reserved != 0; m->a or
 *   m->b equal to BMX_AGG_NO_FIELD; and every refusal of the plain form (the program's, the group arguments', the quantiles', a bad mem, a NULL context /
 *   communicator).
 * Cost: the plain form's sweep, with one probe per operand that is not base_field (one for a == b) per SELECTED candidate. The quantiles form always takes the
 *   plain form's probed route: its first sweep leaves the computed value in the scratch of 8 bytes per index position, which the digit sweeps read.
 * Sharded forms (host memory): a node's rows all live on the shard that owns its id, so a node is classified by one shard alone. The records combine as the
 *   plain forms' do, n_undef and n_range add, and the quantiles form steps the shards in lockstep as bmx_comm_where_quantiles does. One shard gives the bytes
 *   the single-context call gives. */
#ifndef BMX_EXPR_H
#define BMX_EXPR_H
#include "bmx.h"
#include "bmx_where.h"
#include "bmx_group.h"
#include "bmx_quant.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_expr { uint32_t a, b; uint32_t op; uint32_t reserved; } bmx_expr;   /* 16 bytes; reserved must be 0 */
#define BMX_EXPR_ADD 1u   /* value(a) + value(b) */
#define BMX_EXPR_SUB 2u   /* value(a) - value(b) */
#define BMX_EXPR_MUL 3u   /* value(a) * value(b) */
typedef struct bmx_expr_res { uint64_t n_undef, n_range; } bmx_expr_res;                /* 16 bytes */

int bmx_where_aggregate_expr(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                             uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out, bmx_expr_res* xres, int mem);
int bmx_where_group_expr(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                         uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res, bmx_expr_res* xres, int mem);
int bmx_where_quantiles_expr(bmx_ctx* ctx, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                             uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, bmx_expr_res* xres, int mem);
int bmx_comm_where_aggregate_expr(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                                  uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* out, bmx_expr_res* xres);
int bmx_comm_where_group_expr(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                              uint32_t group_field, bmx_group_rec* out, uint64_t cap, bmx_group_res* res, bmx_expr_res* xres);
int bmx_comm_where_quantiles_expr(bmx_comm* comm, uint32_t base_field, uint32_t nclauses, const uint32_t* clause_len, const bmx_lit* lits, const bmx_expr* m,
                                  uint32_t nq, const bmx_quant_q* qs, bmx_quant_rec* out, bmx_quant_res* res, bmx_expr_res* xres);

#ifdef __cplusplus
}
#endif
#endif
