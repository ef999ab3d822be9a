/* include/bmx_expr.h compiles as C99 and its records are the sizes and the offsets the header draws (tests/test_expr_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_expr.h"
_Static_assert(sizeof(bmx_expr) == 16, "bmx_expr is 16 bytes");
_Static_assert(offsetof(bmx_expr, a) == 0 && offsetof(bmx_expr, b) == 4 && offsetof(bmx_expr, op) == 8 && offsetof(bmx_expr, reserved) == 12, "the operands, the op, the reserved word");
_Static_assert(sizeof(bmx_expr_res) == 16, "bmx_expr_res is 16 bytes");
_Static_assert(offsetof(bmx_expr_res, n_undef) == 0 && offsetof(bmx_expr_res, n_range) == 8, "the two counts");
_Static_assert(BMX_EXPR_ADD == 1u && BMX_EXPR_SUB == 2u && BMX_EXPR_MUL == 3u, "the ops");
_Static_assert(sizeof(bmx_lit) == 24 && sizeof(bmx_group_rec) == 56 && sizeof(bmx_group_res) == 112 && sizeof(bmx_quant_rec) == 32, "the headers it brings with it");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const agg)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, const bmx_expr*, uint32_t, int64_t, uint32_t, bmx_agg*, bmx_expr_res*, int) = bmx_where_aggregate_expr;
static int (*const grp)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, const bmx_expr*, uint32_t, bmx_group_rec*, uint64_t, bmx_group_res*, bmx_expr_res*, int) = bmx_where_group_expr;
static int (*const qnt)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, const bmx_expr*, uint32_t, const bmx_quant_q*, bmx_quant_rec*, bmx_quant_res*, bmx_expr_res*, int) = bmx_where_quantiles_expr;
static int (*const cagg)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, const bmx_expr*, uint32_t, int64_t, uint32_t, bmx_agg*, bmx_expr_res*) = bmx_comm_where_aggregate_expr;
static int (*const cgrp)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, const bmx_expr*, uint32_t, bmx_group_rec*, uint64_t, bmx_group_res*, bmx_expr_res*) = bmx_comm_where_group_expr;
static int (*const cqnt)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, const bmx_expr*, uint32_t, const bmx_quant_q*, bmx_quant_rec*, bmx_quant_res*, bmx_expr_res*) = bmx_comm_where_quantiles_expr;
