/* include/bmx_quant.h compiles as C99 and its records are the sizes and the offsets the header draws (tests/test_quant_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_quant.h"
_Static_assert(sizeof(bmx_quant_q) == 8, "bmx_quant_q is 8 bytes");
_Static_assert(offsetof(bmx_quant_q, num) == 0 && offsetof(bmx_quant_q, den) == 4, "the numerator, then the denominator");
_Static_assert(sizeof(bmx_quant_rec) == 32, "bmx_quant_rec is 32 bytes");
_Static_assert(offsetof(bmx_quant_rec, value) == 0 && offsetof(bmx_quant_rec, rank) == 8 && offsetof(bmx_quant_rec, n_below) == 16 && offsetof(bmx_quant_rec, n_equal) == 24, "the value, its rank, the two counts");
_Static_assert(sizeof(bmx_quant_res) == 32, "bmx_quant_res is 32 bytes");
_Static_assert(offsetof(bmx_quant_res, n_match) == 0 && offsetof(bmx_quant_res, n) == 8 && offsetof(bmx_quant_res, min) == 16 && offsetof(bmx_quant_res, max) == 24, "the two counts, the extremes");
_Static_assert(sizeof(bmx_lit) == 24, "bmx_where.h's literal");
_Static_assert(BMX_QUANT_MAX == 8u && BMX_QUANT_MAX_DEN == 1048576u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const quantiles)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const bmx_quant_q*, bmx_quant_rec*, bmx_quant_res*, int) = bmx_where_quantiles;
static int (*const comm_quantiles)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const bmx_quant_q*, bmx_quant_rec*, bmx_quant_res*) = bmx_comm_where_quantiles;
