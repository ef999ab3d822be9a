/* include/bmx_rows.h compiles as C99 and its record is the size and the offsets the header draws (tests/test_rows_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_rows.h"
_Static_assert(sizeof(bmx_rows_res) == 40, "bmx_rows_res is 40 bytes");
_Static_assert(offsetof(bmx_rows_res, n_match) == 0 && offsetof(bmx_rows_res, n_out) == 8 && offsetof(bmx_rows_res, next_pos) == 16 && offsetof(bmx_rows_res, layout) == 24, "the four counts");
_Static_assert(offsetof(bmx_rows_res, next_shard) == 32 && offsetof(bmx_rows_res, reserved) == 36, "the shard of the cursor and its padding");
_Static_assert(sizeof(bmx_lit) == 24, "bmx_where.h's literal");
_Static_assert(BMX_ROWS_MAX_FIELDS == 8u && BMX_ROWS_TS == 1u && BMX_ROWS_NO_CLOCK == -1, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const rows)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, const uint32_t*, uint32_t, uint64_t, uint64_t, uint64_t*, int64_t*, int64_t*,
                         bmx_rows_res*, int) = bmx_where_rows;
static int (*const comm_rows)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, const uint32_t*, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t*, int64_t*,
                              int64_t*, bmx_rows_res*) = bmx_comm_where_rows;
