/* include/bmx_first.h compiles as C99 and its records are the size and the offsets the header draws (tests/test_first_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_first.h"
_Static_assert(sizeof(bmx_first_rec) == 40, "bmx_first_rec is 40 bytes");
_Static_assert(offsetof(bmx_first_rec, key) == 0 && offsetof(bmx_first_rec, id) == 8 && offsetof(bmx_first_rec, val) == 16 && offsetof(bmx_first_rec, n_match) == 24 &&
               offsetof(bmx_first_rec, n) == 32, "the five words of a record");
_Static_assert(sizeof(bmx_first_res) == 40, "bmx_first_res is 40 bytes");
_Static_assert(offsetof(bmx_first_res, n_groups) == 0 && offsetof(bmx_first_res, flags) == 8 && offsetof(bmx_first_res, reserved) == 12 &&
               offsetof(bmx_first_res, total) == 16 && offsetof(bmx_first_res, absent) == 24 && offsetof(bmx_first_res, n_ordered) == 32, "the result record");
_Static_assert(sizeof(bmx_lit) == 24 && sizeof(bmx_rows_res) == 40, "the header brings bmx_where.h and bmx_rows.h with it");
_Static_assert(BMX_FIRST_DESC == 2u && BMX_ROWS_TS == 1u && BMX_FIRST_OVERFLOW == 1u && BMX_FIRST_NO_NODE == 18446744073709551615ull &&
               BMX_FIRST_MAX_CAP == 1048576u && BMX_ROWS_MAX_FIELDS == 8u && BMX_ROWS_NO_CLOCK == -1, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const group_first)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t, uint64_t,
                                bmx_first_rec*, int64_t*, int64_t*, bmx_first_res*, int) = bmx_where_group_first;
static int (*const comm_group_first)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t,
                                     uint64_t, bmx_first_rec*, int64_t*, int64_t*, bmx_first_res*) = bmx_comm_where_group_first;
