/* include/bmx_group_top.h compiles as C99 and its records are the size and the offsets the header draws (tests/test_gtop_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_group_top.h"
_Static_assert(sizeof(bmx_gtop_grp) == 32, "bmx_gtop_grp is 32 bytes");
_Static_assert(offsetof(bmx_gtop_grp, key) == 0 && offsetof(bmx_gtop_grp, n_match) == 8 && offsetof(bmx_gtop_grp, n) == 16 && offsetof(bmx_gtop_grp, n_rows) == 24,
               "the four words of a group");
_Static_assert(sizeof(bmx_gtop_row) == 16 && offsetof(bmx_gtop_row, id) == 0 && offsetof(bmx_gtop_row, val) == 8, "the two words of a row");
_Static_assert(sizeof(bmx_gtop_res) == 48, "bmx_gtop_res is 48 bytes");
_Static_assert(offsetof(bmx_gtop_res, n_groups) == 0 && offsetof(bmx_gtop_res, flags) == 8 && offsetof(bmx_gtop_res, per) == 12 && offsetof(bmx_gtop_res, total) == 16 &&
               offsetof(bmx_gtop_res, absent) == 24 && offsetof(bmx_gtop_res, n_ordered) == 32 && offsetof(bmx_gtop_res, n_rows) == 40, "the result record");
_Static_assert(sizeof(bmx_lit) == 24 && sizeof(bmx_rows_res) == 40, "the header brings bmx_where.h and bmx_rows.h with it");
_Static_assert(BMX_GTOP_DESC == 2u && BMX_ROWS_TS == 1u && BMX_GTOP_OVERFLOW == 1u && BMX_GTOP_NO_NODE == 18446744073709551615ull && BMX_GTOP_MAX_CAP == 1048576u &&
               BMX_GTOP_MAX_PER == 16u && BMX_GTOP_MAX_ROWS == 4194304u && BMX_ROWS_MAX_FIELDS == 8u && BMX_ROWS_NO_CLOCK == -1, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const group_top)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t, uint64_t,
                              bmx_gtop_grp*, bmx_gtop_row*, int64_t*, int64_t*, bmx_gtop_res*, int) = bmx_where_group_top;
static int (*const comm_group_top)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t,
                                   uint64_t, bmx_gtop_grp*, bmx_gtop_row*, int64_t*, int64_t*, bmx_gtop_res*) = bmx_comm_where_group_top;
