/* include/bmx_group.h compiles as C99 and its records are the sizes and the offsets the header draws (tests/test_group_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_group.h"
_Static_assert(sizeof(bmx_group_rec) == 56, "bmx_group_rec is 56 bytes");
_Static_assert(offsetof(bmx_group_rec, key) == 0 && offsetof(bmx_group_rec, agg) == 8, "the key, then the record of bmx_where_aggregate");
_Static_assert(sizeof(bmx_group_res) == 112, "bmx_group_res is 112 bytes");
_Static_assert(offsetof(bmx_group_res, n_groups) == 0 && offsetof(bmx_group_res, flags) == 8 && offsetof(bmx_group_res, reserved) == 12, "the count, the flags word and its padding");
_Static_assert(offsetof(bmx_group_res, absent) == 16 && offsetof(bmx_group_res, total) == 64, "the two records");
_Static_assert(sizeof(bmx_agg) == 48 && sizeof(bmx_lit) == 24, "bmx.h's record and bmx_where.h's literal");
_Static_assert(BMX_GROUP_OVERFLOW == 1u && BMX_GROUP_MAX_CAP == 1048576u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const group)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, bmx_group_rec*, uint64_t, bmx_group_res*, int) = bmx_where_group;
static int (*const comm_group)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, bmx_group_rec*, uint64_t, bmx_group_res*) = bmx_comm_where_group;
