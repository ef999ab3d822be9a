/* include/bmx_group_multi.h compiles as C99 and its records are the sizes and the offsets the header draws (tests/test_mgroup_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_group_multi.h"
_Static_assert(sizeof(bmx_group_key) == 24, "bmx_group_key is 24 bytes");
_Static_assert(offsetof(bmx_group_key, field) == 0 && offsetof(bmx_group_key, flags) == 4 && offsetof(bmx_group_key, origin) == 8 && offsetof(bmx_group_key, width) == 16,
               "the field, its flags word, the origin and the width");
_Static_assert(sizeof(bmx_mgroup_rec) == 80, "bmx_mgroup_rec is 80 bytes");
_Static_assert(offsetof(bmx_mgroup_rec, key) == 0 && offsetof(bmx_mgroup_rec, agg) == 32, "four keys, then the record of bmx_where_aggregate");
_Static_assert(sizeof(bmx_group_res) == 112 && sizeof(bmx_agg) == 48 && sizeof(bmx_lit) == 24, "bmx_group.h's result record, bmx.h's record and bmx_where.h's literal");
_Static_assert(BMX_MGROUP_MAX_KEYS == 4u && BMX_MGROUP_MAX_CAP4 == 16384u && BMX_GROUP_MAX_CAP == 1048576u && BMX_GROUP_OVERFLOW == 1u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const mgroup)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const bmx_group_key*, bmx_mgroup_rec*, uint64_t, bmx_group_res*,
                           int) = bmx_where_group_multi;
static int (*const comm_mgroup)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const bmx_group_key*, bmx_mgroup_rec*, uint64_t,
                                bmx_group_res*) = bmx_comm_where_group_multi;
