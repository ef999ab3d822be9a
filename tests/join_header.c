/* include/bmx_join.h compiles as C99 and its record is the size and the offsets the header draws (tests/test_join_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_join.h"
_Static_assert(sizeof(bmx_join_res) == 184, "bmx_join_res is 184 bytes");
_Static_assert(offsetof(bmx_join_res, n_groups) == 0 && offsetof(bmx_join_res, map_size) == 8 && offsetof(bmx_join_res, n_inner) == 16 &&
               offsetof(bmx_join_res, n_keyed) == 24, "the four counts");
_Static_assert(offsetof(bmx_join_res, flags) == 32 && offsetof(bmx_join_res, reserved) == 36, "the flags word and its padding");
_Static_assert(offsetof(bmx_join_res, absent) == 40 && offsetof(bmx_join_res, unmatched) == 88 && offsetof(bmx_join_res, total) == 136, "the three records");
_Static_assert(sizeof(bmx_lit) == 24 && sizeof(bmx_group_rec) == 56 && sizeof(bmx_agg) == 48, "the header brings bmx_where.h and bmx_group.h with it");
_Static_assert(BMX_JOIN_MAP_OVERFLOW == 1u && BMX_JOIN_GROUP_OVERFLOW == 2u && BMX_JOIN_MAX_MAP == 1048576u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const join_group)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, const bmx_lit*,
                               uint32_t, uint32_t, uint64_t, bmx_group_rec*, uint64_t, bmx_join_res*, int) = bmx_where_join_group;
static int (*const map_group)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const int64_t*, const int64_t*, uint64_t,
                              bmx_group_rec*, uint64_t, bmx_join_res*, int) = bmx_where_map_group;
static int (*const comm_join_group)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*,
                                    const bmx_lit*, uint32_t, uint32_t, uint64_t, bmx_group_rec*, uint64_t, bmx_join_res*) = bmx_comm_where_join_group;
static int (*const comm_map_group)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const int64_t*, const int64_t*, uint64_t,
                                   bmx_group_rec*, uint64_t, bmx_join_res*) = bmx_comm_where_map_group;
