/* include/bmx_join_rows.h compiles as C99 and its record is the size and the offsets the header draws (tests/test_join_rows_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_join_rows.h"
_Static_assert(sizeof(bmx_jrows_res) == 72, "bmx_jrows_res is 72 bytes");
_Static_assert(offsetof(bmx_jrows_res, n_match) == 0 && offsetof(bmx_jrows_res, n_out) == 8 && offsetof(bmx_jrows_res, next_pos) == 16 &&
               offsetof(bmx_jrows_res, layout) == 24, "the four words of bmx_rows_res");
_Static_assert(offsetof(bmx_jrows_res, n_joined) == 32 && offsetof(bmx_jrows_res, map_size) == 40 && offsetof(bmx_jrows_res, n_inner) == 48 &&
               offsetof(bmx_jrows_res, n_keyed) == 56, "the join's counts");
_Static_assert(offsetof(bmx_jrows_res, flags) == 64 && offsetof(bmx_jrows_res, next_shard) == 68, "the flags word and the cursor's shard");
_Static_assert(sizeof(bmx_lit) == 24 && sizeof(bmx_rows_res) == 40 && sizeof(bmx_join_res) == 184, "the header brings bmx_rows.h and bmx_join.h with it");
_Static_assert(BMX_JROWS_INNER == 2u && BMX_ROWS_TS == 1u && BMX_JROWS_NO_NODE == 18446744073709551615ull && BMX_JOIN_MAP_OVERFLOW == 1u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const join_rows)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t, const uint32_t*,
                              const bmx_lit*, uint32_t, uint32_t, const uint32_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint64_t*, int64_t*, int64_t*, uint64_t*,
                              int64_t*, int64_t*, bmx_jrows_res*, int) = bmx_where_join_rows;
static int (*const map_rows)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const uint32_t*, const int64_t*, const uint64_t*,
                             uint64_t, uint32_t, const uint32_t*, uint32_t, uint64_t, uint64_t, uint64_t*, int64_t*, int64_t*, uint64_t*, int64_t*, int64_t*,
                             bmx_jrows_res*, int) = bmx_where_map_rows;
static int (*const comm_join_rows)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t,
                                   const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const uint32_t*, uint64_t, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t*,
                                   int64_t*, int64_t*, uint64_t*, int64_t*, int64_t*, bmx_jrows_res*) = bmx_comm_where_join_rows;
static int (*const comm_map_rows)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const uint32_t*, const int64_t*,
                                  const uint64_t*, uint64_t, uint32_t, const uint32_t*, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t*, int64_t*, int64_t*,
                                  uint64_t*, int64_t*, int64_t*, bmx_jrows_res*) = bmx_comm_where_map_rows;
