/* include/bmx_reach.h compiles as C99 and its record is the size and the offsets the header draws (tests/test_reach_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_reach.h"
_Static_assert(sizeof(bmx_reach_res) == 40, "bmx_reach_res is 40 bytes");
_Static_assert(offsetof(bmx_reach_res, n_match) == 0 && offsetof(bmx_reach_res, set_size) == 8 && offsetof(bmx_reach_res, n_seed) == 16 &&
               offsetof(bmx_reach_res, n_edges) == 24, "the four counts");
_Static_assert(offsetof(bmx_reach_res, rounds) == 32 && offsetof(bmx_reach_res, flags) == 36, "the rounds and the flags word");
_Static_assert(sizeof(bmx_lit) == 24, "bmx_where.h's literal");
_Static_assert(BMX_REACH_OVERFLOW == 1u && BMX_REACH_MORE == 2u && BMX_REACH_MAX_SET == 1048576u && BMX_REACH_MAX_DEPTH == 255u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const reach)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*,
                          const bmx_lit*, uint32_t, uint32_t, uint64_t, uint64_t*, uint8_t*, uint64_t, bmx_reach_res*, int) = bmx_where_reach;
static int (*const reach_from)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, const int64_t*, uint64_t, uint32_t,
                               uint64_t, uint64_t*, uint8_t*, uint64_t, bmx_reach_res*, int) = bmx_where_reach_from;
static int (*const comm_reach)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*,
                               const bmx_lit*, uint32_t, uint32_t, uint64_t, uint64_t*, uint8_t*, uint64_t, bmx_reach_res*) = bmx_comm_where_reach;
static int (*const comm_reach_from)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, const int64_t*, uint64_t,
                                    uint32_t, uint64_t, uint64_t*, uint8_t*, uint64_t, bmx_reach_res*) = bmx_comm_where_reach_from;
