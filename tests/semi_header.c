/* include/bmx_semi.h compiles as C99 and its record is the size and the offsets the header draws (tests/test_semi_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_semi.h"
_Static_assert(sizeof(bmx_semi_res) == 32, "bmx_semi_res is 32 bytes");
_Static_assert(offsetof(bmx_semi_res, n_match) == 0 && offsetof(bmx_semi_res, set_size) == 8 && offsetof(bmx_semi_res, n_inner) == 16, "the three counts");
_Static_assert(offsetof(bmx_semi_res, flags) == 24 && offsetof(bmx_semi_res, reserved) == 28, "the flags word and its padding");
_Static_assert(sizeof(bmx_lit) == 24, "bmx_where.h's literal");
_Static_assert(BMX_SEMI_ANTI == 1u && BMX_SEMI_OVERFLOW == 1u && BMX_SEMI_MAX_SET == 1048576u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const semijoin)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, const bmx_lit*,
                             uint32_t, uint64_t, uint64_t*, uint64_t, bmx_semi_res*, int) = bmx_where_semijoin;
static int (*const where_in)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const int64_t*, uint64_t, uint64_t*, uint64_t,
                             bmx_semi_res*, int) = bmx_where_in;
static int (*const comm_semijoin)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*,
                                  const bmx_lit*, uint32_t, uint64_t, uint64_t*, uint64_t, bmx_semi_res*) = bmx_comm_where_semijoin;
static int (*const comm_where_in)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, const int64_t*, uint64_t, uint64_t*, uint64_t,
                                  bmx_semi_res*) = bmx_comm_where_in;
