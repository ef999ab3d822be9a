/* include/bmx_watch.h compiles as C99 and its record is the size and the offsets the header draws (tests/test_watch_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_watch.h"
_Static_assert(sizeof(bmx_watch_res) == 32, "bmx_watch_res is 32 bytes");
_Static_assert(offsetof(bmx_watch_res, n_entered) == 0 && offsetof(bmx_watch_res, n_left) == 8 && offsetof(bmx_watch_res, n_match) == 16, "the three counts");
_Static_assert(offsetof(bmx_watch_res, flags) == 24 && offsetof(bmx_watch_res, reserved) == 28, "the flags word and its padding");
_Static_assert(sizeof(bmx_lit) == 24, "a watch takes bmx_where.h's literal");
_Static_assert(BMX_WATCH_MAX == 16u && BMX_WATCH_RESET == 1u && BMX_WATCH_OVERFLOW == 2u, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const poll)(bmx_ctx*, uint32_t, uint64_t*, uint64_t, uint64_t*, uint64_t, bmx_watch_res*, int) = bmx_watch_poll;
static int (*const comm_poll)(bmx_comm*, uint32_t, uint64_t*, uint64_t, uint64_t*, uint64_t, bmx_watch_res*) = bmx_comm_watch_poll;
