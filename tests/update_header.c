/* include/bmx_update.h compiles as C99 next to bmx.h and its record is the size and the offsets the header draws (tests/test_update_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx.h"
#include "bmx_update.h"
_Static_assert(sizeof(bmx_upd_res) == 72, "bmx_upd_res is 72 bytes");
_Static_assert(offsetof(bmx_upd_res, n_match) == 0 && offsetof(bmx_upd_res, n_nosrc) == 8 && offsetof(bmx_upd_res, n_range) == 16 && offsetof(bmx_upd_res, n_sent) == 24,
               "what was selected and what was sent");
_Static_assert(offsetof(bmx_upd_res, n_applied) == 32 && offsetof(bmx_upd_res, n_rows) == 40, "what the merge did");
_Static_assert(offsetof(bmx_upd_res, next_pos) == 48 && offsetof(bmx_upd_res, layout) == 56 && offsetof(bmx_upd_res, next_shard) == 64 && offsetof(bmx_upd_res, reserved) == 68,
               "the cursor");
_Static_assert(sizeof(bmx_lit) == 24 && sizeof(bmx_delta_rec) == 32, "the header brings bmx_where.h with it; a record is 32 bytes");
_Static_assert(BMX_UPD_SET == 0u && BMX_UPD_DELETE == 1u && BMX_UPD_COPY == 2u && BMX_UPD_ADD == 3u && BMX_UPD_FORCE == 1u && BMX_UPD_MAX_CAP == 16777216ull, "the constants");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
static int (*const upd)(bmx_ctx*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, int64_t, int64_t, uint32_t, uint64_t, uint64_t,
                        uint64_t*, bmx_upd_res*, int) = bmx_where_update;
static int (*const comm_upd)(bmx_comm*, uint32_t, uint32_t, const uint32_t*, const bmx_lit*, uint32_t, uint32_t, uint32_t, int64_t, int64_t, uint32_t, uint32_t, uint64_t,
                             uint64_t, uint64_t*, bmx_upd_res*) = bmx_comm_where_update;
