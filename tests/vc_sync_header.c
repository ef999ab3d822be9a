/* include/bmx_vc_sync.h compiles as C99 and its records are the sizes and offsets the header draws (tests/test_vc_sync_cabi.py runs cc -fsyntax-only). */
#include <stddef.h>
#include "bmx_vc_sync.h"
_Static_assert(sizeof(bmx_vc_rec) == 64, "bmx_vc_rec is 64 bytes");
_Static_assert(offsetof(bmx_vc_rec, id) == 0 && offsetof(bmx_vc_rec, field) == 8 && offsetof(bmx_vc_rec, aux) == 12, "first quarter");
_Static_assert(offsetof(bmx_vc_rec, val) == 16 && offsetof(bmx_vc_rec, state) == 24 && offsetof(bmx_vc_rec, keyset) == 28, "second quarter");
_Static_assert(offsetof(bmx_vc_rec, clock) == 32 && sizeof(((bmx_vc_rec*)0)->clock) == 32, "the clock is the second half");
_Static_assert(sizeof(bmx_vc_table_info) == 48 && offsetof(bmx_vc_table_info, k_writers) == 32, "bmx_vc_table_info is 48 bytes");
_Static_assert(BMX_ABI_VERSION == 4, "an addition to ABI 4");
