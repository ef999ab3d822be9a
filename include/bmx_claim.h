/* bmx_claim.h — the probe kernel's claim mode: bmx_selfcheck_claim and bmx_get_claim_mode. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it
 * next to bmx.h.
 *
 * How a delta that was not below the value it saw claims its row in the merge's probe kernel:
 *   BMX_CLAIM_STORE  one atomic exchange on the row's head, then — the first claimer only — one 16-byte store of (ts,val);
 *   BMX_CLAIM_TEAM   three lanes of ONE 64-bit swap instruction write the head word, ts and val, which share a 64-byte granule and leave the L2 as one memory-side
 *                    request; nothing is stored and no line is dirtied. Every claimer that beat the value it saw writes, so during a batch a row with several
 *                    claimers holds the value of whichever swapped last; the resolve pass rewrites every such row.
 * `team` rests on a second property the ISA does not promise: an aligned 16-byte load of (ts,val) never observes one word of such a swap without the other.
 * bmx_selfcheck_claim hammers that like bmx_selfcheck (same outputs; the control issues the three swaps as three instructions and MUST tear); it reports and
 * does not fail on a torn pair. bmx_create runs it once per device and process beside bmx_selfcheck: new contexts take `team` if no pair tore and the control
 * did, `store` otherwise (also where BMX_SKIP_SELFCHECK=1 skipped the check). BMX_CLAIM_MODE=store|team in the environment overrides that at create.
 * Batches with BMX_MERGE_UNIQUE_KEYS, bmx_put_rows and the strict-flag kernels claim as before in either mode. The reference has no counterpart. */
#ifndef BMX_CLAIM_H
#define BMX_CLAIM_H
#include "bmx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_CLAIM_STORE 0
#define BMX_CLAIM_TEAM  1
int bmx_selfcheck_claim(int device, uint64_t* reads, uint64_t* torn, uint64_t* control_torn);
int bmx_get_claim_mode(bmx_ctx* ctx);               /* BMX_CLAIM_STORE or BMX_CLAIM_TEAM; < 0: error */

#ifdef __cplusplus
}
#endif
#endif
