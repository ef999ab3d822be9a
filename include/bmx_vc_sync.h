/* bmx_vc_sync.h — replica reconciliation of the K-writer vector-clock table (bmx.h "N4"): a table's description, per-bucket state digests, its version
 * vector, a filtered export as 64-byte records and the record merge that receives them. Additions to the C ABI of bmx.h (ABI 4, unchanged); include it next
 * to bmx.h.
 *
 * What it replaces in the reference: the anti-entropy loop — the producer _collectFullSyncData (src/bullet-network-sync.js:592-664) and the consumer
 * _processSyncEntries (:551-569) — runs between peers with different ids, so the clocks it moves are multi-writer clocks by construction. The scalar table has
 * bmx_digest / bmx_export_rows / bmx_merge_records (bmx.h "replica reconciliation"); this is the same loop for the rows of a bmx_vc: compare digests, export
 * the rows of the buckets that differ, merge them at the peer through its own resolve(). No host-side mirror of the keys is needed for a checkpoint
 * (export everything), a comparison (digests) or a hand-over (export + merge).
 *
 * A ROW is a slot whose id is not the reserved id and whose state is not BMX_VC_ABSENT (the rule of bmx_vc_scan_range). This table has no tombstones; the
 * counts of a digest at any L add up to bmx_vc_row_count.
 *
 * bmx_vc_rec: one row as a delta, 64 bytes — the slot image with the claim word replaced by aux. Exported records carry aux = 0, the row's stored key set and
 *   its state (BMX_VC_DENSE / BMX_VC_SPARSE); components of writers >= K are 0. They never carry the claim word.
 *
 * Row digest (bmx_vc_rec_digest computes exactly this on the host; pure, no GPU). sm = the splitmix64 step of bmx.h "replica reconciliation":
 *     w0 = val, w1 = keyset | (uint64)state << 32, w2..w5 = clock[2i] | (uint64)clock[2i+1] << 32 for i = 0..3 (all eight components whatever K is)
 *     h = sm(w0); h = sm(h ^ w1); ... h = sm(h ^ w5); h = sm(h ^ field); digest = sm(h ^ id)
 *   The key set is part of the digest on purpose: the reference calls two clocks identical only when their JSON texts are (src/bullet-crt.js:200-203), and the
 *   key set is that text's key order. Two tables are comparable when they number their writers alike; K may differ, since components beyond K are zero.
 *
 * bmx_vc_info: the table's shape. n_rows is exact (the stream is waited for); table_bytes = n_slots x 64.
 *
 * bmx_vc_digest: sums[b] = sum mod 2^64 of the row digests of bucket b, counts[b] = number of rows in it, b = bmx_key_bucket(id, field, L), L = log2_buckets
 *   in 0..16 — the scalar table's bucket function, so buckets nest and both tables of a replica agree on it. Both vectors (2^L words each) are written in
 *   full, in stream order; nothing behind 2^L words is touched. flags must be 0. One read-only sweep of n_slots x 64 bytes. L <= 10: accumulated in LDS,
 *   non-zero buckets flushed once per workgroup. L = 11..16 is the SLOW form: one pair of global atomics per row (the split of bmx_digest, for its reasons).
 *   Stands in for the comparison the reference does not have: it ships every entry since a time (src/bullet-network-sync.js:602, :633).
 *
 * bmx_vc_frontier: out8[k] = maximum of clock[k] over all rows; entries for k >= K are 0; an empty table gives all zeros. The table's version vector — what
 *   a peer needs to know to send only what this table has not seen (the `since` of src/bullet-network-sync.js:84, :592, as a vector).
 *
 * bmx_vc_export_rows: one record for every row that passes both filters (the producer, src/bullet-network-sync.js:592-664):
 *     - its bucket's bit is set in bucket_bits (bit b = word b / 64, bit b % 64; 2^L bits, at least one word; NULL = every bucket; lives in `mem` like out and
 *       n_out — the format of bmx_export_rows);
 *     - with a non-NULL frontier8, some clock[k] > frontier8[k] for k < K: the row is not dominated by what the asker has already seen. frontier8 is a HOST
 *       pointer in both mem modes; eight words are read at call time (like the cursor of bmx_scan_top). A row whose clock is all zeros is NEVER selected
 *       under a frontier (it exceeds no frontier, not even the all-zero one): export such rows with frontier8 = NULL.
 *   flags must be 0. Output in ascending slot order (deterministic for a given table); *n_out = number of matches even when cap is smaller; nothing is written
 *   at or beyond out[min(n, cap)]; out == NULL counts only. Host mode stages the records; an `out` in bmx_host_alloc memory is written by the kernel itself.
 *   The table is read twice (count, write).
 *
 * bmx_vc_merge_records: the consumer (src/bullet-network-sync.js:551-569 feeding resolve(), src/bullet-crt.js:164-279). The records are deltas: id, field,
 *   clock[0..K), keyset and val; aux and state are ignored. The outcome is exactly that of bmx_vc_merge_batch_ks over the same columns in the same order —
 *   same flags, same updated_idx, same domain checks (BMX_ERR_RANGE), same growth rule: one unpack kernel into the table's workspace columns, then the
 *   merge's own launches. n <= 2^24; n = 0 writes n_updated = 0. Every record bmx_vc_export_rows produces is accepted; a record with a non-zero component at
 *   k >= K is BMX_ERR_RANGE (host mode: returned; device mode: sticky, reported by bmx_vc_sync). The receiver's join is resolve(), including the quirk that a
 *   first write stores {local: 2} (src/bullet-crt.js:172-185): one exchange does not always equalise two tables; the driver repeats it.
 *
 * mem: BMX_MEM_HOST is synchronous. BMX_MEM_DEVICE takes sums / counts / out8 / bucket_bits / out / n_out / recs / updated_idx / n_updated / flags as device
 *   pointers and only enqueues on the table's stream (bmx_vc_set_stream); outputs, counts and n_updated included, are valid after bmx_vc_sync. Both modes
 *   order behind earlier device-pointer merges by stream order, and both work after a growth.
 * BMX_ERR_INVALID, before any device work and without writing anything: a NULL table, L > 16, unknown flag bits, a bad mem, NULL sums, counts or out8, NULL
 *   n_out together with NULL out, n > 2^24, NULL recs with n > 0. The text goes to the vector-clock error word (bmx_vc_last_error) only. */
#ifndef BMX_VC_SYNC_H
#define BMX_VC_SYNC_H
#include "bmx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmx_vc_rec {        /* 64 bytes: one row of a K-writer table as a delta — the slot image with the claim word replaced by aux */
  uint64_t id; uint32_t field; uint32_t aux;      /* aux: 0 on export, ignored on merge */
  int64_t  val; uint32_t state; uint32_t keyset;  /* state: BMX_VC_DENSE / BMX_VC_SPARSE on export, ignored on merge */
  uint32_t clock[8];                              /* components of writers >= K are 0 */
} bmx_vc_rec;
typedef struct bmx_vc_table_info { uint64_t n_slots, n_rows, capacity_rows, table_bytes; uint32_t k_writers, local_writer, device, reserved; } bmx_vc_table_info;

uint64_t bmx_vc_rec_digest(const bmx_vc_rec* r);                         /* pure, no GPU */
int bmx_vc_info(bmx_vc* t, bmx_vc_table_info* out);
int bmx_vc_digest(bmx_vc* t, uint32_t log2_buckets, uint32_t flags, uint64_t* sums, uint64_t* counts, int mem);
int bmx_vc_frontier(bmx_vc* t, uint32_t* out8, int mem);
int bmx_vc_export_rows(bmx_vc* t, const uint32_t* frontier8, uint32_t log2_buckets, const uint64_t* bucket_bits, uint32_t flags,
                       bmx_vc_rec* out, uint64_t cap, uint64_t* n_out, int mem);
int bmx_vc_merge_records(bmx_vc* t, uint64_t n, const bmx_vc_rec* recs, uint32_t* updated_idx, uint64_t* n_updated, uint8_t* flags, int mem);

#ifdef __cplusplus
}
#endif
#endif
