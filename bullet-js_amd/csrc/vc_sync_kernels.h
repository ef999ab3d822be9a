// vc_sync_kernels.h — read-only sweeps of the K-writer vector-clock table for replica reconciliation (include/bmx_vc_sync.h), gfx950, and the record unpack
// in front of the merge.
//
// k_vc_digest    : per-bucket state digest. One pass over nslots x 64 B, nothing written but 2 x B words.
// k_vc_frontier  : the table's version vector (component-wise maximum of the rows' clocks). One pass, eight words written.
// PredVSlotSync / EmitVRecs : the filtered export as 64-byte records on the select.h skeleton (k_sel_count + k_sel_write).
// k_vc_unpack    : 64-byte records -> the column form the merge kernels (vc_kernels.h) take. No merge kernel knows about records.
//
// A ROW is a slot with id != EMPTY_ID and state != VC_ABSENT (PredVSlotRange's rule). None of the sweeps touches a merge kernel's argument.
//
// How the sweeps read: a slot is four 16-byte quarters { id, field, head | val, state, keyset | clock[0..4) | clock[4..8) }. Lane l of a wave loads quarter
// l & 3 of slot l >> 2 of a ROUND of 16 consecutive slots, so one load instruction of a wave is one contiguous KB (a lane that owned a whole slot would touch
// 64 half-lines with each of its four instructions), and a lane keeps VSYNC_U such loads in flight before it looks at the first. Whether a slot holds a row is
// known to its quarter-0 lane (the id) and its quarter-1 lane (the state): two ballots give every lane the round's row bits.
#pragma once
#include "sync_kernels.h"
#include "vc_kernels.h"
#include "../../include/bmx_vc_sync.h"

namespace bmx {

static_assert(sizeof(bmx_vc_rec) == sizeof(VSlot), "a record is a slot image");

constexpr int VSYNC_U = 8;                                  // 16-byte loads a lane has in flight
constexpr uint32_t VSYNC_ROUND = 16;                        // slots per load instruction of a wave
constexpr uint32_t VSYNC_CHUNK = VSYNC_ROUND * VSYNC_U;     // slots a wave takes per step of its loop (8 KB)

// The row digest of bmx_vc_sync.h: eight chained splitmix64 over val, keyset | state << 32, the eight clock components in pairs, field, id.
__host__ __device__ inline uint64_t vc_row_digest(uint64_t id, uint32_t field, int64_t val, uint32_t state, uint32_t keyset, const uint32_t* c) {
  uint64_t h = splitmix64((uint64_t)val);
  h = splitmix64(h ^ u64_of(keyset, state));
  h = splitmix64(h ^ u64_of(c[0], c[1]));
  h = splitmix64(h ^ u64_of(c[2], c[3]));
  h = splitmix64(h ^ u64_of(c[4], c[5]));
  h = splitmix64(h ^ u64_of(c[6], c[7]));
  h = splitmix64(h ^ (uint64_t)field);
  return splitmix64(h ^ id);
}

// one round's quarter for this lane (slots at and behind nslots read as empty), and the round's row bits: bit 4 s set <=> slot s of the round holds a row
template <bool NT>
__device__ __forceinline__ uint4 vsync_load(const uint4* __restrict__ base, uint64_t s, uint64_t nslots, uint32_t q) {
  if (s < nslots) return load_half<NT>(base + s * 4u + q);
  return q == 0 ? make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ uint64_t vsync_rows(const uint4 v, uint32_t q) {
  const uint64_t m0 = __ballot(q == 0 && !(v.x == 0xFFFFFFFFu && v.y == 0xFFFFFFFFu));
  const uint64_t m1 = __ballot(q == 1 && v.z != VC_ABSENT);
  return m0 & (m1 >> 1);
}

// ---- k_vc_digest ----
// Grid sized to the CUs (two 8-wave workgroups each); every wave walks chunks of 128 consecutive slots. A row costs 8 splitmix64 + 3 mix64 of 64-bit
// multiplies (quarter-rate VALU), the tables run at load <= 0.5, and a row's quarters sit in four lanes: so the wave first PACKS its rows, quarter by quarter,
// into a stack of its own in LDS (rank from the row bits: no atomics, wave-level ordering only, no barrier) and hashes 64 of them at a time, one whole row per
// lane, with every lane busy; what is left over stays on the stack for the next chunk. The stack is quarter-major (st[quarter][entry]): the packing stores of a
// quarter's lanes and the 16-byte reads of the hashing lanes are both consecutive. A round adds at most 16 rows to fewer than 64, so 80 entries hold it.
// LDS_ACC (L <= 10): 64-bit LDS adds into the workgroup's 1024 sums + 32-bit counts (12 KB), flushed once at the end — non-zero buckets only — with no-return
// global atomics. Otherwise (L 11..16, the slow form) one pair of no-return global atomics per row. (k_digest_buckets' split, for its reasons.)
constexpr int VDIG_THREADS = 512;
constexpr int VDIG_WAVES = VDIG_THREADS / 64;
constexpr int VDIG_STACK = 64 + VSYNC_ROUND;   // rows a wave's stack can hold: < 64 left over + the 16 of one round

template <bool LDS_ACC>
__device__ __forceinline__ void vdigest_row(const uint4 a, const uint4 b, const uint4 c0, const uint4 c1, uint32_t L, unsigned long long* s_sum, uint32_t* s_cnt,
                                            unsigned long long* __restrict__ sums, unsigned long long* __restrict__ counts) {
  const uint64_t id = u64_of(a.x, a.y);
  const uint32_t field = a.z;
  const uint32_t c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const uint64_t d = vc_row_digest(id, field, i64_of(b.x, b.y), b.z, b.w, c);     // (a.w, the claim word, is no part of the row)
  const uint32_t bk = key_bucket(id, field, L);
  if (LDS_ACC) { atomicAdd(&s_sum[bk], (unsigned long long)d); atomicAdd(&s_cnt[bk], 1u); }
  else { atomicAdd(&sums[bk], (unsigned long long)d); atomicAdd(&counts[bk], 1ull); }
}

template <bool LDS_ACC, bool NT>
__global__ __launch_bounds__(VDIG_THREADS) void k_vc_digest(const VSlot* __restrict__ slots, uint64_t nslots, uint32_t L, unsigned long long* __restrict__ sums,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_sum[LDS_ACC ? (1u << DIG_LDS_LOG2) : 1];
  __shared__ uint32_t s_cnt[LDS_ACC ? (1u << DIG_LDS_LOG2) : 1];
  __shared__ uint4 st[VDIG_WAVES][4][VDIG_STACK];
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6, q = lane & 3u, sub = lane >> 2, sh = lane & ~3u;
  if (LDS_ACC) {
    for (uint32_t b = threadIdx.x; b < (1u << DIG_LDS_LOG2); b += VDIG_THREADS) { s_sum[b] = 0ull; s_cnt[b] = 0u; }
    __syncthreads();
  }
  uint4(*sq)[VDIG_STACK] = st[w];
  const uint4* base = reinterpret_cast<const uint4*>(slots);
  uint32_t fill = 0;                                               // rows on the wave's stack (the same in every lane)
  const uint64_t nchunks = (nslots + VSYNC_CHUNK - 1) / VSYNC_CHUNK;
  for (uint64_t c = (uint64_t)blockIdx.x * VDIG_WAVES + w; c < nchunks; c += (uint64_t)gridDim.x * VDIG_WAVES) {
    uint4 v[VSYNC_U];
#pragma unroll
    for (int u = 0; u < VSYNC_U; u++) v[u] = vsync_load<NT>(base, c * VSYNC_CHUNK + (uint64_t)u * VSYNC_ROUND + sub, nslots, q);
#pragma unroll
    for (int u = 0; u < VSYNC_U; u++) {
      const uint64_t rows = vsync_rows(v[u], q);
      if ((rows >> sh) & 1ull) sq[q][fill + (uint32_t)__popcll(rows & ((1ull << sh) - 1ull))] = v[u];
      fill += (uint32_t)__popcll(rows);
      if (fill >= 64u) {                                           // (uniform) the top 64 rows of the stack, one per lane
        wave_lds_sync();
        fill -= 64u;
        const uint4 a = sq[0][fill + lane], b = sq[1][fill + lane], c0 = sq[2][fill + lane], c1 = sq[3][fill + lane];
        wave_lds_sync();                                           // the next round's stores land on these entries
        vdigest_row<LDS_ACC>(a, b, c0, c1, L, s_sum, s_cnt, sums, counts);
      }
    }
  }
  wave_lds_sync();
  if (lane < fill) vdigest_row<LDS_ACC>(sq[0][lane], sq[1][lane], sq[2][lane], sq[3][lane], L, s_sum, s_cnt, sums, counts);
  if (LDS_ACC) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < (1u << L); b += VDIG_THREADS) {
      const uint32_t n = s_cnt[b];
      if (n) { atomicAdd(&sums[b], s_sum[b]); atomicAdd(&counts[b], (unsigned long long)n); }
    }
  }
}

// ---- k_vc_frontier ----
// The same walk. The lanes of quarters 2 and 3 keep the running maxima of the four components they load (rows only); lanes of equal quarter fold with four
// xor shuffles, the waves through 32 words of LDS, and the workgroup leaves with at most eight no-return atomicMax into a vector the call zeroed in stream order.
constexpr int VFR_THREADS = 256;
constexpr int VFR_WAVES = VFR_THREADS / 64;

__device__ __forceinline__ uint32_t vfr_fold(uint32_t x) {
  x = max(x, (uint32_t)__shfl_xor((int)x, 4)); x = max(x, (uint32_t)__shfl_xor((int)x, 8));
  x = max(x, (uint32_t)__shfl_xor((int)x, 16)); x = max(x, (uint32_t)__shfl_xor((int)x, 32));
  return x;
}

template <bool NT>
__global__ __launch_bounds__(VFR_THREADS) void k_vc_frontier(const VSlot* __restrict__ slots, uint64_t nslots, uint32_t* __restrict__ out8) {
  __shared__ uint32_t s_max[VFR_WAVES][VC_MAXK];
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6, q = lane & 3u, sub = lane >> 2, sh = lane & ~3u;
  const uint4* base = reinterpret_cast<const uint4*>(slots);
  uint32_t mx = 0, my = 0, mz = 0, mw = 0;
  const uint64_t nchunks = (nslots + VSYNC_CHUNK - 1) / VSYNC_CHUNK;
  for (uint64_t c = (uint64_t)blockIdx.x * VFR_WAVES + w; c < nchunks; c += (uint64_t)gridDim.x * VFR_WAVES) {
    uint4 v[VSYNC_U];
#pragma unroll
    for (int u = 0; u < VSYNC_U; u++) v[u] = vsync_load<NT>(base, c * VSYNC_CHUNK + (uint64_t)u * VSYNC_ROUND + sub, nslots, q);
#pragma unroll
    for (int u = 0; u < VSYNC_U; u++) {
      const uint64_t rows = vsync_rows(v[u], q);
      if (((rows >> sh) & 1ull) && q >= 2u) { mx = max(mx, v[u].x); my = max(my, v[u].y); mz = max(mz, v[u].z); mw = max(mw, v[u].w); }
    }
  }
  mx = vfr_fold(mx); my = vfr_fold(my); mz = vfr_fold(mz); mw = vfr_fold(mw);
  if (lane == 2u || lane == 3u) { uint32_t* d = &s_max[w][4u * (lane - 2u)]; d[0] = mx; d[1] = my; d[2] = mz; d[3] = mw; }
  __syncthreads();
  if (threadIdx.x < (uint32_t)VC_MAXK) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < VFR_WAVES; i++) m = max(m, s_max[i][threadIdx.x]);
    if (m) atomicMax(&out8[threadIdx.x], m);
  }
}

// ---- filtered export (bmx_vc_export_rows) ----
struct PredVSlotSync {  // rows whose key bucket is wanted and, under a frontier, whose clock exceeds it in some component k < K
  static constexpr int E = 2;
  const VSlot* slots; const unsigned long long* bits /* 2^L bits, nullptr = every bucket */; uint32_t L, K, use_fr; uint32_t fr[VC_MAXK];
  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const uint64_t s = first + e;
      if (s < n) {
        const uint4* q = reinterpret_cast<const uint4*>(slots + s);
        const uint4 a = q[0];
        if (!(a.x == 0xFFFFFFFFu && a.y == 0xFFFFFFFFu) && q[1].z != VC_ABSENT) {
          bool want = true;
          if (bits) { const uint32_t bk = key_bucket(u64_of(a.x, a.y), a.z, L); want = (bits[bk >> 6] >> (bk & 63u)) & 1ull; }
          if (want && use_fr) {
            const uint4 c0 = q[2], c1 = q[3];
            const uint32_t c[VC_MAXK] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            bool ahead = false;
#pragma unroll
            for (int k = 0; k < VC_MAXK; k++) if ((uint32_t)k < K && c[k] > fr[k]) ahead = true;
            want = ahead;
          }
          if (want) m |= 1u << e;
        }
      }
    }
    return m;
  }
};
struct EmitVRecs {  // slot -> one 64-byte record (four 16-byte stores), bounded by cap; aux = 0 in place of the claim word
  const VSlot* slots; uint64_t cap; bmx_vc_rec* out;
  __device__ void operator()(uint64_t pos, uint64_t s) const {
    if (pos >= cap) return;
    const uint4* q = reinterpret_cast<const uint4*>(slots + s);
    uint4 a = q[0];
    const uint4 b = q[1], c0 = q[2], c1 = q[3];
    a.w = 0u;
    uint4* o = reinterpret_cast<uint4*>(out + pos);
    o[0] = a; o[1] = b; o[2] = c0; o[3] = c1;
  }
};

// ---- k_vc_unpack (bmx_vc_merge_records) ----
// 256 records (16 KB) per workgroup: read as 1024 consecutive 16-byte words, four per thread, all in flight, into LDS; then thread j owns record j and writes
// the columns, consecutive threads on consecutive elements (the clocks K words apart). A record with a non-zero component at k >= K cannot be said in the
// table's columns: its id becomes the reserved id, which k_vc_link refuses as out of domain (ST_RANGE) like any other.
constexpr int VUNP_THREADS = 256;

__global__ __launch_bounds__(VUNP_THREADS) void k_vc_unpack(const bmx_vc_rec* __restrict__ recs, uint32_t n, uint32_t K, uint64_t* __restrict__ id, uint32_t* __restrict__ field,
                                                            uint32_t* __restrict__ clocks, uint32_t* __restrict__ keysets, int64_t* __restrict__ val) {
  __shared__ uint4 s_rec[VUNP_THREADS * 4];
  const uint32_t r0 = blockIdx.x * (uint32_t)VUNP_THREADS;
  const uint32_t live = min((uint32_t)VUNP_THREADS, n - r0) * 4u;                  // 16-byte words of this workgroup's records
  const uint4* src = reinterpret_cast<const uint4*>(recs + r0);
  uint4 v[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const uint32_t i = (uint32_t)u * VUNP_THREADS + threadIdx.x; v[u] = i < live ? src[i] : make_uint4(0u, 0u, 0u, 0u); }
#pragma unroll
  for (int u = 0; u < 4; u++) s_rec[(uint32_t)u * VUNP_THREADS + threadIdx.x] = v[u];
  __syncthreads();
  const uint32_t j = r0 + threadIdx.x;
  if (j >= n) return;
  const uint4 a = s_rec[4u * threadIdx.x], b = s_rec[4u * threadIdx.x + 1u], c0 = s_rec[4u * threadIdx.x + 2u], c1 = s_rec[4u * threadIdx.x + 3u];
  const uint32_t c[VC_MAXK] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  bool beyond = false;
#pragma unroll
  for (int k = 0; k < VC_MAXK; k++) {
    if ((uint32_t)k < K) clocks[(size_t)j * K + k] = c[k];
    else if (c[k] != 0u) beyond = true;
  }
  id[j] = beyond ? EMPTY_ID : u64_of(a.x, a.y);
  field[j] = a.z;
  val[j] = i64_of(b.x, b.y);
  keysets[j] = b.w;
}

}  // namespace bmx
