// sync_kernels.h — read-only sweeps of the resident table for replica reconciliation (bmx.h "replica reconciliation"), gfx950.
//
// k_digest_buckets : per-bucket state digest. One pass over nslots x 32 B, nothing written but 2 x B words.
// PredSlotSync / EmitRecs : the filtered export as 32-byte delta records on the select.h skeleton (k_sel_count + k_sel_write).
//
// Neither touches a merge kernel's argument or the index/view state: they read slots exactly as the row dump does.
#pragma once
#include "select.h"
#include "../../include/bmx.h"

namespace bmx {

typedef uint32_t sync_u32x4 __attribute__((ext_vector_type(4)));
// one 16-byte half of a slot; nt: the table is larger than the Infinity Cache and read once (same rule as the scans' value columns)
template <bool NT>
__device__ __forceinline__ uint4 load_half(const uint4* p) {
  if (NT) { const sync_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const sync_u32x4*>(p)); return make_uint4(v.x, v.y, v.z, v.w); }
  return *p;
}

// The project's row digest (oracle/bmx_oracle.c orc_row_digest, oracle/oracle.py rows_digest, oracle/gen_golden.js rowDigest), restated: four chained
// splitmix64 over val, ts, field, id. A state digest is the sum mod 2^64 of it over the rows, so it does not depend on their order.
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t row_digest(uint64_t id, uint32_t field, int64_t ts, int64_t val) {
  uint64_t h = splitmix64((uint64_t)val);
  h = splitmix64(h ^ (uint64_t)ts);
  h = splitmix64(h ^ (uint64_t)field);
  return splitmix64(h ^ id);
}

// ---- k_digest_buckets ----
// Grid sized to the CUs (two 8-wave workgroups each), every wave walks chunks of 64 x DIG_U consecutive slots with all 2 x DIG_U 16-byte loads of a lane in
// flight before the first is looked at. Hashing a row costs ~14 64-bit multiplies (quarter-rate VALU), and at the load factors the tables run at only every
// second to fourth slot holds one: hashing under the occupancy branch would pay a full wave instruction stream for a quarter of the lanes. So the wave first
// PACKS its rows into 4 KB of LDS of its own (ballot + mbcnt rank, two 16-byte LDS stores per row; wave-level ordering only, no barrier) and hashes 64 of them
// at a time with every lane busy; what is left over stays on the stack for the next chunk.
// LDS_ACC (L <= 10): 64-bit LDS adds into the workgroup's 1024 sums + 32-bit counts (12 KB), flushed once at the end — non-zero buckets only — with no-return
// global atomics: at most 2 x B memory-side requests per workgroup, whatever the table holds. Otherwise (L 11..16, the slow form) one pair of no-return global
// atomics per row.
constexpr int DIG_THREADS = 512;
constexpr int DIG_WAVES = DIG_THREADS / 64;
constexpr int DIG_U = 4;
constexpr uint32_t DIG_LDS_LOG2 = 10;
constexpr int DIG_STACK = 128;             // rows a wave's stack can hold: < 64 left over + 64 of one load round

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <bool LDS_ACC>
__device__ __forceinline__ void digest_row(const uint4 a, const uint4 b, uint32_t L, unsigned long long* s_sum, uint32_t* s_cnt,
                                           unsigned long long* __restrict__ sums, unsigned long long* __restrict__ counts) {
  const uint64_t id = u64_of(a.x, a.y);
  const uint32_t field = a.z;
  const uint64_t d = row_digest(id, field, ts_value(i64_of(b.x, b.y)), i64_of(b.z, b.w));   // the epoch mark of a row created by the running epoch is no part of its clock
  const uint32_t bk = key_bucket(id, field, L);
  if (LDS_ACC) { atomicAdd(&s_sum[bk], (unsigned long long)d); atomicAdd(&s_cnt[bk], 1u); }
  else { atomicAdd(&sums[bk], (unsigned long long)d); atomicAdd(&counts[bk], 1ull); }
}

template <bool LDS_ACC, bool NT>
__global__ __launch_bounds__(DIG_THREADS) void k_digest_buckets(const Slot* __restrict__ slots, uint64_t nslots, uint32_t L, uint32_t tombstones,
                                                                unsigned long long* __restrict__ sums, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_sum[LDS_ACC ? (1u << DIG_LDS_LOG2) : 1];
  __shared__ uint32_t s_cnt[LDS_ACC ? (1u << DIG_LDS_LOG2) : 1];
  __shared__ uint4 st_lo[DIG_WAVES][DIG_STACK], st_hi[DIG_WAVES][DIG_STACK];
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  if (LDS_ACC) {
    for (uint32_t b = threadIdx.x; b < (1u << DIG_LDS_LOG2); b += DIG_THREADS) { s_sum[b] = 0ull; s_cnt[b] = 0u; }
    __syncthreads();
  }
  uint4* slo = st_lo[w]; uint4* shi = st_hi[w];
  uint32_t fill = 0;                                               // rows on the wave's stack (the same in every lane)
  constexpr uint64_t CHUNK = 64ull * DIG_U;
  const uint64_t nchunks = (nslots + CHUNK - 1) / CHUNK;
  for (uint64_t c = (uint64_t)blockIdx.x * DIG_WAVES + w; c < nchunks; c += (uint64_t)gridDim.x * DIG_WAVES) {
    uint4 lo[DIG_U], hi[DIG_U];
#pragma unroll
    for (int u = 0; u < DIG_U; u++) {
      const uint64_t s = c * CHUNK + (uint64_t)u * 64u + lane;
      if (s < nslots) {
        const uint4* q = reinterpret_cast<const uint4*>(slots + s);
        lo[u] = load_half<NT>(q); hi[u] = load_half<NT>(q + 1);
      } else { lo[u] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u); hi[u] = make_uint4(0u, 0u, 0u, 0u); }
    }
#pragma unroll
    for (int u = 0; u < DIG_U; u++) {
      const bool occ = !(lo[u].x == 0xFFFFFFFFu && lo[u].y == 0xFFFFFFFFu);
      const bool sel = occ && (tombstones || i64_of(hi[u].z, hi[u].w) != VAL_DELETED);
      const uint64_t m = __ballot(sel);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (sel) { slo[fill + rank] = lo[u]; shi[fill + rank] = hi[u]; }
      fill += (uint32_t)__popcll(m);
      if (fill >= 64u) {                                           // (uniform) the top 64 rows of the stack, one per lane
        wave_lds_sync();
        fill -= 64u;
        const uint4 a = slo[fill + lane], b = shi[fill + lane];
        wave_lds_sync();                                           // the next round's stores land on these entries
        digest_row<LDS_ACC>(a, b, L, s_sum, s_cnt, sums, counts);
      }
    }
  }
  wave_lds_sync();
  if (lane < fill) digest_row<LDS_ACC>(slo[lane], shi[lane], L, s_sum, s_cnt, sums, counts);
  if (LDS_ACC) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < (1u << L); b += DIG_THREADS) {
      const uint32_t n = s_cnt[b];
      if (n) { atomicAdd(&sums[b], s_sum[b]); atomicAdd(&counts[b], (unsigned long long)n); }
    }
  }
}

// ---- filtered export (bmx_export_rows) ----
struct PredSlotSync {  // occupied slots of one kind (data rows, or tombstones) with clock >= since whose key bucket is wanted
  static constexpr int E = 2;
  const Slot* slots; int64_t since; const unsigned long long* bits /* 2^L bits, nullptr = every bucket */; uint32_t L; bool tombs; bool nt;
  __device__ uint32_t mask(uint64_t first, uint64_t n) const {
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const uint64_t s = first + e;
      if (s < n) {
        const uint4* q = reinterpret_cast<const uint4*>(slots + s);
        uint4 lo, hi;
        if (nt) { lo = load_half<true>(q); hi = load_half<true>(q + 1); } else { lo = q[0]; hi = q[1]; }
        const bool occ = !(lo.x == 0xFFFFFFFFu && lo.y == 0xFFFFFFFFu);
        if (occ && (i64_of(hi.z, hi.w) == VAL_DELETED) == tombs && ts_value(i64_of(hi.x, hi.y)) >= since) {
          bool want = true;
          if (bits) { const uint32_t bk = key_bucket(u64_of(lo.x, lo.y), lo.z, L); want = (bits[bk >> 6] >> (bk & 63u)) & 1ull; }
          if (want) m |= 1u << e;
        }
      }
    }
    return m;
  }
};
struct EmitRecs {  // slot -> one 32-byte record (two 16-byte stores), bounded by cap; aux = 0, the clock without its epoch mark
  const Slot* slots; uint64_t cap; bmx_delta_rec* out;
  __device__ void operator()(uint64_t pos, uint64_t s) const {
    if (pos >= cap) return;
    const uint4* q = reinterpret_cast<const uint4*>(slots + s);
    uint4 lo = q[0], hi = q[1];
    lo.w = 0u;
    hi.y &= (uint32_t)(TS_VALUE_MASK >> 32);
    uint4* o = reinterpret_cast<uint4*>(out + pos);
    o[0] = lo; o[1] = hi;
  }
};

}  // namespace bmx
