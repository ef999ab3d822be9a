// agg_kernels.h — aggregate queries (bmx.h bmx_scan_aggregate): count, sum, min, max and group-by over the nodes a declarative filter selects, gfx950.
//
// The selection is bmx_scan_filter's (term 0 on the index column, the other terms probed in the table); what differs is the end: nothing is emitted. A
// matching row adds {1, value of the measure field} to the record of its group, and the only thing written is one 48-byte record per group — no id
// output, no mask, nothing proportional to the match count.
//
// k_agg_sweep<T, PROBE, G> : one read of term 0's value column (T = int32_t / int64_t, 16-byte loads, AGG_U of them in flight per lane).
//                            PROBE = false is the single-field form (one term, measure and group each that field or none): it touches neither the id
//                            column nor the table and carries no probe code.
// k_agg_view<T, G>         : the candidates are the run of the value-ordered view for term 0's range (main - pending deleted + pending inserted, enumerated
//                            as k_ordered_filter_p does): O(log R + candidates).
// k_agg_finish             : composes the exact 128-bit sums and delivers the records; it also leaves the accumulators clean for the next query.
//
// G = 0: no grouping. A lane reduces into registers, a wave with shuffles, the workgroup through LDS: one set of no-return global atomics per workgroup.
// G = 1: 1..AGG_LDS_GROUPS groups. The workgroup accumulates into its LDS copy of the records (40 bytes per group) and flushes the non-empty ones once
//        (k_digest_buckets' pattern): at most 6 memory-side atomics per group and workgroup, whatever the column holds.
// G = 2: AGG_LDS_GROUPS + 1 .. 65536 groups, the SLOW form: no-return global atomics per matching row.
//
// The sum is exact: every workgroup adds sum((uint32)val) as u64 and sum(val >> 32) as i64 (|val| <= 2^53 - 1 and fewer than 2^32 rows: below 2^64 and 2^53),
// k_agg_finish composes (hi << 32) + lo in 128 bits. Integer sums do not depend on the order of the adds: the answer is bit-reproducible.
#pragma once
#include "select.h"
#include "scan_kernels.h"
#include "view_kernels.h"
#include "../../include/bmx.h"

namespace bmx {

constexpr int AGG_THREADS = 512;
constexpr int AGG_WAVES = AGG_THREADS / 64;
constexpr int AGG_U = 4;                        // 16-byte loads of the value column a lane has in flight
constexpr uint32_t AGG_LDS_GROUPS = 1024;       // G = 1 up to here: 1025 records x 40 B = 41 KB of LDS per workgroup, two workgroups per CU
constexpr uint32_t AGG_SRC_NONE = 0xFFu;        // AggArgs::m_src / g_src: no measure / no grouping
constexpr uint32_t AGG_SRC_PROBE = 0xFEu;       // ... the field is none of the terms': a probe of its own (0..7: the value term k read anyway)

// accumulator of one group in device memory; the layout of bmx_agg with the sum still in its two partial words
struct AggRaw { unsigned long long nm, n; long long mn, mx; unsigned long long slo; long long shi; };
static_assert(sizeof(AggRaw) == sizeof(bmx_agg) && sizeof(AggRaw) == 48, "one record per group");

struct AggArgs {
  const Slot* slots; uint64_t nslots;
  AggRaw* acc;
  int64_t group_lo; uint32_t ngroups;
  uint32_t measure, group;                      // field hashes (read where m_src / g_src == AGG_SRC_PROBE)
  uint32_t m_src, g_src;
  uint32_t nterms; bmx_term t[MAX_TERMS];       // t[k].lo >= -VAL_MAX: a tombstone matches no term
};

struct AggLane { unsigned long long nm = 0, n = 0; long long mn = INT64_MAX, mx = INT64_MIN; unsigned long long slo = 0; long long shi = 0; };

template <int G>
struct AggLds {                                 // G = 1: the workgroup's records; G = 0: one partial per wave; G = 2: nothing
  static constexpr uint32_t N = G == 1 ? AGG_LDS_GROUPS + 1 : (G == 0 ? AGG_WAVES : 1);
  uint32_t nm[N], n[N];
  long long mn[N], mx[N];
  unsigned long long slo[N]; long long shi[N];
};

// the row (id, field) of the table: false = absent; x = its value (VAL_DELETED for a tombstone), ts = its clock (a tombstone's is the clock of the delete):
// the slot's second 16 bytes hold both, so the clock costs no further load
__device__ __forceinline__ bool agg_probe_ts(const Slot* __restrict__ slots, uint64_t nslots, uint64_t id, uint32_t field, int64_t& x, int64_t& ts) {
  ProbeSeq<4> ps(id, field, nslots);
  for (uint64_t p = 0; p < nslots; ++p) {
    const uint4* q = reinterpret_cast<const uint4*>(slots + ps.slot());
    const uint4 lo = q[0];
    const uint64_t sid = u64_of(lo.x, lo.y);
    if (sid == EMPTY_ID) return false;
    if (sid == id && lo.z == field) {
      const uint4 hi = q[1];
      ts = ts_value(i64_of(hi.x, hi.y));
      x = i64_of(hi.z, hi.w);
      return true;
    }
    ps.next();
  }
  return false;
}
// ... for the callers that want the value alone
__device__ __forceinline__ bool agg_probe(const Slot* __restrict__ slots, uint64_t nslots, uint64_t id, uint32_t field, int64_t& x) {
  int64_t ts;
  return agg_probe_ts(slots, nslots, id, field, x, ts);
}

// one matching row into the record of group g
template <int G>
__device__ __forceinline__ void agg_add(const AggArgs& A, AggLane& L, AggLds<G>& S, uint32_t g, bool have_m, int64_t mval) {
  const unsigned long long lo = (unsigned long long)(uint32_t)mval; const long long hi = mval >> 32;
  if (G == 0) {
    L.nm++;
    if (have_m) { L.n++; L.slo += lo; L.shi += hi; L.mn = mval < L.mn ? mval : L.mn; L.mx = mval > L.mx ? mval : L.mx; }
  } else if (G == 1) {
    atomicAdd(&S.nm[g], 1u);
    if (have_m) {
      if (A.m_src == AGG_SRC_PROBE) atomicAdd(&S.n[g], 1u);          // (otherwise every match has its measure: n == n_match, set by k_agg_finish)
      atomicAdd(&S.slo[g], lo);
      if (hi) atomicAdd(reinterpret_cast<unsigned long long*>(&S.shi[g]), (unsigned long long)hi);
      atomicMin(&S.mn[g], (long long)mval); atomicMax(&S.mx[g], (long long)mval);
    }
  } else {
    AggRaw* r = A.acc + g;
    atomicAdd(&r->nm, 1ull);
    if (have_m) {
      if (A.m_src == AGG_SRC_PROBE) atomicAdd(&r->n, 1ull);
      atomicAdd(&r->slo, lo);
      if (hi) atomicAdd(reinterpret_cast<unsigned long long*>(&r->shi), (unsigned long long)hi);
      atomicMin(&r->mn, (long long)mval); atomicMax(&r->mx, (long long)mval);
    }
  }
}

// a row whose term-0 value v0 is inside term 0's range: the other terms, the measure and the group value (one probe yields both the predicate and the
// value when a term's field is also the measure or the group field), then the add
template <int G, bool PROBE>
__device__ __forceinline__ void agg_row(const AggArgs& A, int64_t v0, uint64_t id, AggLane& L, AggLds<G>& S) {
  int64_t mval = v0, gval = v0;
  bool have_m = A.m_src == 0u, have_g = A.g_src == 0u;
  if (PROBE) {
    for (uint32_t k = 1; k < A.nterms; k++) {
      int64_t x;
      if (!agg_probe(A.slots, A.nslots, id, A.t[k].field, x) || x < A.t[k].lo || x > A.t[k].hi) return;
      if (A.m_src == k) { mval = x; have_m = true; }
      if (A.g_src == k) { gval = x; have_g = true; }
    }
    if (A.m_src == AGG_SRC_PROBE) { int64_t x; if (agg_probe(A.slots, A.nslots, id, A.measure, x) && x != VAL_DELETED) { mval = x; have_m = true; } }
    if (A.g_src == AGG_SRC_PROBE) { int64_t x; if (agg_probe(A.slots, A.nslots, id, A.group, x) && x != VAL_DELETED) { gval = x; have_g = true; } }
  }
  uint32_t g = 0;
  if (G) {   // (the difference of two int64 is exact mod 2^64 once gval >= group_lo)
    const uint64_t d = (uint64_t)gval - (uint64_t)A.group_lo;
    g = (have_g && gval >= A.group_lo && d < (uint64_t)A.ngroups) ? (uint32_t)d : A.ngroups;
  }
  agg_add<G>(A, L, S, g, have_m, mval);
}

template <int G>
__device__ __forceinline__ void agg_begin(const AggArgs& A, AggLds<G>& S) {
  if (G == 1) {
    for (uint32_t g = threadIdx.x; g <= A.ngroups; g += AGG_THREADS) { S.nm[g] = 0u; S.n[g] = 0u; S.mn[g] = INT64_MAX; S.mx[g] = INT64_MIN; S.slo[g] = 0ull; S.shi[g] = 0ll; }
    __syncthreads();
  }
}
__device__ __forceinline__ void agg_flush_one(AggRaw* r, unsigned long long nm, unsigned long long n, long long mn, long long mx, unsigned long long slo, long long shi) {
  atomicAdd(&r->nm, nm);
  if (n) atomicAdd(&r->n, n);
  if (slo) atomicAdd(&r->slo, slo);
  if (shi) atomicAdd(reinterpret_cast<unsigned long long*>(&r->shi), (unsigned long long)shi);
  if (mn != INT64_MAX) { atomicMin(&r->mn, mn); atomicMax(&r->mx, mx); }      // (no value is INT64_MAX: a measure was seen)
}
// every lane of the workgroup, once, behind its last row
template <int G>
__device__ __forceinline__ void agg_end(const AggArgs& A, AggLane& L, AggLds<G>& S) {
  if (G == 0) {
    for (int d = 32; d >= 1; d >>= 1) {
      L.nm += __shfl_xor(L.nm, d); L.n += __shfl_xor(L.n, d); L.slo += __shfl_xor(L.slo, d); L.shi += __shfl_xor(L.shi, d);
      const long long a = __shfl_xor(L.mn, d), b = __shfl_xor(L.mx, d);
      L.mn = a < L.mn ? a : L.mn; L.mx = b > L.mx ? b : L.mx;
    }
    const uint32_t w = threadIdx.x >> 6;
    // (a wave has fewer than 2^32 rows: the two counts fit the 32-bit LDS words)
    if ((threadIdx.x & 63u) == 0) { S.nm[w] = (uint32_t)L.nm; S.n[w] = (uint32_t)L.n; S.mn[w] = L.mn; S.mx[w] = L.mx; S.slo[w] = L.slo; S.shi[w] = L.shi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long nm = 0, n = 0, slo = 0; long long mn = INT64_MAX, mx = INT64_MIN, shi = 0;
#pragma unroll
      for (int i = 0; i < AGG_WAVES; i++) { nm += S.nm[i]; n += S.n[i]; slo += S.slo[i]; shi += S.shi[i]; mn = S.mn[i] < mn ? S.mn[i] : mn; mx = S.mx[i] > mx ? S.mx[i] : mx; }
      if (nm) agg_flush_one(A.acc, nm, n, mn, mx, slo, shi);
    }
  } else if (G == 1) {
    __syncthreads();
    for (uint32_t g = threadIdx.x; g <= A.ngroups; g += AGG_THREADS) {
      const uint32_t nm = S.nm[g];
      if (nm) agg_flush_one(A.acc + g, nm, S.n[g], S.mn[g], S.mx[g], S.slo[g], S.shi[g]);
    }
  }
}

template <class T, bool PROBE, int G>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_sweep(const T* __restrict__ col, const uint64_t* __restrict__ ids, uint64_t n, T lo, T hi, uint32_t nt, AggArgs A) {
  constexpr int E = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(E)));
  __shared__ AggLds<G> S;
  AggLane L;
  agg_begin<G>(A, S);
  const uint64_t nv = n / E;                                  // whole 16-byte units; the ragged tail is block 0's
  for (uint64_t b = (uint64_t)blockIdx.x * (AGG_THREADS * AGG_U); b < nv; b += (uint64_t)gridDim.x * (AGG_THREADS * AGG_U)) {
    vec_t x[AGG_U];
#pragma unroll
    for (int u = 0; u < AGG_U; u++) {
      const uint64_t i = b + (uint64_t)u * AGG_THREADS + threadIdx.x;
      if (i < nv) x[u] = nt ? __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(col) + i) : reinterpret_cast<const vec_t*>(col)[i];
      else { const vec_t z = {}; x[u] = z; }
    }
#pragma unroll
    for (int u = 0; u < AGG_U; u++) {
      const uint64_t i = b + (uint64_t)u * AGG_THREADS + threadIdx.x;
      if (i >= nv) continue;
#pragma unroll
      for (int e = 0; e < E; e++) {
        const T v = x[u][e];
        if (v >= lo && v <= hi) agg_row<G, PROBE>(A, (int64_t)v, PROBE ? ids[i * E + e] : 0ull, L, S);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < n - nv * E) {
    const uint64_t i = nv * E + threadIdx.x;
    const T v = col[i];
    if (v >= lo && v <= hi) agg_row<G, PROBE>(A, (int64_t)v, PROBE ? ids[i] : 0ull, L, S);
  }
  agg_end<G>(A, L, S);
}

// the view's run for [lo, hi] (ab: k_ordered_bounds / k_ordered_bounds_p): main's keys that are not pending deleted, then the pending inserted keys. need_id = 0:
// the single-field form, nothing but the view's value column is read.
template <class T, int G>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_view(const T* __restrict__ v, const uint32_t* __restrict__ p, const uint64_t* __restrict__ s_ids, const T* __restrict__ dv,
                                                          const uint32_t* __restrict__ dp, const T* __restrict__ iv, const uint64_t* __restrict__ i_ids,
                                                          const unsigned long long* __restrict__ ab, uint32_t pending, uint32_t need_id, AggArgs A) {
  __shared__ AggLds<G> S;
  const uint64_t a = ab[0], m = ab[1] - a;
  const uint64_t da = pending ? ab[2] : 0, db = pending ? ab[3] : 0, ia = pending ? ab[4] : 0, mi = pending ? ab[5] - ia : 0;
  const uint64_t tot = m + mi;
  if ((uint64_t)blockIdx.x * AGG_THREADS >= tot) return;      // (uniform) a workgroup beyond the run has nothing to add
  AggLane L;
  agg_begin<G>(A, S);
  for (uint64_t i = (uint64_t)blockIdx.x * AGG_THREADS + threadIdx.x; i < tot; i += (uint64_t)gridDim.x * AGG_THREADS) {
    if (i < m) {
      const T kv = v[a + i];
      if (da != db) {
        const uint32_t kp = p[a + i];
        const uint64_t r = vk_bound<T>(dv, dp, da, db, kv, kp);
        if (r < db && dv[r] == kv && dp[r] == kp) continue;
      }
      agg_row<G, true>(A, (int64_t)kv, need_id ? s_ids[a + i] : 0ull, L, S);
    } else {
      const uint64_t j = ia + (i - m);
      agg_row<G, true>(A, (int64_t)iv[j], need_id ? i_ids[j] : 0ull, L, S);
    }
  }
  agg_end<G>(A, L, S);
}

// accumulators -> records (out: device memory), and the accumulators back to their empty state for the next query. n_is_match: every match had its measure
// (or there is none): n = n_match.
__global__ __launch_bounds__(256) void k_agg_finish(AggRaw* __restrict__ acc, bmx_agg* __restrict__ out, uint32_t nrec, uint32_t n_is_match) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < nrec; r += gridDim.x * 256u) {
    const AggRaw x = acc[r];
    const __int128 s = ((__int128)x.shi << 32) + (__int128)x.slo;
    bmx_agg o;
    o.n_match = x.nm; o.n = n_is_match ? x.nm : x.n; o.min = x.mn; o.max = x.mx;
    o.sum_lo = (uint64_t)s; o.sum_hi = (int64_t)(s >> 64);
    out[r] = o;
    acc[r] = AggRaw{0ull, 0ull, INT64_MAX, INT64_MIN, 0ull, 0ll};
  }
}
__global__ __launch_bounds__(256) void k_agg_clear(AggRaw* __restrict__ acc, uint32_t nrec) {
  for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < nrec; r += gridDim.x * 256u) acc[r] = AggRaw{0ull, 0ull, INT64_MAX, INT64_MIN, 0ull, 0ll};
}

}  // namespace bmx
