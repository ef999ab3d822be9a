// Microbenchmark (round 6): can a winning delta of a resident row claim the head AND write (ts,val) in ONE memory-side request?
// A slot is four aligned 8-byte words { id | field,head | ts | val }; words 1..3 lie in one 64-byte granule. 1M random slots, 84 % written.
//   A        (today's mix)  32-B slot read, one-lane 32-bit exchange on head, plain 16-B store of (ts,val)
//   B        (team form)    the same read, then ONE returning 64-bit swap instruction per 16 deltas: lanes 4i, 4i+1, 4i+2 write words 1, 2, 3 of
//                           delta i's slot, lane 4i+3 is off; operands reach the team by __shfl, the old head goes back the same way; four rounds per wave
//   B-split  (control)      the same three swaps as three separate instructions of the delta's own lane
// Also the tear check the team form needs: a plain aligned 16-B load of (ts,val) must never see one word of a team swap without the other
// (writers swap (tag, x, ~x ^ K) into hot slots, readers load; the control issues the three swaps as three instructions and must tear).
//   team_claim_micro          timings (interleaved repeats) + tear check
//   team_claim_micro --pmc    three launches of each variant on the 1408 MB table, for a counter pass (rocprofv3 --pmc ... -- team_claim_micro --pmc)
// Not part of the product path.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("HIP error %s at %d\n",hipGetErrorString(e),__LINE__); exit(1);} }while(0)
__device__ __forceinline__ uint64_t mix64(uint64_t x){ x^=x>>33; x*=0xff51afd7ed558ccdULL; x^=x>>33; x*=0xc4ceb9fe1a85ec53ULL; x^=x>>33; return x; }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src){ return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32); }
__device__ __forceinline__ uint64_t swap64(uint64_t* p, uint64_t v){ return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// V = 0: A, 1: B, 2: B-split. One wave per workgroup, one lane per delta (the probe kernel's shape); n is a multiple of 64.
template <int V>
__global__ __launch_bounds__(64) void k_claim(uint64_t* tab, uint64_t nslots, uint32_t n, uint64_t seed, uint32_t epoch, uint32_t* out) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x, lane = threadIdx.x;
  const uint64_t s = __umul64hi(mix64(j + seed), nslots);
  const uint4* q = reinterpret_cast<const uint4*>(tab + 4 * s);
  const uint4 lo = q[0], hi = q[1];
  uint32_t x = lo.x ^ lo.y ^ lo.z ^ lo.w ^ hi.x ^ hi.y ^ hi.z ^ hi.w;
  const bool win = (mix64(j * 7 + seed) % 100) < 84;
  const uint32_t tag = (epoch << 24) | j;
  const uint64_t w1 = (uint64_t)lo.z | ((uint64_t)tag << 32), w2 = (uint64_t)j | ((uint64_t)(uint32_t)seed << 32), w3 = (uint64_t)x | (7ull << 32);
  if (V == 0) {
    if (win) {
      x ^= atomicExch(reinterpret_cast<uint32_t*>(tab + 4 * s) + 3, tag);
      reinterpret_cast<uint4*>(tab + 4 * s)[1] = make_uint4((uint32_t)w2, (uint32_t)(w2 >> 32), x, 7u);
    }
  } else if (V == 1) {
    const uint32_t role = lane & 3u;
    uint32_t prev = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int src = 16 * p + (int)(lane >> 2);
      const uint64_t ss = shfl64(s, src);
      const bool on = __shfl((int)win, src) != 0 && role < 3u;
      const uint64_t a1 = shfl64(w1, src), a2 = shfl64(w2, src), a3 = shfl64(w3, src);
      const uint64_t opnd = role == 0 ? a1 : (role == 1 ? a2 : a3);
      uint64_t old = 0;
      if (on) old = swap64(tab + 4 * ss + 1 + role, opnd);
      const uint32_t got = (uint32_t)__shfl((int)(uint32_t)(old >> 32), 4 * (int)(lane & 15u));
      if ((int)(lane >> 4) == p) prev = got;
    }
    if (win) x ^= prev;
  } else {
    if (win) {
      x ^= (uint32_t)(swap64(tab + 4 * s + 1, w1) >> 32);
      asm volatile("" ::: "memory");
      swap64(tab + 4 * s + 2, w2);
      asm volatile("" ::: "memory");
      swap64(tab + 4 * s + 3, w3);
    }
  }
  out[j] = x;
}

// Tear check. Workgroups alternate in groups of eight (so that every XCD runs writers and readers): writers swap (tag, x, ~x ^ K) into words 1..3 of
// random slots of a small hot table, one team of four lanes per slot; readers load words 2..3 with one 16-B load (plain, or nontemporal on every second reader group).
// SPLIT: the same lanes issue the three swaps as three instructions (the control). `fresh` counts loads that saw a written pair at all.
constexpr uint64_t TEAR_K = 0x5DEECE66DA5A5A5Aull;
template <bool SPLIT>
__global__ __launch_bounds__(256) void k_tear(uint64_t* tab, uint32_t nslots, uint32_t iters, unsigned long long* torn, unsigned long long* reads, unsigned long long* fresh) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
  const bool writer = ((blockIdx.x >> 3) & 1u) == 0;
  const uint32_t role = threadIdx.x & 3u;
  uint64_t x = (uint64_t)(writer ? gid >> 2 : gid) * 0x9E3779B97F4A7C15ull + 1;     // the four lanes of a team draw the same slots and values
  unsigned long long bad = 0, n = 0, fr = 0, sink = 0;     // the swaps return, as the product's do
  for (uint32_t i = 0; i < iters; i++) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t s = (uint32_t)(x >> 40) % nslots;
    uint64_t* p = tab + 4 * (size_t)s;
    if (writer) {
      const uint64_t opnd = role == 0 ? ((uint64_t)gid << 32) | 77u : (role == 1 ? x : ~x ^ TEAR_K);
      if (SPLIT) {
        if (role == 0) sink ^= swap64(p + 1, opnd);
        asm volatile("" ::: "memory");
        if (role == 1) sink ^= swap64(p + 2, opnd);
        asm volatile("" ::: "memory");
        if (role == 2) sink ^= swap64(p + 3, opnd);
      } else if (role < 3u) {
        sink ^= swap64(p + 1 + role, opnd);
      }
    } else {
      u32x4 v;
      if (blockIdx.x & 16u) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 2));
      else { v = *reinterpret_cast<const u32x4*>(p + 2); asm volatile("" ::: "memory"); }
      const uint64_t a = (uint64_t)v.x | ((uint64_t)v.y << 32), b = (uint64_t)v.z | ((uint64_t)v.w << 32);
      if (!(a == 0 && b == 0)) { fr++; if (b != (~a ^ TEAR_K)) bad++; }
      n++;
    }
  }
  if (bad) atomicAdd(torn, bad);
  if (n | (sink == 0x0123456789ABCDEFull)) atomicAdd(reads, n);
  if (fr) atomicAdd(fresh, fr);
}

__global__ void k_fill(uint4* t, size_t n16){ size_t i=(size_t)blockIdx.x*blockDim.x+threadIdx.x; size_t st=(size_t)gridDim.x*blockDim.x; for(;i<n16;i+=st){ uint32_t v=(uint32_t)i; t[i]=make_uint4(v,v*3,v*5,v*7);} }

static void launch(int v, uint64_t* tab, uint64_t nslots, uint32_t n, uint64_t seed, uint32_t epoch, uint32_t* out) {
  const dim3 g(n / 64), b(64);
  if (v == 0) hipLaunchKernelGGL((k_claim<0>), g, b, 0, 0, tab, nslots, n, seed, epoch, out);
  else if (v == 1) hipLaunchKernelGGL((k_claim<1>), g, b, 0, 0, tab, nslots, n, seed, epoch, out);
  else hipLaunchKernelGGL((k_claim<2>), g, b, 0, 0, tab, nslots, n, seed, epoch, out);
}
#define SEED(i) ((uint64_t)(i)*1315423911ull+17)

int main(int argc, char** argv) {
  const bool pmc = argc > 1 && !strcmp(argv[1], "--pmc");
  const uint32_t n = 1u << 20;
  uint32_t* out; CK(hipMalloc(&out, (size_t)n * 4));
  const char* names[3] = {"A read+xchg32+store16", "B team swap_x2", "B-split 3 swaps"};
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const uint64_t sizes_mb[2] = {640, 1408};
  int launch_no = 0;
  for (int si = pmc ? 1 : 0; si < 2; si++) {
    const size_t bytes = sizes_mb[si] << 20; const uint64_t nslots = bytes / 32;
    uint64_t* tab; CK(hipMalloc(&tab, bytes));
    hipLaunchKernelGGL(k_fill, dim3(2048), dim3(256), 0, 0, reinterpret_cast<uint4*>(tab), bytes / 16); CK(hipDeviceSynchronize());
    if (pmc) {
      for (int r = 0; r < 3; r++) for (int v = 0; v < 3; v++) { launch(v, tab, nslots, n, SEED(launch_no), (uint32_t)(launch_no & 255), out); launch_no++; CK(hipDeviceSynchronize()); }
      printf("pmc mode: 3 launches of each variant on the %llu MB table\n", (unsigned long long)sizes_mb[si]);
    } else {
      for (int v = 0; v < 3; v++) for (int w = 0; w < 3; w++) { launch(v, tab, nslots, n, SEED(launch_no), (uint32_t)(launch_no & 255), out); launch_no++; }   // warm-up
      CK(hipDeviceSynchronize());
      const int REPEATS = 7, R = 10;
      std::vector<float> t[3];
      for (int rep = 0; rep < REPEATS; rep++) for (int v = 0; v < 3; v++) {       // interleaved: A, B, B-split, A, B, ...
        CK(hipEventRecord(e0));
        for (int r = 0; r < R; r++) { launch(v, tab, nslots, n, SEED(launch_no), (uint32_t)(launch_no & 255), out); launch_no++; }
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1)); t[v].push_back(ms / R * 1000.f);
      }
      for (int v = 0; v < 3; v++) {
        printf("table %5llu MB | %-22s | us per 1M, %d repeats of %d launches:", (unsigned long long)sizes_mb[si], names[v], REPEATS, R);
        for (float x : t[v]) printf(" %.1f", x);
        printf(" | min %.1f max %.1f range %.1f\n", *std::min_element(t[v].begin(), t[v].end()), *std::max_element(t[v].begin(), t[v].end()),
               *std::max_element(t[v].begin(), t[v].end()) - *std::min_element(t[v].begin(), t[v].end()));
      }
      fflush(stdout);
    }
    CK(hipFree(tab));
  }
  if (!pmc) {
    const uint32_t NS = 4096, ITERS = 4096, BLOCKS = 512;
    uint64_t* tab; unsigned long long* d; CK(hipMalloc(&tab, (size_t)NS * 32)); CK(hipMalloc(&d, 6 * 8));
    unsigned long long h[6];
    CK(hipMemset(tab, 0, (size_t)NS * 32)); CK(hipMemset(d, 0, 6 * 8));
    hipLaunchKernelGGL((k_tear<false>), dim3(BLOCKS), dim3(256), 0, 0, tab, NS, ITERS, d, d + 1, d + 2); CK(hipDeviceSynchronize());
    CK(hipMemset(tab, 0, (size_t)NS * 32));
    hipLaunchKernelGGL((k_tear<true>), dim3(BLOCKS), dim3(256), 0, 0, tab, NS, ITERS / 4, d + 3, d + 4, d + 5); CK(hipDeviceSynchronize());
    CK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
    printf("tear check | team swap: %llu loads, %llu saw a written pair, %llu torn | control (three instructions): %llu loads, %llu saw a written pair, %llu torn\n",
           h[1], h[2], h[0], h[4], h[5], h[3]);
  }
  return 0;
}
