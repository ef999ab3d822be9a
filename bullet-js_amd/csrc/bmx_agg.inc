// bmx_agg.inc — aggregate queries (bmx.h "aggregate queries"): bmx_scan_aggregate over one context. The kernels are agg_kernels.h; included by bmx.hip (one
// translation unit), which keeps their scratch (AggScratch): the groups' accumulators, left empty by every query's last kernel, and the records of a
// host-mode answer on their way down.
namespace {

// what every caller's arguments must satisfy before anything touches a device (bmx_comm_scan_aggregate asks the same)
const char* agg_bad_args(uint32_t nterms, const bmx_term* terms, uint32_t group_field, uint32_t ngroups, const bmx_agg* out) {
  if (const char* bad = bad_terms(nterms, terms, "aggregate needs 1..8 terms")) return bad;
  if (!out) return "bmx_scan_aggregate: null output";
  if (ngroups > BMX_AGG_MAX_GROUPS) return "bmx_scan_aggregate: more than BMX_AGG_MAX_GROUPS groups";
  if (ngroups && group_field == BMX_AGG_NO_FIELD) return "bmx_scan_aggregate: groups without a group field";
  return nullptr;
}
inline uint32_t agg_records(uint32_t ngroups) { return ngroups ? ngroups + 1 : 1; }

// where the kernels find a field's value: the index column (0), the probe of term k (k), a probe of its own, or nowhere
uint32_t agg_source(uint32_t field, uint32_t nterms, const bmx_term* terms) {
  if (field == BMX_AGG_NO_FIELD) return AGG_SRC_NONE;
  for (uint32_t k = 0; k < nterms; k++) if (terms[k].field == field) return k;
  return AGG_SRC_PROBE;
}

int agg_scratch(bmx_ctx* ctx, uint32_t nrec) {
  AggScratch& s = ctx->agg;
  if (nrec > s.cap) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.cap = 0;
    const uint32_t cap = nrec <= AGG_LDS_GROUPS + 1 ? AGG_LDS_GROUPS + 1 : BMX_AGG_MAX_GROUPS + 1;
    if (int rc = dev_alloc_all(ctx, {{s.raw, cap * sizeof(AggRaw)}, {s.stage, cap * sizeof(bmx_agg)}})) return rc;
    s.cap = cap; s.clean = false;
  }
  if (!s.clean) {     // new accumulators, or a query that did not get as far as its last kernel
    hipLaunchKernelGGL(k_agg_clear, dim3((s.cap + 255) / 256), dim3(256), 0, ctx->stream, s.raw, s.cap);
    LAUNCHCHK("k_agg_clear");
  }
  return BMX_OK;
}

template <class T, int G>
void agg_launch_sweep(bmx_ctx* ctx, const Index* ix, T lo, T hi, bool probe, const AggArgs& A) {
  const T* col = sizeof(T) == 4 ? reinterpret_cast<const T*>(ix->v32) : reinterpret_cast<const T*>(ix->v64);
  const uint32_t nt = ix->n * sizeof(T) > SCAN_NT_BYTES ? 1u : 0u;
  // no workgroup with fewer than four rounds of loads to spread its one flush over
  const uint32_t blocks = sweep_grid(ctx, ix->n, 4ull * AGG_THREADS * AGG_U * (16 / sizeof(T)));
  if (probe) hipLaunchKernelGGL((k_agg_sweep<T, true, G>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, col, (const uint64_t*)ix->ids, ix->n, lo, hi, nt, A);
  else hipLaunchKernelGGL((k_agg_sweep<T, false, G>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, col, (const uint64_t*)ix->ids, ix->n, lo, hi, nt, A);
}

template <class T, int G>
void agg_launch_view(bmx_ctx* ctx, const OrderedView& v, T lo, T hi, bool need_id, const AggArgs& A) {
  unsigned long long* ab = ctx->ds->ord_ab;
  const T* sv = static_cast<const T*>(v.s_val);
  const bool pending = v.npd + v.npi > 0;           // the logical view = main - pd + pi (bmx_view.inc)
  const int q = v.pcur, qi = v.icur;
  const T* dv = static_cast<const T*>(v.pd_v[q]); const T* iv = static_cast<const T*>(v.pi_v[qi]);
  if (pending) hipLaunchKernelGGL((k_ordered_bounds_p<T>), dim3(1), dim3(384), 0, ctx->stream, sv, v.ord_n, dv, v.npd, iv, v.npi, lo, hi, ab, (unsigned long long*)nullptr, 1u);
  else hipLaunchKernelGGL((k_ordered_bounds<T>), dim3(1), dim3(128), 0, ctx->stream, sv, v.ord_n, lo, hi, ab, (unsigned long long*)nullptr, 1u);
  // the run's length is the device's: a grid for the whole view, whose workgroups beyond the run leave at once
  const uint32_t blocks = sweep_grid(ctx, v.ord_n + v.npi, 4ull * AGG_THREADS);
  hipLaunchKernelGGL((k_agg_view<T, G>), dim3(blocks), dim3(AGG_THREADS), 0, ctx->stream, sv, (const uint32_t*)v.s_pos, (const uint64_t*)v.s_ids, dv, (const uint32_t*)v.pd_p[q], iv,
                     (const uint64_t*)v.pi_ids[qi], (const unsigned long long*)ab, pending ? 1u : 0u, need_id ? 1u : 0u, A);
}

template <class T>
void agg_launch(bmx_ctx* ctx, const Index* ix, bool ordered, int64_t lo, int64_t hi, bool probe, const AggArgs& A) {
  const int G = A.ngroups == 0 ? 0 : (A.ngroups <= AGG_LDS_GROUPS ? 1 : 2);
  const T l = (T)lo, h = (T)hi;
  if (ordered) {
    if (G == 0) agg_launch_view<T, 0>(ctx, ix->view, l, h, probe, A); else if (G == 1) agg_launch_view<T, 1>(ctx, ix->view, l, h, probe, A); else agg_launch_view<T, 2>(ctx, ix->view, l, h, probe, A);
  } else {
    if (G == 0) agg_launch_sweep<T, 0>(ctx, ix, l, h, probe, A); else if (G == 1) agg_launch_sweep<T, 1>(ctx, ix, l, h, probe, A); else agg_launch_sweep<T, 2>(ctx, ix, l, h, probe, A);
  }
}

// Enqueue one aggregate query; its records go to d_out (device memory), or, with d_out == nullptr, to the context's staging buffer (agg_collect fetches them).
// The arguments have been checked (agg_bad_args) and the context entered.
int agg_enqueue(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint32_t measure_field, uint32_t group_field, int64_t group_lo, uint32_t ngroups, bmx_agg* d_out) {
  Index* ix;
  if (int rc = fresh_index(ctx, terms[0].field, &ix)) return rc;
  const uint32_t nrec = agg_records(ngroups);
  if (int rc = agg_scratch(ctx, nrec)) return rc;
  AggArgs A{};
  A.slots = ctx->slots; A.nslots = ctx->nslots; A.acc = ctx->agg.raw;
  A.group_lo = group_lo; A.ngroups = ngroups; A.measure = measure_field; A.group = group_field;
  A.m_src = agg_source(measure_field, nterms, terms); A.g_src = ngroups ? agg_source(group_field, nterms, terms) : AGG_SRC_NONE;
  A.nterms = nterms;
  copy_terms(A.t, terms, nterms);
  const bool probe = nterms > 1 || A.m_src == AGG_SRC_PROBE || A.g_src == AGG_SRC_PROBE;
  const bool ordered = ensure_ordered_view(ctx, ix);
  const bool fits32 = ordered ? ix->view.ord_fits32 : ix->fits32;
  ctx->agg.clean = false;
  if (fits32) {   // the 4-byte column
    const Range32 r = clamp_i32(A.t[0].lo, A.t[0].hi);
    agg_launch<int32_t>(ctx, ix, ordered, r.lo, r.hi, probe, A);
  } else agg_launch<int64_t>(ctx, ix, ordered, A.t[0].lo, A.t[0].hi, probe, A);
  LAUNCHCHK("k_agg_sweep / k_agg_view");
  hipLaunchKernelGGL(k_agg_finish, dim3(std::min<uint32_t>((nrec + 255) / 256, 64)), dim3(256), 0, ctx->stream, ctx->agg.raw, d_out ? d_out : ctx->agg.stage, nrec,
                     A.m_src != AGG_SRC_PROBE ? 1u : 0u);
  LAUNCHCHK("k_agg_finish");
  ctx->agg.clean = true;
  if (ordered) view_after_query(ctx, ix);
  return BMX_OK;
}

// second half of a host-mode query: wait for it and copy its records down
int agg_collect(bmx_ctx* ctx, uint32_t nrec, bmx_agg* out) {
  HIPCHK(hipMemcpyAsync(out, ctx->agg.stage, (size_t)nrec * sizeof(bmx_agg), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_scan_aggregate(bmx_ctx* ctx, uint32_t nterms, const bmx_term* terms, uint32_t measure_field, uint32_t group_field, int64_t group_lo, uint32_t ngroups,
                       bmx_agg* out, int mem) {
  if (const char* bad = agg_bad_args(nterms, terms, group_field, ngroups, out)) return fail(ctx, BMX_ERR_INVALID, bad);
  if (mem != BMX_MEM_HOST && mem != BMX_MEM_DEVICE) return fail(ctx, BMX_ERR_INVALID, "bad mem kind");
  if (!ctx) return fail(nullptr, BMX_ERR_INVALID, "null context");
  if (int erc = enter(ctx)) return erc;
  if (int rc = agg_enqueue(ctx, nterms, terms, measure_field, group_field, group_lo, ngroups, mem == BMX_MEM_DEVICE ? out : nullptr)) return rc;
  return mem == BMX_MEM_HOST ? agg_collect(ctx, agg_records(ngroups), out) : BMX_OK;
}

}  // extern "C"
