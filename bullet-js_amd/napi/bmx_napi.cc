// bmx_napi.cc — thin N-API shim over the C ABI (include/bmx.h). No logic lives here: it converts typed
// arrays to pointers, calls libbmx.so and throws a JS Error carrying bmx_last_error() on failure
// (reference error policy: the hot path reports, never aborts — src/bullet.js:230-234).
// Built by bullet-js_amd/Makefile into bullet-js_amd/bmx.node and loaded by js/native.js.
//
// A new binding is put together from these, each of which exists once:
//   HANDLE(Kind, N)            arguments + the live handle of that kind (Engine, Vc, Comm), or the kind's "invalid or closed" error
//   get_u32 / get_count / get_i64 / get_ta / get_keys / get_cols / get_terms / is_nullish      argument parsing; all of it BEFORE the turn is taken
//   Turn turn(h->q)            the call runs in issue order with everything else on the handle (bmx_ticket.h)
//   fail<Kind>(env, h->p, rc)  the "bmx error <rc>: <text>" Error with .code
//   make_ta / copy_ta / num / cols_result / merge_result / scan_result      results; a null from them means a JS error is pending: return it
//   Job<Kind> + queue_job      work on a libuv worker behind a promise
// A call that exists for the engine and for the communicator is ONE template over the kind; Init names both instances.
#include <node_api.h>
#include <cmath>
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "bmx.h"
#include "bmx_top.h"
#include "bmx_where.h"
#include "bmx_where_agg.h"
#include "bmx_rows.h"
#include "bmx_ticket.h"

namespace {

#define NAPI_OK(call)                                           \
  do {                                                          \
    if ((call) != napi_ok) {                                    \
      napi_throw_error(env, nullptr, "N-API call failed: " #call); \
      return nullptr;                                           \
    }                                                           \
  } while (0)

// ---- handle kinds: what differs between the engine, the vector-clock table and the communicator ------------------------------------
// host(fn, args...) calls an entry point on host buffers: the engine's take a trailing `mem`, the communicator's are host-only.
struct Engine {
  using T = bmx_ctx;
  static constexpr uint32_t tag = 0x626d7801u;
  static constexpr const char* closed = "bmx: invalid or closed engine handle";
  static constexpr const char* gone = "engine closed";
  static constexpr auto destroy = bmx_destroy;
  static constexpr auto last_error = bmx_last_error;
  static constexpr auto load_rows = bmx_load_rows;
  static constexpr auto put_rows = bmx_put_rows;
  static constexpr auto get_rows = bmx_get_rows;
  static constexpr auto row_count = bmx_row_count;
  static constexpr auto dump_rows = bmx_dump_rows;
  static constexpr auto index_build = bmx_index_build;
  static constexpr auto index_set_ordered = bmx_index_set_ordered;
  static constexpr auto scan_range = bmx_scan_range;
  static constexpr auto scan_count = bmx_scan_count;
  static constexpr auto digest = bmx_digest;
  static constexpr auto export_rows = bmx_export_rows;
  static constexpr auto scan_aggregate = bmx_scan_aggregate;
  static constexpr auto scan_top = bmx_scan_top;
  static constexpr auto where_aggregate = bmx_where_aggregate;
  static constexpr auto where_top = bmx_where_top;
  template <class F, class... A> static int host(F fn, A... a) { return fn(a..., BMX_MEM_HOST); }
};
struct Comm {
  using T = bmx_comm;
  static constexpr uint32_t tag = 0x626d7802u;
  static constexpr const char* closed = "bmx: invalid or closed communicator handle";
  static constexpr auto destroy = bmx_comm_destroy;
  static constexpr auto last_error = bmx_comm_last_error;
  static constexpr auto load_rows = bmx_comm_load_rows;
  static constexpr auto put_rows = bmx_comm_put_rows;
  static constexpr auto get_rows = bmx_comm_get_rows;
  static constexpr auto row_count = bmx_comm_row_count;
  static constexpr auto dump_rows = bmx_comm_dump_rows;
  static constexpr auto index_build = bmx_comm_index_build;
  static constexpr auto index_set_ordered = bmx_comm_index_set_ordered;
  static constexpr auto scan_range = bmx_comm_scan_range;
  static constexpr auto scan_count = bmx_comm_scan_count;
  static constexpr auto digest = bmx_comm_digest;
  static constexpr auto export_rows = bmx_comm_export_rows;
  static constexpr auto scan_aggregate = bmx_comm_scan_aggregate;
  static constexpr auto scan_top = bmx_comm_scan_top;
  static constexpr auto where_aggregate = bmx_comm_where_aggregate;
  static constexpr auto where_top = bmx_comm_where_top;
  template <class F, class... A> static int host(F fn, A... a) { return fn(a...); }
};
struct Vc {
  using T = bmx_vc;
  static constexpr uint32_t tag = 0x626d7803u;
  static constexpr const char* closed = "bmx: invalid or closed vector-clock table handle";
  static constexpr const char* gone = "table closed";
  static constexpr auto destroy = bmx_vc_destroy;
  static constexpr auto last_error = bmx_vc_last_error;
};

// What a JS external of this addon points to. The tag comes first and is checked before anything else is read: an external of another kind is
// refused, never cast (Node 12 has no napi_type_tag_object). p == nullptr: closed. K: the vector-clock table's writers, 0 otherwise.
template <class Kind> struct Handle {
  const uint32_t tag = Kind::tag;
  typename Kind::T* p = nullptr;
  uint32_t K = 0;
  Tickets q;
};

template <class Kind> Handle<Kind>* peek_handle(napi_env env, napi_value v) {   // open or closed; null for anything else
  void* p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || *static_cast<const uint32_t*>(p) != Kind::tag) return nullptr;
  return static_cast<Handle<Kind>*>(p);
}
template <class Kind> Handle<Kind>* get_handle(napi_env env, napi_value v) {
  Handle<Kind>* h = peek_handle<Kind>(env, v);
  if (h && h->p) return h;
  napi_throw_error(env, nullptr, Kind::closed);
  return nullptr;
}
template <class Kind> void finalize(napi_env, void* data, void*) {
  Handle<Kind>* h = static_cast<Handle<Kind>*>(data);
  if (h->p) Kind::destroy(h->p);
  delete h;
}
template <class Kind> napi_value wrap(napi_env env, typename Kind::T* p, uint32_t K = 0) {
  Handle<Kind>* h = new Handle<Kind>();
  h->p = p; h->K = K;
  napi_value ext;
  if (napi_create_external(env, h, finalize<Kind>, nullptr, &ext) != napi_ok) { finalize<Kind>(env, h, nullptr); napi_throw_error(env, nullptr, "bmx: external refused"); return nullptr; }
  return ext;
}

// ---- errors ---------------------------------------------------------------------------------------------------------------------------
napi_value bmx_error(napi_env env, int rc, const char* text) {
  std::string msg = "bmx error " + std::to_string(rc) + ": " + text;
  napi_value code, err, m;
  napi_create_string_utf8(env, msg.c_str(), NAPI_AUTO_LENGTH, &m);
  napi_create_error(env, nullptr, m, &err);
  napi_create_int32(env, rc, &code);
  napi_set_named_property(env, err, "code", code);
  return err;
}
napi_value throw_bmx(napi_env env, int rc, const char* text) { napi_throw(env, bmx_error(env, rc, text)); return nullptr; }
template <class Kind> napi_value fail(napi_env env, const typename Kind::T* p, int rc) { return throw_bmx(env, rc, Kind::last_error(p)); }

// ---- arguments ------------------------------------------------------------------------------------------------------------------------
#define ARGS_OPT(MIN, MAX)                                   \
  size_t argc = MAX; napi_value argv[MAX];                   \
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr)); \
  if (argc < MIN) { napi_throw_type_error(env, nullptr, "bmx: missing arguments"); return nullptr; }
#define ARGS(N) ARGS_OPT(N, N)
#define HANDLE(Kind, N) ARGS(N); Handle<Kind>* h = get_handle<Kind>(env, argv[0]); if (!h) return nullptr;

bool is_nullish(napi_env env, napi_value v) { napi_valuetype t; napi_typeof(env, v, &t); return t == napi_undefined || t == napi_null; }
bool get_u32(napi_env env, napi_value v, uint32_t* out) {
  if (napi_get_value_uint32(env, v, out) == napi_ok) return true;
  napi_throw_error(env, nullptr, "N-API call failed: napi_get_value_uint32");
  return false;
}
bool get_count(napi_env env, napi_value v, double* out) {   // a row count or position: a double on the way in, checked or cast by the caller
  if (napi_get_value_double(env, v, out) == napi_ok) return true;
  napi_throw_error(env, nullptr, "N-API call failed: napi_get_value_double");
  return false;
}
// number | bigint -> int64 (saturating; +-Infinity allowed, as range() accepts them: src/bullet-query.js:248-253)
bool get_i64(napi_env env, napi_value v, int64_t* out) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  if (t == napi_bigint) {
    bool lossless;
    return napi_get_value_bigint_int64(env, v, out, &lossless) == napi_ok;
  }
  double d;
  if (napi_get_value_double(env, v, &d) != napi_ok || isnan(d)) { napi_throw_type_error(env, nullptr, "bmx: expected a number or bigint"); return false; }
  if (d >= 9.2e18) *out = INT64_MAX; else if (d <= -9.2e18) *out = INT64_MIN; else *out = (int64_t)d;
  return true;
}
// typed array -> (pointer, element count); checks the element type
template <class E> bool get_ta(napi_env env, napi_value v, napi_typedarray_type want, const E** data, size_t* len) {
  napi_typedarray_type t; napi_value ab; size_t off; void* p;
  if (napi_get_typedarray_info(env, v, &t, len, &p, &ab, &off) != napi_ok || t != want) {
    napi_throw_type_error(env, nullptr, "bmx: wrong typed-array type (id BigUint64Array, field Uint32Array, ts/val BigInt64Array)");
    return false;
  }
  *data = static_cast<const E*>(p);
  return true;
}
struct Cols { const uint64_t* id; const uint32_t* field; const int64_t *ts, *val; size_t n; };
bool get_keys(napi_env env, napi_value* a, Cols* c) {   // (id, field) of one length
  size_t n1;
  if (!get_ta(env, a[0], napi_biguint64_array, &c->id, &c->n) || !get_ta(env, a[1], napi_uint32_array, &c->field, &n1)) return false;
  if (c->n != n1) { napi_throw_range_error(env, nullptr, "bmx: column lengths differ"); return false; }
  return true;
}
bool get_cols(napi_env env, napi_value* a, Cols* c) {   // (id, field, ts, val) of one length
  size_t n1, n2, n3;
  if (!get_ta(env, a[0], napi_biguint64_array, &c->id, &c->n) || !get_ta(env, a[1], napi_uint32_array, &c->field, &n1) ||
      !get_ta(env, a[2], napi_bigint64_array, &c->ts, &n2) || !get_ta(env, a[3], napi_bigint64_array, &c->val, &n3)) return false;
  if (c->n != n1 || c->n != n2 || c->n != n3) { napi_throw_range_error(env, nullptr, "bmx: column lengths differ"); return false; }
  return true;
}
// [[field, lo, hi], ...] -> terms[8]; returns the count, 0 with a JS error pending. `what` words the message: filter, aggregate, top
uint32_t get_terms(napi_env env, napi_value list, const char* what, bmx_term* terms) {
  uint32_t nt = 0;
  if (napi_get_array_length(env, list, &nt) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_array_length"); return 0; }
  if (nt == 0 || nt > 8) { napi_throw_range_error(env, nullptr, (std::string("bmx: ") + what + " needs 1..8 terms").c_str()); return 0; }
  for (uint32_t k = 0; k < nt; k++) {
    napi_value t, e0, e1, e2;
    if (napi_get_element(env, list, k, &t) != napi_ok || napi_get_element(env, t, 0, &e0) != napi_ok || napi_get_element(env, t, 1, &e1) != napi_ok ||
        napi_get_element(env, t, 2, &e2) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_element"); return 0; }
    terms[k].reserved = 0;
    if (!get_u32(env, e0, &terms[k].field) || !get_i64(env, e1, &terms[k].lo) || !get_i64(env, e2, &terms[k].hi)) return 0;
  }
  return nt;
}

// ---- results: a null return means a JS error is pending --------------------------------------------------------------------------------
size_t ta_elem(napi_typedarray_type t) { return t == napi_uint8_array ? 1 : t == napi_uint32_array ? 4 : 8; }   // the three widths this addon hands out
napi_value make_ta(napi_env env, napi_typedarray_type t, size_t n, void** data) {
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, n * ta_elem(t), data, &ab) == napi_ok && napi_create_typedarray(env, t, n, ab, 0, &ta) == napi_ok) return ta;
  napi_throw_error(env, nullptr, "bmx: could not allocate a result array");
  return nullptr;
}
napi_value copy_ta(napi_env env, napi_typedarray_type t, size_t n, const void* src) {
  void* p; napi_value ta = make_ta(env, t, n, &p);
  if (ta && n) memcpy(p, src, n * ta_elem(t));
  return ta;
}
napi_value num(napi_env env, double v) { napi_value n; napi_create_double(env, v, &n); return n; }
void set_num(napi_env env, napi_value obj, const char* k, double v) { napi_set_named_property(env, obj, k, num(env, v)); }
// {k0: v0, k1: v1, ...} in this order; null if a value is
struct Member { const char* key; napi_value v; };
napi_value object_of(napi_env env, std::initializer_list<Member> members) {
  napi_value out;
  for (const Member& m : members) if (!m.v) return nullptr;
  NAPI_OK(napi_create_object(env, &out));
  for (const Member& m : members) napi_set_named_property(env, out, m.key, m.v);
  return out;
}
napi_value cols_object(napi_env env, napi_value id, napi_value field, napi_value ts, napi_value val) { return object_of(env, {{"id", id}, {"field", field}, {"ts", ts}, {"val", val}}); }
napi_value cols_result(napi_env env, size_t m, const uint64_t* id, const uint32_t* field, const int64_t* ts, const int64_t* val) {
  return cols_object(env, copy_ta(env, napi_biguint64_array, m, id), copy_ta(env, napi_uint32_array, m, field), copy_ta(env, napi_bigint64_array, m, ts), copy_ta(env, napi_bigint64_array, m, val));
}
napi_value cols_result(napi_env env, size_t m, const bmx_delta_rec* recs) {
  void *pi = nullptr, *pf = nullptr, *pt = nullptr, *pv = nullptr;
  napi_value out = cols_object(env, make_ta(env, napi_biguint64_array, m, &pi), make_ta(env, napi_uint32_array, m, &pf), make_ta(env, napi_bigint64_array, m, &pt), make_ta(env, napi_bigint64_array, m, &pv));
  if (out) for (size_t i = 0; i < m; i++) { ((uint64_t*)pi)[i] = recs[i].id; ((uint32_t*)pf)[i] = recs[i].field; ((int64_t*)pt)[i] = recs[i].ts; ((int64_t*)pv)[i] = recs[i].val; }
  return out;
}
// {applied, [flags,] nApplied, nConflicts, nRows}; flags == nullptr: the communicator's, which collects none
napi_value merge_result(napi_env env, const uint32_t* applied, uint64_t na, const napi_value* flags, const bmx_merge_stats& st) {
  napi_value ta = copy_ta(env, napi_uint32_array, (size_t)na, applied);
  napi_value out = flags ? object_of(env, {{"applied", ta}, {"flags", *flags}}) : object_of(env, {{"applied", ta}});
  if (out) { set_num(env, out, "nApplied", (double)st.n_applied); set_num(env, out, "nConflicts", (double)st.n_conflicts); set_num(env, out, "nRows", (double)st.n_rows); }
  return out;
}
// count-then-fill: count(&m) sizes the array, fill(out, m) writes it; both return a bmx status. Takes the turn.
template <class Kind, class Count, class Fill>
napi_value scan_result(napi_env env, Handle<Kind>* h, napi_typedarray_type t, Count count, Fill fill) {
  Turn turn(h->q);
  uint64_t m = 0; int rc = count(&m);
  if (rc) return fail<Kind>(env, h->p, rc);
  void* out; napi_value ta = make_ta(env, t, m, &out);
  if (ta && m && (rc = fill(out, m))) return fail<Kind>(env, h->p, rc);
  return ta;
}

// ---- asynchronous work: the job runs on a libuv worker thread in its turn; the promise resolves to the job's result() -------------------
template <class Kind> struct Job {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  std::vector<napi_ref> refs;            // the handle and the input arrays: they outlive the job (and must not be mutated meanwhile)
  Handle<Kind>* h = nullptr;
  uint64_t ticket = 0;
  int rc = 0; std::string err;
  virtual ~Job() {}
  virtual int run() = 0;                 // worker thread, inside the turn, handle open: the bmx status
  virtual napi_value result(napi_env env) = 0;   // JS thread, after run() returned BMX_OK
};
template <class Kind> void job_execute(napi_env, void* data) {
  Job<Kind>* j = static_cast<Job<Kind>*>(data);
  Turn turn(j->h->q, j->ticket);         // in the order JS issued it, whatever worker picks it up
  if (!j->h->p) { j->rc = BMX_ERR_INVALID; j->err = Kind::gone; return; }
  if ((j->rc = j->run())) j->err = Kind::last_error(j->h->p);
}
template <class Kind> void job_drop(napi_env env, Job<Kind>* j) {
  for (napi_ref r : j->refs) napi_delete_reference(env, r);
  if (j->work) napi_delete_async_work(env, j->work);
  delete j;
}
template <class Kind> void job_complete(napi_env env, napi_status, void* data) {
  Job<Kind>* j = static_cast<Job<Kind>*>(data);
  napi_value out = j->rc ? nullptr : j->result(env);
  if (j->rc) napi_reject_deferred(env, j->deferred, bmx_error(env, j->rc, j->err.c_str()));
  else if (out) napi_resolve_deferred(env, j->deferred, out);
  else { napi_value thrown; napi_get_and_clear_last_exception(env, &thrown); napi_reject_deferred(env, j->deferred, thrown); }   // a result array was refused
  job_drop(env, j);
}
// Owns j from here on. keep[0..nkeep): the values to reference until completion. Call it when nothing else can fail.
template <class Kind> napi_value queue_job(napi_env env, Job<Kind>* j, const char* name, napi_value* keep, size_t nkeep) {
  napi_value promise, nm;
  auto drop = [&](const char* what) { job_drop(env, j); napi_throw_error(env, nullptr, what); return (napi_value) nullptr; };
  if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) return drop("bmx: could not create a promise");
  for (size_t k = 0; k < nkeep; k++) { napi_ref r; if (napi_create_reference(env, keep[k], 1, &r) == napi_ok) j->refs.push_back(r); }   // (an absent optional argument takes none)
  if (napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &nm) != napi_ok ||
      napi_create_async_work(env, nullptr, nm, job_execute<Kind>, job_complete<Kind>, j, &j->work) != napi_ok) return drop("bmx: could not create the async work item");
  // the ticket is taken last: a ticket that never runs would block every later operation on this handle
  j->ticket = j->h->q.take();
  if (napi_queue_async_work(env, j->work) != napi_ok) {
    { Turn skip(j->h->q, j->ticket); }   // give the turn back
    return drop("bmx: could not queue the async work item");
  }
  return promise;
}

// ---- no handle ------------------------------------------------------------------------------------------------------------------------
// ownersOf(id: BigUint64Array, nshards) -> Uint8Array: bmx_owner_of for every id (the host-side routing of small batches and of the K-writer table)
napi_value OwnersOf(napi_env env, napi_callback_info info) {
  ARGS(2);
  const uint64_t* id; size_t n;
  if (!get_ta(env, argv[0], napi_biguint64_array, &id, &n)) return nullptr;
  uint32_t ns; if (!get_u32(env, argv[1], &ns)) return nullptr;
  if (ns == 0 || ns > 255) { napi_throw_range_error(env, nullptr, "bmx: 1..255 shards"); return nullptr; }
  void* o; napi_value out = make_ta(env, napi_uint8_array, n, &o);
  if (out) for (size_t i = 0; i < n; i++) ((uint8_t*)o)[i] = (uint8_t)bmx_owner_of(id[i], ns);
  return out;
}

napi_value AbiVersion(napi_env env, napi_callback_info) { napi_value v; napi_create_int32(env, bmx_abi_version(), &v); return v; }

// hostColumns(n) -> {id: BigUint64Array, field: Uint32Array, ts: BigInt64Array, val: BigInt64Array} of n rows over ONE page-locked allocation
// (bmx_host_alloc): batches built in it upload at the link's rate, with no pinning of fresh pages by the runtime. Freed when the buffer is collected.
void finalize_host_buffer(napi_env, void* data, void*) { (void)bmx_host_free(data); }
napi_value HostColumns(napi_env env, napi_callback_info info) {
  ARGS(1);
  double dn;
  if (napi_get_value_double(env, argv[0], &dn) != napi_ok || !(dn >= 1) || dn > 16777216) { napi_throw_range_error(env, nullptr, "bmx: hostColumns(n) wants 1 <= n <= 2^24"); return nullptr; }
  const size_t n = (size_t)dn;
  void* mem = nullptr;
  int rc = bmx_host_alloc(28ull * n, &mem);
  if (rc) return fail<Engine>(env, nullptr, rc);
  napi_value ab, id, field, ts, val;
  if (napi_create_external_arraybuffer(env, mem, 28 * n, finalize_host_buffer, nullptr, &ab) != napi_ok) { (void)bmx_host_free(mem); napi_throw_error(env, nullptr, "bmx: external ArrayBuffer refused"); return nullptr; }
  NAPI_OK(napi_create_typedarray(env, napi_biguint64_array, n, ab, 0, &id));
  NAPI_OK(napi_create_typedarray(env, napi_bigint64_array, n, ab, 8 * n, &ts));
  NAPI_OK(napi_create_typedarray(env, napi_bigint64_array, n, ab, 16 * n, &val));
  NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, ab, 24 * n, &field));
  return cols_object(env, id, field, ts, val);
}

// ---- every kind -----------------------------------------------------------------------------------------------------------------------
template <class Kind> napi_value Destroy(napi_env env, napi_callback_info info) {
  ARGS(1);
  if (Handle<Kind>* h = peek_handle<Kind>(env, argv[0])) {
    Turn turn(h->q);                                // after every operation issued before the close
    if (h->p) { Kind::destroy(h->p); h->p = nullptr; }
  }
  return nullptr;
}

// ---- the engine and the communicator: one body per call -------------------------------------------------------------------------------
// loadRows / putRows(h, id, field, ts, val): putRows stores rows decided on the host as given; val == -2^63 (BMX_VAL_DELETED) leaves a tombstone
template <class Kind, bool put> napi_value StoreRows(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 5);
  Cols c; if (!get_cols(env, argv + 1, &c)) return nullptr;
  Turn turn(h->q);
  int rc = put ? Kind::host(Kind::put_rows, h->p, c.n, c.id, c.field, c.ts, c.val) : Kind::host(Kind::load_rows, h->p, c.n, c.id, c.field, c.ts, c.val);
  return rc ? fail<Kind>(env, h->p, rc) : nullptr;
}
// getRows(h, id, field) -> {ts, val, found}
template <class Kind> napi_value GetRows(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 3);
  Cols c; if (!get_keys(env, argv + 1, &c)) return nullptr;
  void *ts = nullptr, *val = nullptr, *found = nullptr;
  napi_value out = object_of(env, {{"ts", make_ta(env, napi_bigint64_array, c.n, &ts)}, {"val", make_ta(env, napi_bigint64_array, c.n, &val)}, {"found", make_ta(env, napi_uint8_array, c.n, &found)}});
  if (!out) return nullptr;
  Turn turn(h->q);
  int rc = Kind::host(Kind::get_rows, h->p, c.n, c.id, c.field, (int64_t*)ts, (int64_t*)val, (uint8_t*)found);
  return rc ? fail<Kind>(env, h->p, rc) : out;
}
template <class Kind> napi_value RowCount(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 1);
  Turn turn(h->q);
  uint64_t n = 0; int rc = Kind::row_count(h->p, &n);
  return rc ? fail<Kind>(env, h->p, rc) : num(env, (double)n);
}
template <class Kind> napi_value DumpRows(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 1);
  Turn turn(h->q);
  uint64_t n = 0; int rc = Kind::row_count(h->p, &n);
  if (rc) return fail<Kind>(env, h->p, rc);
  std::vector<uint64_t> id(n ? n : 1); std::vector<uint32_t> f(n ? n : 1); std::vector<int64_t> ts(n ? n : 1), val(n ? n : 1);
  uint64_t m = 0;
  rc = Kind::host(Kind::dump_rows, h->p, n, id.data(), f.data(), ts.data(), val.data(), &m);
  if (rc) return fail<Kind>(env, h->p, rc);
  if (m > n) m = n;                    // rows in use >= rows dumped: tombstones keep their slot and are not data
  return cols_result(env, m, id.data(), f.data(), ts.data(), val.data());
}
template <class Kind> napi_value IndexBuild(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 2);
  uint32_t f; if (!get_u32(env, argv[1], &f)) return nullptr;
  Turn turn(h->q);
  int rc = Kind::index_build(h->p, f);
  return rc ? fail<Kind>(env, h->p, rc) : nullptr;
}
/* indexSetOrdered(handle, field, afterQueries): value-ordered view of the index (bmx_index_set_ordered); 0 = off */
template <class Kind> napi_value IndexSetOrdered(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 3);
  uint32_t f, n; if (!get_u32(env, argv[1], &f) || !get_u32(env, argv[2], &n)) return nullptr;
  Turn turn(h->q);
  int rc = Kind::index_set_ordered(h->p, f, n);
  return rc ? fail<Kind>(env, h->p, rc) : nullptr;
}
// scanRange(h, field, lo, hi) -> BigUint64Array of node ids
template <class Kind> napi_value ScanRange(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 4);
  uint32_t f; int64_t lo, hi; if (!get_u32(env, argv[1], &f) || !get_i64(env, argv[2], &lo) || !get_i64(env, argv[3], &hi)) return nullptr;
  return scan_result(env, h, napi_biguint64_array, [&](uint64_t* m) { return Kind::host(Kind::scan_count, h->p, f, lo, hi, m); },
                     [&](void* out, uint64_t m) { uint64_t m2 = 0; return Kind::host(Kind::scan_range, h->p, f, lo, hi, (uint64_t*)out, m, &m2); });
}
template <class Kind> napi_value ScanCount(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 4);
  uint32_t f; int64_t lo, hi; if (!get_u32(env, argv[1], &f) || !get_i64(env, argv[2], &lo) || !get_i64(env, argv[3], &hi)) return nullptr;
  Turn turn(h->q);
  uint64_t m = 0; int rc = Kind::host(Kind::scan_count, h->p, f, lo, hi, &m);
  return rc ? fail<Kind>(env, h->p, rc) : num(env, (double)m);
}
/* Replica reconciliation (bmx.h): thin bindings, no logic.
 * digest(handle, log2Buckets, tombstones) / commDigest(comm, ...) -> {sums: BigUint64Array, counts: BigUint64Array}
 * exportRows(handle, since, log2Buckets, bucketBits: BigUint64Array | null, onlyTombstones) / commExportRows(comm, ...) -> {id, field, ts, val, n} */
template <class Kind> napi_value Digest(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 3);
  uint32_t L; if (!get_u32(env, argv[1], &L)) return nullptr;
  bool tomb = false; NAPI_OK(napi_get_value_bool(env, argv[2], &tomb));
  if (L > 16) { napi_throw_range_error(env, nullptr, "bmx: log2Buckets is 0..16"); return nullptr; }
  void *ps = nullptr, *pc = nullptr;
  napi_value out = object_of(env, {{"sums", make_ta(env, napi_biguint64_array, (size_t)1 << L, &ps)}, {"counts", make_ta(env, napi_biguint64_array, (size_t)1 << L, &pc)}});
  if (!out) return nullptr;
  Turn turn(h->q);
  const int rc = Kind::host(Kind::digest, h->p, L, tomb ? BMX_SYNC_TOMBSTONES : 0u, (uint64_t*)ps, (uint64_t*)pc);
  return rc ? fail<Kind>(env, h->p, rc) : out;
}
template <class Kind> napi_value ExportRows(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 5);
  int64_t since; if (!get_i64(env, argv[1], &since)) return nullptr;
  uint32_t L; if (!get_u32(env, argv[2], &L)) return nullptr;
  if (L > 16) { napi_throw_range_error(env, nullptr, "bmx: log2Buckets is 0..16"); return nullptr; }
  const uint64_t* bits = nullptr;
  if (!is_nullish(env, argv[3])) {
    size_t words;
    if (!get_ta(env, argv[3], napi_biguint64_array, &bits, &words)) return nullptr;
    if (words < std::max<size_t>(1, ((size_t)1 << L) / 64)) { napi_throw_range_error(env, nullptr, "bmx: bucketBits needs 2^log2Buckets bits"); return nullptr; }
  }
  bool only_tomb = false; NAPI_OK(napi_get_value_bool(env, argv[4], &only_tomb));
  const uint32_t fl = only_tomb ? BMX_EXPORT_ONLY_TOMBSTONES : 0u;
  Turn turn(h->q);
  uint64_t n = 0, m = 0;
  int rc = Kind::host(Kind::export_rows, h->p, since, L, bits, fl, (bmx_delta_rec*)nullptr, (uint64_t)0, &n);
  std::vector<bmx_delta_rec> recs(n ? n : 1);
  if (!rc && n) rc = Kind::host(Kind::export_rows, h->p, since, L, bits, fl, recs.data(), n, &m);
  if (rc) return fail<Kind>(env, h->p, rc);
  if (m > n) m = n;
  napi_value out = cols_result(env, m, recs.data());
  if (out) set_num(env, out, "n", (double)m);
  return out;
}
/* Aggregate queries (bmx.h bmx_scan_aggregate): thin bindings, no logic.
 * scanAggregate(handle, [[field, lo, hi], ...], measure | null, group | null, groupLo, nGroups) / commScanAggregate(comm, ...) ->
 * {nMatch, n: BigUint64Array, min, max: BigInt64Array, sumLo: BigUint64Array, sumHi: BigInt64Array}, one entry per record (nGroups + 1, or 1 without groups) */
// measure | null, group | null, groupLo, nGroups at argv[0..3] -> fld[2], glo, ng; false with a JS error pending
bool get_agg_tail(napi_env env, const napi_value* argv, uint32_t* fld, int64_t* glo, uint32_t* ng) {
  fld[0] = fld[1] = BMX_AGG_NO_FIELD;
  for (int k = 0; k < 2; k++) if (!is_nullish(env, argv[k]) && !get_u32(env, argv[k], &fld[k])) return false;
  if (!get_i64(env, argv[2], glo) || !get_u32(env, argv[3], ng)) return false;
  if (*ng > BMX_AGG_MAX_GROUPS || (*ng && fld[1] == BMX_AGG_NO_FIELD)) { napi_throw_range_error(env, nullptr, "bmx: nGroups is 0..65536 and needs a group field"); return false; }
  return true;
}
napi_value agg_result(napi_env env, const std::vector<bmx_agg>& recs) {
  const size_t nrec = recs.size();
  void *pm = nullptr, *pn = nullptr, *plo = nullptr, *phi = nullptr, *psl = nullptr, *psh = nullptr;
  napi_value out = object_of(env, {{"nMatch", make_ta(env, napi_biguint64_array, nrec, &pm)}, {"n", make_ta(env, napi_biguint64_array, nrec, &pn)}, {"min", make_ta(env, napi_bigint64_array, nrec, &plo)},
                                   {"max", make_ta(env, napi_bigint64_array, nrec, &phi)}, {"sumLo", make_ta(env, napi_biguint64_array, nrec, &psl)}, {"sumHi", make_ta(env, napi_bigint64_array, nrec, &psh)}});
  if (out) for (size_t i = 0; i < nrec; i++) {
    ((uint64_t*)pm)[i] = recs[i].n_match; ((uint64_t*)pn)[i] = recs[i].n; ((int64_t*)plo)[i] = recs[i].min; ((int64_t*)phi)[i] = recs[i].max;
    ((uint64_t*)psl)[i] = recs[i].sum_lo; ((int64_t*)psh)[i] = recs[i].sum_hi;
  }
  return out;
}
template <class Kind> napi_value ScanAggregate(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 6);
  bmx_term terms[8]; const uint32_t nt = get_terms(env, argv[1], "aggregate", terms); if (!nt) return nullptr;
  uint32_t fld[2]; int64_t glo; uint32_t ng;
  if (!get_agg_tail(env, argv + 2, fld, &glo, &ng)) return nullptr;
  std::vector<bmx_agg> recs(ng ? (size_t)ng + 1 : 1);
  int rc;
  { Turn turn(h->q); rc = Kind::host(Kind::scan_aggregate, h->p, nt, (const bmx_term*)terms, fld[0], fld[1], glo, ng, recs.data()); }
  return rc ? fail<Kind>(env, h->p, rc) : agg_result(env, recs);
}
/* Ordered top-k queries (bmx_top.h bmx_scan_top): thin bindings, no logic.
 * scanTop(handle, [[field, lo, hi], ...], desc, after | null, k) / commScanTop(comm, ...) -> {ids: BigUint64Array, vals: BigInt64Array, nEligible}: the first k
 * eligible nodes in (value, id) order; after = [id (BigInt), value] is the cursor. Ids are BigUint64Array entries, as scanFilter delivers them. */
// desc, after | null, k at argv[0..2] -> flags, the cursor, k; false with a JS error pending
struct TopTail { uint32_t flags = 0, k = 0; bmx_top_rec cur{0, 0}; bool have_cur = false; const bmx_top_rec* after() const { return have_cur ? &cur : nullptr; } };
bool get_top_tail(napi_env env, const napi_value* argv, TopTail* t) {
  bool desc = false; if (napi_get_value_bool(env, argv[0], &desc) != napi_ok) { napi_throw_type_error(env, nullptr, "bmx: desc is a boolean"); return false; }
  t->flags = desc ? BMX_TOP_DESC : 0u;
  t->have_cur = !is_nullish(env, argv[1]);
  if (t->have_cur) {
    napi_value e0, e1; bool lossless = false;
    if (napi_get_element(env, argv[1], 0, &e0) != napi_ok || napi_get_element(env, argv[1], 1, &e1) != napi_ok || napi_get_value_bigint_uint64(env, e0, &t->cur.id, &lossless) != napi_ok) {
      napi_throw_type_error(env, nullptr, "bmx: after is [id (BigInt), value]"); return false;
    }
    if (!get_i64(env, e1, &t->cur.val)) return false;
  }
  if (!get_u32(env, argv[2], &t->k)) return false;
  if (t->k == 0 || t->k > BMX_TOP_MAX_K) { napi_throw_range_error(env, nullptr, "bmx: k is 1..4096"); return false; }
  return true;
}
napi_value top_result(napi_env env, const std::vector<bmx_top_rec>& recs, uint64_t m, uint64_t ne) {
  void *pi = nullptr, *pv = nullptr;
  napi_value out = object_of(env, {{"ids", make_ta(env, napi_biguint64_array, m, &pi)}, {"vals", make_ta(env, napi_bigint64_array, m, &pv)}, {"nEligible", num(env, (double)ne)}});
  if (out) for (uint64_t i = 0; i < m; i++) { ((uint64_t*)pi)[i] = recs[i].id; ((int64_t*)pv)[i] = recs[i].val; }
  return out;
}
template <class Kind> napi_value ScanTop(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 5);
  bmx_term terms[8]; const uint32_t nt = get_terms(env, argv[1], "top", terms); if (!nt) return nullptr;
  TopTail t; if (!get_top_tail(env, argv + 2, &t)) return nullptr;
  std::vector<bmx_top_rec> recs(t.k);
  uint64_t m = 0, ne = 0; int rc;
  { Turn turn(h->q); rc = Kind::host(Kind::scan_top, h->p, nt, (const bmx_term*)terms, t.flags, t.after(), t.k, recs.data(), &m, &ne); }
  return rc ? fail<Kind>(env, h->p, rc) : top_result(env, recs, m, ne);
}
// The engine sweeps once: room for the whole index of `base`, as scanFilter sizes its answer (the sweep is bound by its probes: a count in front would double
// it). The communicator's shards have no common size: it counts first, then fetches — two sweeps.
napi_value where_answer(napi_env env, Handle<Engine>* h, uint32_t base, uint32_t nc, const uint32_t* lens, const std::vector<bmx_lit>& lits) {
  Turn turn(h->q);
  uint64_t cap = 0; int rc = bmx_index_size(h->p, base, &cap);
  if (rc) return fail<Engine>(env, h->p, rc);
  std::vector<uint64_t> tmp(cap ? cap : 1);
  uint64_t m = 0; rc = bmx_scan_where(h->p, base, nc, lens, lits.data(), tmp.data(), cap, &m, BMX_MEM_HOST);
  return rc ? fail<Engine>(env, h->p, rc) : copy_ta(env, napi_biguint64_array, (size_t)std::min(m, cap), tmp.data());
}
napi_value where_answer(napi_env env, Handle<Comm>* h, uint32_t base, uint32_t nc, const uint32_t* lens, const std::vector<bmx_lit>& lits) {
  return scan_result(env, h, napi_biguint64_array, [&](uint64_t* m) { return bmx_comm_scan_where(h->p, base, nc, lens, lits.data(), nullptr, 0, m); },
                     [&](void* out, uint64_t m) { uint64_t m2 = 0; return bmx_comm_scan_where(h->p, base, nc, lens, lits.data(), (uint64_t*)out, m, &m2); });
}
/* Boolean filters (bmx_where.h bmx_scan_where): thin bindings, no logic.
 * scanWhere(handle, base, [[[field, lo, hi, not], ...], ...]) / commScanWhere(comm, ...) -> BigUint64Array: the nodes holding data in field `base` for which some
 * clause has all of its literals true (not: a truthy fourth entry negates the literal), in index order of `base`. A fifth entry, [field, lo, hi, not, field2],
 * compares two fields of the node: lo <= field - field2 <= hi (bmx_where.h BMX_LIT_MINUS). A sixth entry, [field, lo, hi, not, null, states], makes the
 * literal range over the CLOCK of the field's row (bmx_where.h BMX_LIT_CLOCK, BMX_LIT_CLOCK_TOMB): states 1 = a row that holds data qualifies, 2 = a tombstoned
 * row, 3 = either. */
// [[[field, lo, hi, not(, field2)], ...], ...] -> the program as bmx_scan_where takes it; false with a JS error pending
struct Program { uint32_t nc = 0; uint32_t lens[BMX_WHERE_MAX_CLAUSES]; std::vector<bmx_lit> lits; };
bool get_program(napi_env env, napi_value clauses, Program* P) {
  if (napi_get_array_length(env, clauses, &P->nc) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_array_length"); return false; }
  if (P->nc == 0 || P->nc > BMX_WHERE_MAX_CLAUSES) { napi_throw_range_error(env, nullptr, "bmx: where needs 1..8 clauses"); return false; }
  for (uint32_t c = 0; c < P->nc; c++) {
    napi_value cl;
    uint32_t nl;
    if (napi_get_element(env, clauses, c, &cl) != napi_ok || napi_get_array_length(env, cl, &nl) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_array_length"); return false; }
    P->lens[c] = 0;      // in entries: a literal [f, lo, hi, not, f2] (lo <= f - f2 <= hi) takes two, the BMX_LIT_MINUS entry and its BMX_LIT_SUBTRAHEND entry
    for (uint32_t k = 0; k < nl && k < 8; k++) {
      napi_value t, e[6]; bmx_lit L{0, 0, 0, 0}; bool neg = false;
      bool ok = napi_get_element(env, cl, k, &t) == napi_ok;
      for (uint32_t j = 0; ok && j < 6; j++) ok = napi_get_element(env, t, j, &e[j]) == napi_ok;
      napi_valuetype second = napi_undefined, sixth = napi_undefined;
      if (!ok || napi_typeof(env, e[4], &second) != napi_ok || napi_typeof(env, e[5], &sixth) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_element"); return false; }
      if (!get_u32(env, e[0], &L.field) || !get_i64(env, e[1], &L.lo) || !get_i64(env, e[2], &L.hi)) return false;
      if (napi_coerce_to_bool(env, e[3], &e[3]) != napi_ok || napi_get_value_bool(env, e[3], &neg) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_coerce_to_bool"); return false; }
      const bool pair = second != napi_undefined && second != napi_null;
      uint32_t states = 0;      // the sixth entry: which row states a clock literal names
      if (sixth != napi_undefined && sixth != napi_null) {
        if (!get_u32(env, e[5], &states)) return false;
        if (states == 0 || states > 3) { napi_throw_range_error(env, nullptr, "bmx: a clock literal names states 1 (data), 2 (deleted) or 3 (either)"); return false; }
      }
      L.flags = (neg ? BMX_LIT_NOT : 0u) | (pair ? BMX_LIT_MINUS : 0u) | (states & 1u ? BMX_LIT_CLOCK : 0u) | (states & 2u ? BMX_LIT_CLOCK_TOMB : 0u);
      P->lits.push_back(L); P->lens[c]++;
      if (pair) {
        bmx_lit B{0, BMX_LIT_SUBTRAHEND, 0, 0};
        if (!get_u32(env, e[4], &B.field)) return false;
        P->lits.push_back(B); P->lens[c]++;
      }
    }
    if (nl == 0 || nl > 8 || P->lens[c] > 8 || P->lits.size() > BMX_WHERE_MAX_LITS) { napi_throw_range_error(env, nullptr, "bmx: a where clause has 1..8 literals, a program 32 at most"); return false; }
  }
  return true;
}
template <class Kind> napi_value ScanWhere(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 3);
  uint32_t base; if (!get_u32(env, argv[1], &base)) return nullptr;
  Program P; if (!get_program(env, argv[2], &P)) return nullptr;
  return where_answer(env, h, base, P.nc, P.lens, P.lits);
}
/* Aggregates and top-k over boolean filters (bmx_where_agg.h): thin bindings, no logic. The program is scanWhere's, the other arguments and the answers are
 * scanAggregate's and scanTop's.
 * whereAggregate(handle, base, clauses, measure | null, group | null, groupLo, nGroups) / commWhereAggregate(comm, ...)
 * whereTop(handle, base, clauses, desc, after | null, k) / commWhereTop(comm, ...): ordered by the value of `base`, then id */
template <class Kind> napi_value WhereAggregate(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 7);
  uint32_t base; if (!get_u32(env, argv[1], &base)) return nullptr;
  Program P; if (!get_program(env, argv[2], &P)) return nullptr;
  uint32_t fld[2]; int64_t glo; uint32_t ng;
  if (!get_agg_tail(env, argv + 3, fld, &glo, &ng)) return nullptr;
  std::vector<bmx_agg> recs(ng ? (size_t)ng + 1 : 1);
  int rc;
  { Turn turn(h->q); rc = Kind::host(Kind::where_aggregate, h->p, base, P.nc, (const uint32_t*)P.lens, (const bmx_lit*)P.lits.data(), fld[0], fld[1], glo, ng, recs.data()); }
  return rc ? fail<Kind>(env, h->p, rc) : agg_result(env, recs);
}
template <class Kind> napi_value WhereTop(napi_env env, napi_callback_info info) {
  HANDLE(Kind, 6);
  uint32_t base; if (!get_u32(env, argv[1], &base)) return nullptr;
  Program P; if (!get_program(env, argv[2], &P)) return nullptr;
  TopTail t; if (!get_top_tail(env, argv + 3, &t)) return nullptr;
  std::vector<bmx_top_rec> recs(t.k);
  uint64_t m = 0, ne = 0; int rc;
  { Turn turn(h->q); rc = Kind::host(Kind::where_top, h->p, base, P.nc, (const uint32_t*)P.lens, (const bmx_lit*)P.lits.data(), t.flags, t.after(), t.k, recs.data(), &m, &ne); }
  return rc ? fail<Kind>(env, h->p, rc) : top_result(env, recs, m, ne);
}
/* Row projection (bmx_rows.h bmx_where_rows): thin bindings, no logic. The program is scanWhere's.
 * whereRows(handle, base, clauses, [field, ...], ts, start, cap) / commWhereRows(comm, base, clauses, [field, ...], ts, startShard, startPos, cap) ->
 * {ids: BigUint64Array, vals: [BigInt64Array per field], ts: [BigInt64Array per field] (with a truthy ts), nMatch, nextPos, nextShard, layout}: the first cap
 * selected nodes from the cursor on, in index order of `base`; a cell without data holds BMX_VAL_DELETED, the clock of an absent cell BMX_ROWS_NO_CLOCK. */
struct RowsTail { uint32_t nf = 0, fields[BMX_ROWS_MAX_FIELDS] = {}, flags = 0; };
bool get_rows_tail(napi_env env, const napi_value* argv, RowsTail* t) {        // [field, ...], ts at argv[0..1]; false with a JS error pending
  if (napi_get_array_length(env, argv[0], &t->nf) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_array_length"); return false; }
  if (t->nf > BMX_ROWS_MAX_FIELDS) { napi_throw_range_error(env, nullptr, "bmx: whereRows takes 0..8 fields"); return false; }
  for (uint32_t k = 0; k < t->nf; k++) {
    napi_value e;
    if (napi_get_element(env, argv[0], k, &e) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_get_element"); return false; }
    if (!get_u32(env, e, &t->fields[k])) return false;
  }
  napi_value b; bool ts = false;
  if (napi_coerce_to_bool(env, argv[1], &b) != napi_ok || napi_get_value_bool(env, b, &ts) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: napi_coerce_to_bool"); return false; }
  t->flags = ts ? BMX_ROWS_TS : 0u;
  return true;
}
bool get_rows_count(napi_env env, napi_value v, const char* what, uint64_t* out) {      // a cursor position or a cap: a whole number below 2^53
  double d;
  if (!get_count(env, v, &d)) return false;
  if (!(d >= 0) || d > 9007199254740991.0 || d != floor(d)) { napi_throw_range_error(env, nullptr, (std::string("bmx: ") + what + " is a whole number >= 0").c_str()); return false; }
  *out = (uint64_t)d;
  return true;
}
napi_value rows_columns(napi_env env, uint32_t nf, uint64_t m, uint64_t cap, const int64_t* cells) {
  napi_value arr;
  NAPI_OK(napi_create_array_with_length(env, nf, &arr));
  for (uint32_t f = 0; f < nf; f++) {
    napi_value col = copy_ta(env, napi_bigint64_array, (size_t)m, cells + (size_t)f * cap);
    if (!col) return nullptr;
    NAPI_OK(napi_set_element(env, arr, f, col));
  }
  return arr;
}
// call(out_ids, out_val, out_ts, &res) -> rc, inside the handle's turn
template <class Kind, class Call> napi_value rows_answer(napi_env env, Handle<Kind>* h, const RowsTail& t, uint64_t cap, Call call) {
  const bool ts = (t.flags & BMX_ROWS_TS) != 0;
  if (cap > (1ull << 31)) { napi_throw_range_error(env, nullptr, "bmx: cap is 2^31 rows at most (page with start)"); return nullptr; }
  std::vector<uint64_t> ids(cap ? cap : 1);
  std::vector<int64_t> vals((size_t)t.nf * cap + 1), clk(ts ? (size_t)t.nf * cap + 1 : 1);
  bmx_rows_res r; int rc;
  { Turn turn(h->q); rc = call(ids.data(), vals.data(), clk.data(), &r); }
  if (rc) return fail<Kind>(env, h->p, rc);
  napi_value out = object_of(env, {{"ids", copy_ta(env, napi_biguint64_array, (size_t)r.n_out, ids.data())}, {"vals", rows_columns(env, t.nf, r.n_out, cap, vals.data())},
                                   {"nMatch", num(env, (double)r.n_match)}, {"nextPos", num(env, (double)r.next_pos)}, {"nextShard", num(env, r.next_shard)}, {"layout", num(env, (double)r.layout)}});
  if (out && ts) {
    napi_value c = rows_columns(env, t.nf, r.n_out, cap, clk.data());
    if (!c) return nullptr;
    napi_set_named_property(env, out, "ts", c);
  }
  return out;
}
napi_value WhereRows(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 7);
  uint32_t base; if (!get_u32(env, argv[1], &base)) return nullptr;
  Program P; if (!get_program(env, argv[2], &P)) return nullptr;
  RowsTail t; if (!get_rows_tail(env, argv + 3, &t)) return nullptr;
  uint64_t start, cap; if (!get_rows_count(env, argv[5], "start", &start) || !get_rows_count(env, argv[6], "cap", &cap)) return nullptr;
  return rows_answer(env, h, t, cap, [&](uint64_t* ids, int64_t* vals, int64_t* clk, bmx_rows_res* r) {
    return bmx_where_rows(h->p, base, P.nc, P.lens, P.lits.data(), t.nf, t.fields, t.flags, start, cap, ids, vals, clk, r, BMX_MEM_HOST);
  });
}
napi_value CommWhereRows(napi_env env, napi_callback_info info) {
  HANDLE(Comm, 8);
  uint32_t base; if (!get_u32(env, argv[1], &base)) return nullptr;
  Program P; if (!get_program(env, argv[2], &P)) return nullptr;
  RowsTail t; if (!get_rows_tail(env, argv + 3, &t)) return nullptr;
  uint32_t shard; if (!get_u32(env, argv[5], &shard)) return nullptr;
  uint64_t start, cap; if (!get_rows_count(env, argv[6], "start", &start) || !get_rows_count(env, argv[7], "cap", &cap)) return nullptr;
  return rows_answer(env, h, t, cap, [&](uint64_t* ids, int64_t* vals, int64_t* clk, bmx_rows_res* r) {
    return bmx_comm_where_rows(h->p, base, P.nc, P.lens, P.lits.data(), t.nf, t.fields, t.flags, shard, start, cap, ids, vals, clk, r);
  });
}

// ---- the engine alone -----------------------------------------------------------------------------------------------------------------
napi_value Create(napi_env env, napi_callback_info info) {
  ARGS(2);
  int32_t device; double cap;
  NAPI_OK(napi_get_value_int32(env, argv[0], &device));
  if (!get_count(env, argv[1], &cap)) return nullptr;
  bmx_ctx* ctx = nullptr;
  int rc = bmx_create(device, (uint64_t)cap, 0, &ctx);
  return rc ? fail<Engine>(env, nullptr, rc) : wrap<Engine>(env, ctx);
}

// mergeBatch(h, id, field, ts, val, mode) -> {applied: Uint32Array, flags: Uint8Array, nApplied, nConflicts, nRows}
napi_value MergeBatch(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 6);
  Cols c; if (!get_cols(env, argv + 1, &c)) return nullptr;
  int32_t mode; NAPI_OK(napi_get_value_int32(env, argv[5], &mode));
  std::vector<uint32_t> applied(c.n ? c.n : 1);
  void* fl = nullptr;
  napi_value flags = make_ta(env, napi_uint8_array, c.n, &fl); if (!flags) return nullptr;
  uint64_t na = 0; bmx_merge_stats st; memset(&st, 0, sizeof(st));
  Turn turn(h->q);
  int rc = bmx_merge_batch(h->p, c.n, c.id, c.field, c.ts, c.val, mode, BMX_MEM_HOST, applied.data(), &na, (uint8_t*)fl, &st);
  return rc ? fail<Engine>(env, h->p, rc) : merge_result(env, applied.data(), na, &flags, st);
}

// mergeBatchAsync(h, id, field, ts, val, mode) -> Promise<{applied, flags, nApplied, nConflicts, nRows}>: the H2D copy, kernels and D2H copy run on a
// libuv worker thread; resolves to the same object as mergeBatch
struct MergeJob : Job<Engine> {
  Cols c; int mode = 0;
  std::vector<uint32_t> applied; std::vector<uint8_t> flags;
  uint64_t na = 0; bmx_merge_stats st;
  int run() override { return bmx_merge_batch(h->p, c.n, c.id, c.field, c.ts, c.val, mode, BMX_MEM_HOST, applied.data(), &na, flags.data(), &st); }
  napi_value result(napi_env env) override {
    napi_value fl = copy_ta(env, napi_uint8_array, c.n, flags.data());
    return fl ? merge_result(env, applied.data(), na, &fl, st) : nullptr;
  }
};
napi_value MergeBatchAsync(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 6);
  Cols c; if (!get_cols(env, argv + 1, &c)) return nullptr;
  int32_t mode; if (napi_get_value_int32(env, argv[5], &mode) != napi_ok) { napi_throw_type_error(env, nullptr, "bmx: bad mode"); return nullptr; }
  MergeJob* j = new MergeJob();
  j->h = h; j->c = c; j->mode = mode;
  j->applied.resize(c.n ? c.n : 1); j->flags.resize(c.n ? c.n : 1);
  memset(&j->st, 0, sizeof(j->st));
  return queue_job<Engine>(env, j, "bmx.mergeBatchAsync", argv, 5);   // the engine handle and the four columns
}

napi_value Reserve(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 2);
  double cap; if (!get_count(env, argv[1], &cap)) return nullptr;
  Turn turn(h->q);
  int rc = bmx_reserve(h->p, (uint64_t)cap);
  return rc ? fail<Engine>(env, h->p, rc) : nullptr;
}
/* indexOrderedInfo(handle, field) -> {afterQueries, valid, sorts, ...} */
napi_value IndexOrderedInfo(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 2);
  uint32_t f; if (!get_u32(env, argv[1], &f)) return nullptr;
  Turn turn(h->q);
  uint32_t after = 0; int valid = 0; uint64_t sorts = 0;
  int rc = bmx_index_ordered_info(h->p, f, &after, &valid, &sorts);
  if (rc) return fail<Engine>(env, h->p, rc);
  napi_value out; NAPI_OK(napi_create_object(env, &out));
  set_num(env, out, "afterQueries", after); set_num(env, out, "valid", valid); set_num(env, out, "sorts", (double)sorts);
  // round 5 (ABI 4): what kept the view current — patches from the change log instead of sorts (bmx_index_ordered_stats)
  uint64_t s2 = 0, patches = 0, keys = 0, rewrites = 0, pending = 0; double sort_us = 0, patch_us = 0;
  if (bmx_index_ordered_stats(h->p, f, &s2, &patches, &keys, &sort_us, &patch_us, &rewrites, &pending) == BMX_OK) {
    set_num(env, out, "patches", (double)patches); set_num(env, out, "keysPatched", (double)keys); set_num(env, out, "lastSortUs", sort_us); set_num(env, out, "lastPatchUs", patch_us);
    set_num(env, out, "rewrites", (double)rewrites); set_num(env, out, "pendingKeys", (double)pending);
  }
  return out;
}
napi_value IndexDrop(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 2);
  uint32_t f; if (!get_u32(env, argv[1], &f)) return nullptr;
  Turn turn(h->q);
  int rc = bmx_index_drop(h->p, f);
  return rc && rc != BMX_ERR_NO_INDEX ? fail<Engine>(env, h->p, rc) : nullptr;
}
napi_value IndexSize(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 2);
  uint32_t f; if (!get_u32(env, argv[1], &f)) return nullptr;
  Turn turn(h->q);
  uint64_t n = 0; int rc = bmx_index_size(h->p, f, &n);
  return rc ? fail<Engine>(env, h->p, rc) : num(env, (double)n);
}
// indexRefreshCounts(h) -> {fullBuilds, incremental}: how often the indexes were rebuilt from the table / brought up to date from the change log
napi_value IndexRefreshCounts(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 1);
  Turn turn(h->q);
  uint64_t a = 0, b = 0; int rc = bmx_index_refresh_counts(h->p, &a, &b);
  return rc ? fail<Engine>(env, h->p, rc) : object_of(env, {{"fullBuilds", num(env, (double)a)}, {"incremental", num(env, (double)b)}});
}
// scanRangePos(h, field, lo, hi) -> Uint32Array of index positions (ascending): no id gather on the device, no id -> path lookup on the host
napi_value ScanRangePos(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 4);
  uint32_t f; int64_t lo, hi; if (!get_u32(env, argv[1], &f) || !get_i64(env, argv[2], &lo) || !get_i64(env, argv[3], &hi)) return nullptr;
  return scan_result(env, h, napi_uint32_array, [&](uint64_t* m) { return bmx_scan_count(h->p, f, lo, hi, m, BMX_MEM_HOST); },
                     [&](void* out, uint64_t m) { uint64_t m2 = 0; return bmx_scan_range_pos(h->p, f, lo, hi, (uint32_t*)out, m, &m2, BMX_MEM_HOST); });
}
// indexIds(h, field, first, count) -> BigUint64Array: node ids of index positions [first, first + count)
napi_value IndexIds(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 4);
  uint32_t f; double first, count; if (!get_u32(env, argv[1], &f) || !get_count(env, argv[2], &first) || !get_count(env, argv[3], &count)) return nullptr;
  Turn turn(h->q);
  // validated BEFORE anything is allocated: a negative, fractional or NaN count cast to size_t is undefined behaviour or a huge allocation
  uint64_t size = 0; int rc = bmx_index_size(h->p, f, &size);
  if (rc) return fail<Engine>(env, h->p, rc);
  if (!(first >= 0 && count >= 0) || first != std::floor(first) || count != std::floor(count) || first > (double)size || count > (double)size - first) {
    napi_throw_range_error(env, nullptr, "bmx: indexIds(first, count) reaches outside the index");
    return nullptr;
  }
  void* out; napi_value ta = make_ta(env, napi_biguint64_array, (size_t)count, &out); if (!ta) return nullptr;
  rc = bmx_index_ids(h->p, f, (uint64_t)first, (uint64_t)count, (uint64_t*)out, BMX_MEM_HOST);
  return rc ? fail<Engine>(env, h->p, rc) : ta;
}
// scanFilter(h, [[field, lo, hi], ...]) -> BigUint64Array; sized by the first term's index
napi_value ScanFilter(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 2);
  bmx_term terms[8]; const uint32_t nt = get_terms(env, argv[1], "filter", terms); if (!nt) return nullptr;
  Turn turn(h->q);
  uint64_t cap = 0; int rc = bmx_index_size(h->p, terms[0].field, &cap);
  if (rc) return fail<Engine>(env, h->p, rc);
  std::vector<uint64_t> tmp(cap ? cap : 1);
  uint64_t m = 0; rc = bmx_scan_filter(h->p, nt, terms, tmp.data(), cap, &m, BMX_MEM_HOST);
  return rc ? fail<Engine>(env, h->p, rc) : copy_ta(env, napi_biguint64_array, m, tmp.data());
}
napi_value Info(napi_env env, napi_callback_info info) {
  HANDLE(Engine, 1);
  Turn turn(h->q);
  bmx_info i; int rc = bmx_get_info(h->p, &i);
  if (rc) return fail<Engine>(env, h->p, rc);
  napi_value out; NAPI_OK(napi_create_object(env, &out));
  set_num(env, out, "capacityRows", (double)i.capacity_rows); set_num(env, out, "nSlots", (double)i.n_slots);
  set_num(env, out, "tableBytes", (double)i.table_bytes); set_num(env, out, "nRows", (double)i.n_rows);
  set_num(env, out, "device", i.device); set_num(env, out, "abiVersion", i.abi_version); set_num(env, out, "nIndexes", i.n_indexes);
  return out;
}

// ---- N4: vector-clock table (bmx_vc_*) -----------------------------------------------------------------------------
// vcCreate(device, capacityRows, kWriters, localWriter) -> handle
napi_value VcCreate(napi_env env, napi_callback_info info) {
  ARGS(4);
  int32_t device; double cap; uint32_t K, local;
  NAPI_OK(napi_get_value_int32(env, argv[0], &device));
  if (!get_count(env, argv[1], &cap) || !get_u32(env, argv[2], &K) || !get_u32(env, argv[3], &local)) return nullptr;
  bmx_vc* t = nullptr;
  int rc = bmx_vc_create(device, (uint64_t)cap, K, local, &t);
  return rc ? fail<Vc>(env, nullptr, rc) : wrap<Vc>(env, t, K);
}

// (id BigUint64Array, field Uint32Array, clocks Uint32Array[n*K], val BigInt64Array[, keysets Uint32Array[n]]): keysets say which writers each clock names,
// in which order (include/bmx.h); absent / undefined = all K, in order
struct VcCols { const uint64_t* id; const uint32_t *field, *clocks, *ks; const int64_t* val; size_t n; };
bool get_vc_cols(napi_env env, size_t argc, napi_value* argv, uint32_t K, VcCols* c) {
  size_t n1, n2, n3, nk;
  if (!get_ta(env, argv[1], napi_biguint64_array, &c->id, &c->n) || !get_ta(env, argv[2], napi_uint32_array, &c->field, &n1) ||
      !get_ta(env, argv[3], napi_uint32_array, &c->clocks, &n2) || !get_ta(env, argv[4], napi_bigint64_array, &c->val, &n3)) return false;
  if (c->n != n1 || c->n != n3 || n2 != c->n * K) { napi_throw_range_error(env, nullptr, "bmx: column lengths differ (clocks must hold n*K counters)"); return false; }
  c->ks = nullptr;
  if (argc <= 5 || is_nullish(env, argv[5])) return true;
  if (!get_ta(env, argv[5], napi_uint32_array, &c->ks, &nk)) return false;
  if (nk != c->n) { napi_throw_range_error(env, nullptr, "bmx: keysets must hold one word per row"); return false; }
  return true;
}
// {updated, flags, [rows,] nRows}
napi_value vc_merge_result(napi_env env, const uint32_t* upd, uint64_t nu, napi_value flags, const napi_value* rows, uint64_t nrows) {
  napi_value updated = copy_ta(env, napi_uint32_array, (size_t)nu, upd);
  napi_value out = rows ? object_of(env, {{"updated", updated}, {"flags", flags}, {"rows", *rows}}) : object_of(env, {{"updated", updated}, {"flags", flags}});
  if (out) set_num(env, out, "nRows", (double)nrows);
  return out;
}

// vcLoadRows(h, id, field, clocks, val[, keysets])
napi_value VcLoadRows(napi_env env, napi_callback_info info) {
  ARGS_OPT(5, 6);
  Handle<Vc>* h = get_handle<Vc>(env, argv[0]); if (!h) return nullptr;
  VcCols c; if (!get_vc_cols(env, argc, argv, h->K, &c)) return nullptr;
  Turn turn(h->q);
  int rc = bmx_vc_load_rows_ks(h->p, c.n, c.id, c.field, c.clocks, c.ks, c.val);
  return rc ? fail<Vc>(env, h->p, rc) : nullptr;
}

// vcMergeBatch(h, id, field, clocks, val[, keysets]) -> {updated: Uint32Array, flags: Uint8Array, nRows}
napi_value VcMergeBatch(napi_env env, napi_callback_info info) {
  ARGS_OPT(5, 6);
  Handle<Vc>* h = get_handle<Vc>(env, argv[0]); if (!h) return nullptr;
  VcCols c; if (!get_vc_cols(env, argc, argv, h->K, &c)) return nullptr;
  std::vector<uint32_t> upd(c.n ? c.n : 1);
  void* fl = nullptr;
  napi_value flags = make_ta(env, napi_uint8_array, c.n, &fl); if (!flags) return nullptr;
  uint64_t nu = 0, rows = 0;
  Turn turn(h->q);
  int rc = bmx_vc_merge_batch_ks(h->p, c.n, c.id, c.field, c.clocks, c.ks, c.val, upd.data(), &nu, (uint8_t*)fl);
  if (rc) return fail<Vc>(env, h->p, rc);
  bmx_vc_row_count(h->p, &rows);
  return vc_merge_result(env, upd.data(), nu, flags, nullptr, rows);
}

// vcMergeBatchAsync(h, id, field, clocks, val[, keysets]) -> Promise<{updated, flags, nRows, rows: {clocks, keysets} of the updated rows}>: the upload,
// the kernels and the read-back of the updated rows' clocks run on a libuv worker thread, in issue order with every other operation on the table
// (reference seam: the sync loop src/bullet-network-sync.js:551-569 under general vector clocks, src/bullet-crt.js:68-153). The rows' clocks come back
// with the merge because a later merge — already in flight when this one is applied — would have moved them.
struct VcJob : Job<Vc> {
  VcCols c;
  std::vector<uint32_t> upd, rclocks, rks; std::vector<uint8_t> flags, rstate; std::vector<int64_t> rval;
  uint64_t nu = 0, rows = 0;
  int run() override {
    int rc = bmx_vc_merge_batch_ks(h->p, c.n, c.id, c.field, c.clocks, c.ks, c.val, upd.data(), &nu, flags.data());
    if (rc) return rc;
    bmx_vc_row_count(h->p, &rows);
    if (!nu) return BMX_OK;
    std::vector<uint64_t> ids(nu); std::vector<uint32_t> fields(nu);
    for (uint64_t k = 0; k < nu; k++) { ids[k] = c.id[upd[k]]; fields[k] = c.field[upd[k]]; }
    rclocks.resize(nu * h->K); rks.resize(nu); rval.resize(nu); rstate.resize(nu);
    return bmx_vc_get_rows_ks(h->p, nu, ids.data(), fields.data(), rclocks.data(), rks.data(), rval.data(), rstate.data());
  }
  napi_value result(napi_env env) override {
    napi_value fl = copy_ta(env, napi_uint8_array, c.n, flags.data());
    napi_value rows_of = object_of(env, {{"clocks", copy_ta(env, napi_uint32_array, (size_t)nu * h->K, rclocks.data())}, {"keysets", copy_ta(env, napi_uint32_array, (size_t)nu, rks.data())}});
    return fl && rows_of ? vc_merge_result(env, upd.data(), nu, fl, &rows_of, rows) : nullptr;
  }
};
napi_value VcMergeBatchAsync(napi_env env, napi_callback_info info) {
  ARGS_OPT(5, 6);
  Handle<Vc>* h = get_handle<Vc>(env, argv[0]); if (!h) return nullptr;
  VcCols c; if (!get_vc_cols(env, argc, argv, h->K, &c)) return nullptr;
  VcJob* j = new VcJob();
  j->h = h; j->c = c;
  j->upd.resize(c.n ? c.n : 1); j->flags.resize(c.n ? c.n : 1);
  return queue_job<Vc>(env, j, "bmx.vcMergeBatchAsync", argv, std::min<size_t>(argc, 6));   // the table handle and the columns
}

// vcGetRows(h, id, field) -> {clocks: Uint32Array[n*K], val: BigInt64Array, state: Uint8Array, keysets: Uint32Array}
napi_value VcGetRows(napi_env env, napi_callback_info info) {
  HANDLE(Vc, 3);
  Cols k; if (!get_keys(env, argv + 1, &k)) return nullptr;
  void *c = nullptr, *v = nullptr, *st = nullptr, *ks = nullptr;
  napi_value clocks = make_ta(env, napi_uint32_array, k.n * h->K, &c), val = make_ta(env, napi_bigint64_array, k.n, &v), state = make_ta(env, napi_uint8_array, k.n, &st);
  napi_value out = object_of(env, {{"keysets", make_ta(env, napi_uint32_array, k.n, &ks)}, {"clocks", clocks}, {"val", val}, {"state", state}});
  if (!out) return nullptr;
  Turn turn(h->q);
  int rc = bmx_vc_get_rows_ks(h->p, k.n, k.id, k.field, (uint32_t*)c, (uint32_t*)ks, (int64_t*)v, (uint8_t*)st);
  return rc ? fail<Vc>(env, h->p, rc) : out;
}

// vcScanRange(h, field, lo, hi) -> BigUint64Array of node ids (rows of `field` with lo <= val <= hi)
napi_value VcScanRange(napi_env env, napi_callback_info info) {
  HANDLE(Vc, 4);
  uint32_t f; int64_t lo, hi; if (!get_u32(env, argv[1], &f) || !get_i64(env, argv[2], &lo) || !get_i64(env, argv[3], &hi)) return nullptr;
  return scan_result(env, h, napi_biguint64_array, [&](uint64_t* m) { return bmx_vc_scan_range(h->p, f, lo, hi, nullptr, 0, m); },
                     [&](void* out, uint64_t m) { uint64_t m2 = 0; return bmx_vc_scan_range(h->p, f, lo, hi, (uint64_t*)out, m, &m2); });
}
napi_value VcRowCount(napi_env env, napi_callback_info info) {
  HANDLE(Vc, 1);
  Turn turn(h->q);
  uint64_t n = 0; int rc = bmx_vc_row_count(h->p, &n);
  return rc ? fail<Vc>(env, h->p, rc) : num(env, (double)n);
}

// ---- N shards in one process (bmx_comm_*): one JS object owns all GPUs of the node ------------------------------------
// commCreate([device, device, ...], capacityRowsPerShard) -> handle   (a device may be listed several times: logical shards)
napi_value CommCreate(napi_env env, napi_callback_info info) {
  ARGS(2);
  uint32_t n = 0; NAPI_OK(napi_get_array_length(env, argv[0], &n));
  if (n == 0 || n > 16) { napi_throw_range_error(env, nullptr, "bmx: a communicator has 1..16 shards"); return nullptr; }
  std::vector<int> devs(n);
  for (uint32_t i = 0; i < n; i++) { napi_value e; NAPI_OK(napi_get_element(env, argv[0], i, &e)); int32_t d; NAPI_OK(napi_get_value_int32(env, e, &d)); devs[i] = d; }
  double cap; if (!get_count(env, argv[1], &cap)) return nullptr;
  bmx_comm* c = nullptr;
  int rc = bmx_comm_create(n, devs.data(), (uint64_t)cap, 0, &c);
  return rc ? fail<Comm>(env, nullptr, rc) : wrap<Comm>(env, c);
}
// commMergeBatch(h, id, field, ts, val, mode) -> {applied: Uint32Array (indices into this batch), nApplied, nConflicts, nRows}
napi_value CommMergeBatch(napi_env env, napi_callback_info info) {
  HANDLE(Comm, 6);
  Cols c; if (!get_cols(env, argv + 1, &c)) return nullptr;
  int32_t mode; NAPI_OK(napi_get_value_int32(env, argv[5], &mode));
  std::vector<uint32_t> applied(c.n ? c.n : 1);
  uint64_t na = 0; bmx_merge_stats st; memset(&st, 0, sizeof(st));
  Turn turn(h->q);
  int rc = bmx_comm_merge(h->p, c.n, c.id, c.field, c.ts, c.val, mode, applied.data(), &na, &st);
  return rc ? fail<Comm>(env, h->p, rc) : merge_result(env, applied.data(), na, nullptr, st);
}
napi_value CommIndexDrop(napi_env env, napi_callback_info info) {   // every shard, whatever it answers
  HANDLE(Comm, 2);
  uint32_t f; if (!get_u32(env, argv[1], &f)) return nullptr;
  Turn turn(h->q);
  for (uint32_t s = 0; s < bmx_comm_nshards(h->p); s++) (void)bmx_index_drop(bmx_comm_shard(h->p, s), f);
  return nullptr;
}
napi_value CommIndexSize(napi_env env, napi_callback_info info) {   // the shards' sizes added; a shard's error is that shard's
  HANDLE(Comm, 2);
  uint32_t f; if (!get_u32(env, argv[1], &f)) return nullptr;
  Turn turn(h->q);
  uint64_t tot = 0;
  for (uint32_t s = 0; s < bmx_comm_nshards(h->p); s++) {
    uint64_t n = 0; int rc = bmx_index_size(bmx_comm_shard(h->p, s), f, &n);
    if (rc) return fail<Engine>(env, bmx_comm_shard(h->p, s), rc);
    tot += n;
  }
  return num(env, (double)tot);
}
napi_value CommScanFilter(napi_env env, napi_callback_info info) {   // counts first: the shards' indexes have no common size
  HANDLE(Comm, 2);
  bmx_term terms[8]; const uint32_t nt = get_terms(env, argv[1], "filter", terms); if (!nt) return nullptr;
  return scan_result(env, h, napi_biguint64_array, [&](uint64_t* m) { return bmx_comm_scan_filter(h->p, nt, terms, nullptr, 0, m); },
                     [&](void* out, uint64_t m) { uint64_t m2 = 0; return bmx_comm_scan_filter(h->p, nt, terms, (uint64_t*)out, m, &m2); });
}

napi_value Init(napi_env env, napi_value exports) {
  struct { const char* name; napi_callback fn; } fns[] = {
      {"abiVersion", AbiVersion}, {"ownersOf", OwnersOf}, {"hostColumns", HostColumns},
      {"create", Create}, {"destroy", Destroy<Engine>}, {"mergeBatch", MergeBatch}, {"mergeBatchAsync", MergeBatchAsync}, {"reserve", Reserve}, {"indexDrop", IndexDrop},
      {"indexOrderedInfo", IndexOrderedInfo}, {"indexSize", IndexSize}, {"indexRefreshCounts", IndexRefreshCounts}, {"scanRangePos", ScanRangePos}, {"indexIds", IndexIds},
      {"scanFilter", ScanFilter}, {"info", Info},
      {"loadRows", StoreRows<Engine, false>}, {"putRows", StoreRows<Engine, true>}, {"getRows", GetRows<Engine>}, {"rowCount", RowCount<Engine>}, {"dumpRows", DumpRows<Engine>},
      {"indexBuild", IndexBuild<Engine>}, {"indexSetOrdered", IndexSetOrdered<Engine>}, {"scanRange", ScanRange<Engine>}, {"scanCount", ScanCount<Engine>}, {"digest", Digest<Engine>},
      {"exportRows", ExportRows<Engine>}, {"scanAggregate", ScanAggregate<Engine>}, {"scanTop", ScanTop<Engine>}, {"scanWhere", ScanWhere<Engine>},
      {"whereAggregate", WhereAggregate<Engine>}, {"whereTop", WhereTop<Engine>}, {"commWhereAggregate", WhereAggregate<Comm>}, {"commWhereTop", WhereTop<Comm>},
      {"whereRows", WhereRows}, {"commWhereRows", CommWhereRows},
      {"commLoadRows", StoreRows<Comm, false>}, {"commPutRows", StoreRows<Comm, true>}, {"commGetRows", GetRows<Comm>}, {"commRowCount", RowCount<Comm>}, {"commDumpRows", DumpRows<Comm>},
      {"commIndexBuild", IndexBuild<Comm>}, {"commIndexSetOrdered", IndexSetOrdered<Comm>}, {"commScanRange", ScanRange<Comm>}, {"commScanCount", ScanCount<Comm>}, {"commDigest", Digest<Comm>},
      {"commExportRows", ExportRows<Comm>}, {"commScanAggregate", ScanAggregate<Comm>}, {"commScanTop", ScanTop<Comm>}, {"commScanWhere", ScanWhere<Comm>},
      {"commCreate", CommCreate}, {"commDestroy", Destroy<Comm>}, {"commMergeBatch", CommMergeBatch}, {"commIndexDrop", CommIndexDrop}, {"commIndexSize", CommIndexSize}, {"commScanFilter", CommScanFilter},
      {"vcCreate", VcCreate}, {"vcDestroy", Destroy<Vc>}, {"vcLoadRows", VcLoadRows}, {"vcMergeBatch", VcMergeBatch}, {"vcMergeBatchAsync", VcMergeBatchAsync}, {"vcGetRows", VcGetRows},
      {"vcRowCount", VcRowCount}, {"vcScanRange", VcScanRange}};
  for (auto& f : fns) {
    napi_value v;
    if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &v) != napi_ok) return nullptr;
    napi_set_named_property(env, exports, f.name, v);
  }
  struct { const char* name; int v; } consts[] = {{"INSERT_REFERENCE", BMX_INSERT_REFERENCE}, {"INSERT_DELTA", BMX_INSERT_DELTA},
                                                  {"MERGE_UNIQUE_KEYS", BMX_MERGE_UNIQUE_KEYS}, {"MERGE_STRICT_FLAGS", BMX_MERGE_STRICT_FLAGS}, {"MERGE_MARK_CREATED", BMX_MERGE_MARK_CREATED}, {"FLAG_INCOMING", BMX_FLAG_INCOMING},
                                                  {"FLAG_CURRENT", BMX_FLAG_CURRENT}, {"FLAG_HISTORICAL", BMX_FLAG_HISTORICAL}, {"FLAG_CONCURRENT", BMX_FLAG_CONCURRENT},
                                                  {"VC_MAX_WRITERS", BMX_VC_MAX_WRITERS}, {"VC_ABSENT", BMX_VC_ABSENT}, {"VC_DENSE", BMX_VC_DENSE}, {"VC_SPARSE", BMX_VC_SPARSE}};
  for (auto& c : consts) { napi_value v; napi_create_int32(env, c.v, &v); napi_set_named_property(env, exports, c.name, v); }
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
