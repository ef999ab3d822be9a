// bmx_query.inc — what the queries over an index (range and filter scans, the ordered view's launches, aggregates, top-k, the digest's grid) set up the same
// way in front of their launches. Host arithmetic only: nothing here launches a kernel, so its place in bmx.hip's include list moves nothing in the code object.
namespace {

// a filter has 1..MAX_TERMS terms; `msg` is the caller's own text for a list that has not (nullptr: the list is fine)
inline const char* bad_terms(uint32_t nterms, const bmx_term* terms, const char* msg) { return (nterms == 0 || nterms > (uint32_t)MAX_TERMS || !terms) ? msg : nullptr; }
// values live in +-(2^53-1): a lower bound raised to -VAL_MAX changes no answer and keeps tombstones (INT64_MIN) out of every range
inline int64_t above_tombstones(int64_t lo) { return std::max<int64_t>(lo, -VAL_MAX); }
// the caller's terms as the kernels take them: no term matches a tombstone
inline void copy_terms(bmx_term* dst, const bmx_term* terms, uint32_t nterms) {
  for (uint32_t k = 0; k < nterms; k++) { dst[k] = terms[k]; dst[k].lo = above_tombstones(terms[k].lo); }
}
// A range over a 4-byte column (or a view sorted from one): the bounds clamped into int32. INT32_MIN itself is what a tombstone looks like there and is never
// matched (a real -2^31 makes the index wide: scan_kernels.h v32_of); a range that lies outside int32 altogether stays empty.
struct Range32 { int64_t lo, hi; };
inline Range32 clamp_i32(int64_t lo, int64_t hi) {
  if (lo > INT32_MAX || hi < INT32_MIN) return {1, 0};
  return {std::max<int64_t>(lo, (int64_t)INT32_MIN + 1), std::min<int64_t>(hi, INT32_MAX)};
}
// the workgroups of one sweep over `work` items, `per_wg` to a workgroup at least: two per CU at most, one at least
inline uint32_t sweep_grid(const bmx_ctx* ctx, uint64_t work, uint64_t per_wg) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((work + per_wg - 1) / per_wg, 2ull * (uint64_t)ctx->cus));
}

}  // namespace
