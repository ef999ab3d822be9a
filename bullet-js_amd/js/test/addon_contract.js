"use strict";
/*
 * addon_contract.js — what bmx.node promises the JS host, written down: the exported names, the class, text and .code of every error, the type of
 * every result member, what a closed (or foreign) handle does, and the order in which operations on one handle run.
 *
 *   node addon_contract.js host                      no device needed: exports, constants, argument errors, dead handles
 *   node addon_contract.js gpu [--no-wrong-kind]     engine, vector-clock table (K = 2), communicators of one and of two logical shards on device 0
 *   [--addon=PATH]                                   another build of the addon (default: bullet-js_amd/bmx.node)
 *
 * Result values are asserted only where the inputs alone fix them (rows stored as given, keys that are new to the table, a scan against a plain
 * filter of the stored column): no expected value comes from the merge rule. --no-wrong-kind leaves out the handles of another kind; an addon
 * that does not tag its handles reads them as its own, which is undefined behaviour in this process.
 */
const assert = require("assert");
const path = require("path");

const args = process.argv.slice(2);
const mode = args[0];
const addonArg = args.find((a) => a.startsWith("--addon="));
const wrongKind = !args.includes("--no-wrong-kind");
const b = require(addonArg ? path.resolve(addonArg.slice(8)) : path.join(__dirname, "..", "..", "bmx.node"));
let checks = 0;

const FUNCTIONS = ["abiVersion", "create", "destroy", "mergeBatch", "mergeBatchAsync", "reserve", "loadRows", "putRows", "hostColumns", "scanRangePos", "indexIds",
  "commPutRows", "getRows", "rowCount", "dumpRows", "indexBuild", "indexDrop", "indexSetOrdered", "indexOrderedInfo", "indexSize", "indexRefreshCounts", "scanRange",
  "scanCount", "scanFilter", "info", "vcCreate", "vcDestroy", "vcLoadRows", "vcMergeBatch", "vcMergeBatchAsync", "vcGetRows", "vcRowCount", "vcScanRange", "ownersOf",
  "commCreate", "commDestroy", "commMergeBatch", "commLoadRows", "commGetRows", "commRowCount", "commDumpRows", "digest", "exportRows", "commDigest", "commExportRows",
  "commIndexBuild", "commIndexSetOrdered", "commIndexDrop", "commIndexSize", "commScanRange", "commScanCount", "commScanFilter", "scanAggregate", "commScanAggregate",
  "scanTop", "commScanTop", "scanWhere", "commScanWhere", "whereAggregate", "commWhereAggregate", "whereTop", "commWhereTop", "whereRows", "commWhereRows"];
const CONSTANTS = { INSERT_REFERENCE: 0, INSERT_DELTA: 1, MERGE_UNIQUE_KEYS: 0x100, MERGE_STRICT_FLAGS: 0x200, MERGE_MARK_CREATED: 0x1000, FLAG_INCOMING: 1, FLAG_CURRENT: 2,
  FLAG_HISTORICAL: 4, FLAG_CONCURRENT: 8, VC_MAX_WRITERS: 8, VC_ABSENT: 0, VC_DENSE: 1, VC_SPARSE: 2 };   // include/bmx.h

const CLOSED = { engine: "bmx: invalid or closed engine handle", vc: "bmx: invalid or closed vector-clock table handle", comm: "bmx: invalid or closed communicator handle" };
const DESTROY = { engine: "destroy", vc: "vcDestroy", comm: "commDestroy" };
const LENGTHS = "bmx: column lengths differ";

/* fn throws an error of exactly class `cls`; message: the whole text, or {prefix}; code: the .code, or undefined for "has none" */
function throwsWith(fn, cls, message, code, what) {
  let e = null;
  try { fn(); } catch (x) { e = x; }
  assert.ok(e, "no throw: " + (what || fn));
  assert.strictEqual(Object.getPrototypeOf(e), cls.prototype, (what || fn) + ": " + e);
  if (typeof message === "string") assert.strictEqual(e.message, message, what);
  else assert.ok(e.message.startsWith(message.prefix), (what || fn) + ": " + e.message);
  if (code === undefined) assert.ok(!("code" in e), (what || fn) + " carries a code");
  else assert.strictEqual(e.code, code, what);
  checks++;
}

/* one valid call of every function that takes a handle, per kind: what a closed or foreign handle is tried on */
const I1 = new BigUint64Array([5n]), F1 = new Uint32Array([7]), T1 = new BigInt64Array([3n]), V1 = new BigInt64Array([4n]), C2 = new Uint32Array([1, 1]);
const TERM = [[7, 0, 1]];
const CALLS = {
  engine: {
    mergeBatch: (h) => b.mergeBatch(h, I1, F1, T1, V1, 1), mergeBatchAsync: (h) => b.mergeBatchAsync(h, I1, F1, T1, V1, 1), reserve: (h) => b.reserve(h, 2048),
    loadRows: (h) => b.loadRows(h, I1, F1, T1, V1), putRows: (h) => b.putRows(h, I1, F1, T1, V1), getRows: (h) => b.getRows(h, I1, F1), rowCount: (h) => b.rowCount(h),
    dumpRows: (h) => b.dumpRows(h), indexBuild: (h) => b.indexBuild(h, 7), indexDrop: (h) => b.indexDrop(h, 7), indexSetOrdered: (h) => b.indexSetOrdered(h, 7, 1),
    indexOrderedInfo: (h) => b.indexOrderedInfo(h, 7), indexSize: (h) => b.indexSize(h, 7), indexRefreshCounts: (h) => b.indexRefreshCounts(h),
    scanRange: (h) => b.scanRange(h, 7, 0, 1), scanCount: (h) => b.scanCount(h, 7, 0, 1), scanRangePos: (h) => b.scanRangePos(h, 7, 0, 1), indexIds: (h) => b.indexIds(h, 7, 0, 0),
    scanFilter: (h) => b.scanFilter(h, TERM), info: (h) => b.info(h), digest: (h) => b.digest(h, 4, false), exportRows: (h) => b.exportRows(h, 0, 4, null, false),
    scanAggregate: (h) => b.scanAggregate(h, TERM, null, null, 0, 0), scanTop: (h) => b.scanTop(h, TERM, false, null, 1),
    scanWhere: (h) => b.scanWhere(h, 7, [TERM]),
    whereAggregate: (h) => b.whereAggregate(h, 7, [TERM], null, null, 0, 0), whereTop: (h) => b.whereTop(h, 7, [TERM], false, null, 1),
    whereRows: (h) => b.whereRows(h, 7, [TERM], [7], false, 0, 1),
  },
  vc: {
    vcLoadRows: (h) => b.vcLoadRows(h, I1, F1, C2, V1), vcMergeBatch: (h) => b.vcMergeBatch(h, I1, F1, C2, V1), vcMergeBatchAsync: (h) => b.vcMergeBatchAsync(h, I1, F1, C2, V1),
    vcGetRows: (h) => b.vcGetRows(h, I1, F1), vcRowCount: (h) => b.vcRowCount(h), vcScanRange: (h) => b.vcScanRange(h, 7, 0, 1),
  },
  comm: {
    commMergeBatch: (h) => b.commMergeBatch(h, I1, F1, T1, V1, 1), commLoadRows: (h) => b.commLoadRows(h, I1, F1, T1, V1), commPutRows: (h) => b.commPutRows(h, I1, F1, T1, V1),
    commGetRows: (h) => b.commGetRows(h, I1, F1), commRowCount: (h) => b.commRowCount(h), commDumpRows: (h) => b.commDumpRows(h), commDigest: (h) => b.commDigest(h, 4, false),
    commExportRows: (h) => b.commExportRows(h, 0, 4, null, false), commIndexBuild: (h) => b.commIndexBuild(h, 7), commIndexSetOrdered: (h) => b.commIndexSetOrdered(h, 7, 1),
    commIndexDrop: (h) => b.commIndexDrop(h, 7), commIndexSize: (h) => b.commIndexSize(h, 7), commScanRange: (h) => b.commScanRange(h, 7, 0, 1),
    commScanCount: (h) => b.commScanCount(h, 7, 0, 1), commScanFilter: (h) => b.commScanFilter(h, TERM), commScanAggregate: (h) => b.commScanAggregate(h, TERM, null, null, 0, 0),
    commScanTop: (h) => b.commScanTop(h, TERM, false, null, 1),
    commScanWhere: (h) => b.commScanWhere(h, 7, [TERM]),
    commWhereAggregate: (h) => b.commWhereAggregate(h, 7, [TERM], null, null, 0, 0), commWhereTop: (h) => b.commWhereTop(h, 7, [TERM], false, null, 1),
    commWhereRows: (h) => b.commWhereRows(h, 7, [TERM], [7], false, 0, 0, 1),
  },
};

/* every function of `kind` refuses handle h with the kind's own text */
function refusedByAll(kind, h, what) {
  for (const [name, call] of Object.entries(CALLS[kind])) throwsWith(() => call(h), Error, CLOSED[kind], undefined, name + " on " + what);
}

function host() {
  assert.strictEqual(b.abiVersion(), 4);
  assert.deepStrictEqual(Object.keys(b).sort(), FUNCTIONS.concat(Object.keys(CONSTANTS)).sort());
  assert.strictEqual(Object.keys(b).length, 77);
  for (const k of FUNCTIONS) assert.strictEqual(typeof b[k], "function", k);
  for (const [k, v] of Object.entries(CONSTANTS)) assert.strictEqual(b[k], v, k);
  // the tables above name every function that takes a handle
  const NO_HANDLE = ["abiVersion", "create", "vcCreate", "commCreate", "hostColumns", "ownersOf"];
  const named = NO_HANDLE.concat(Object.values(DESTROY), ...Object.values(CALLS).map(Object.keys));
  assert.deepStrictEqual(named.slice().sort(), FUNCTIONS.slice().sort());
  checks += 5;

  throwsWith(() => b.commCreate([], 1000), RangeError, "bmx: a communicator has 1..16 shards");
  for (const kind of Object.keys(CALLS)) {
    refusedByAll(kind, {}, "{}");
    assert.strictEqual(b[DESTROY[kind]]({}), undefined);
    checks++;
  }
  throwsWith(() => b.rowCount(), TypeError, "bmx: missing arguments");
  const owners = b.ownersOf(new BigUint64Array([1n, 2n, 3n]), 4);
  assert.ok(owners instanceof Uint8Array);
  assert.deepStrictEqual(Array.from(owners), [3, 0, 1]);
  throwsWith(() => b.ownersOf(new BigUint64Array([1n]), 0), RangeError, "bmx: 1..255 shards");
  throwsWith(() => b.ownersOf(new Uint32Array([1]), 2), TypeError, "bmx: wrong typed-array type (id BigUint64Array, field Uint32Array, ts/val BigInt64Array)");
  throwsWith(() => b.hostColumns(0), RangeError, "bmx: hostColumns(n) wants 1 <= n <= 2^24");
  checks += 2;

  // what a machine without a device answers; with one, the same calls succeed and the gpu half covers them
  let h = null, refusal = null;
  try { h = b.create(0, 1000); } catch (e) { refusal = e; }
  if (h) { b.destroy(h); console.log("addon_contract host: a device is present, the no-device errors are not checked"); return; }
  const NO_DEVICE = "no HIP device: this library has no CPU path";
  throwsWith(() => b.create(0, 1000), Error, "bmx error -7: " + NO_DEVICE, -7);
  throwsWith(() => b.vcCreate(0, 1000, 2, 0), Error, "bmx error -7: " + NO_DEVICE, -7);
  throwsWith(() => b.commCreate([0], 1000), Error, "bmx error -7: shard 0: " + NO_DEVICE, -7);
  throwsWith(() => b.hostColumns(4), Error, { prefix: "bmx error -2: " }, -2);
  assert.strictEqual(refusal.code, -7);
  console.log("addon_contract host: no device");
}

/* ---- gpu half ---- */
const CAP = 1024, SIZES = [0, 1, 64, 65];   // 65 crosses one wave of 64
const seq = (n) => Array.from({ length: n }, (_, i) => i);
const isType = (x, cls, n, what) => { assert.strictEqual(Object.getPrototypeOf(x), cls.prototype, what); if (n !== undefined) assert.strictEqual(x.length, n, what); checks++; };
const isCount = (x, v, what) => { assert.strictEqual(typeof x, "number", what); assert.strictEqual(x, v, what); checks++; };
const sortedIds = (a) => Array.from(a).sort((x, y) => (x < y ? -1 : x > y ? 1 : 0));

/* n rows of `field` with ids base .. base + n - 1, clocks 10 + i and values in -50 .. 50 that a range splits */
function rows(base, n, field) {
  return { id: BigUint64Array.from(seq(n), (i) => BigInt(base + i)), field: new Uint32Array(n).fill(field), ts: BigInt64Array.from(seq(n), (i) => BigInt(10 + i)),
    val: BigInt64Array.from(seq(n), (i) => BigInt(((base + i) * 37) % 101 - 50)) };
}
function concat(list) {
  const n = list.reduce((s, r) => s + r.id.length, 0);
  const out = { id: new BigUint64Array(n), field: new Uint32Array(n), ts: new BigInt64Array(n), val: new BigInt64Array(n) };
  let at = 0;
  for (const r of list) { for (const k of Object.keys(out)) out[k].set(r[k], at); at += r.id.length; }
  return out;
}
const rowKeys = (r) => seq(r.id.length).map((i) => [r.id[i], r.field[i], r.ts[i], r.val[i]].join()).sort();
function mergeResult(r, n, nRows, flags, what) {
  isType(r.applied, Uint32Array, n, what); assert.deepStrictEqual(Array.from(r.applied), seq(n), what);
  if (flags) isType(r.flags, Uint8Array, n, what); else assert.ok(!("flags" in r), what);
  isCount(r.nApplied, n, what); isCount(r.nConflicts, 0, what);
  if (n) isCount(r.nRows, nRows, what); else assert.strictEqual(typeof r.nRows, "number", what);   // an empty batch returns before the library counts rows
}

/* the engine (prefix "") and a communicator (prefix "comm") answer to the same names */
async function tableContract(kind, open, what) {
  const f = (name) => b[kind === "comm" ? "comm" + name[0].toUpperCase() + name.slice(1) : name];
  const h = open();
  let nRows = 0, base = 1000;
  isCount(f("rowCount")(h), 0, what);
  // rows stored as given come back as given
  const stored = [];
  for (const store of ["loadRows", "putRows"]) for (const n of SIZES) {
    const r = rows(base, n, 7); base += n; nRows += n; stored.push(r);
    assert.strictEqual(f(store)(h, r.id, r.field, r.ts, r.val), undefined);
    const g = f("getRows")(h, r.id, r.field);
    isType(g.ts, BigInt64Array, n, what); isType(g.val, BigInt64Array, n, what); isType(g.found, Uint8Array, n, what);
    assert.deepStrictEqual([g.ts, g.val, Array.from(g.found)], [r.ts, r.val, seq(n).map(() => 1)], what + " " + store + " " + n);
    isCount(f("rowCount")(h), nRows, what);
  }
  const second = rows(1000, 65, 9);   // another field of the first 65 nodes, for a filter of two terms
  f("loadRows")(h, second.id, second.field, second.ts, second.val); nRows += 65; stored.push(second);
  const all = concat(stored), d = f("dumpRows")(h);
  isType(d.id, BigUint64Array, nRows, what); isType(d.field, Uint32Array, nRows, what); isType(d.ts, BigInt64Array, nRows, what); isType(d.val, BigInt64Array, nRows, what);
  assert.deepStrictEqual(rowKeys(d), rowKeys(all), what + " dumpRows");

  // scans over the stored column == a plain filter of it
  const col7 = concat(stored.slice(0, -1)), want = (lo, hi) => sortedIds(col7.id.filter((_, i) => col7.val[i] >= lo && col7.val[i] <= hi));
  const val9 = new Map(seq(65).map((i) => [second.id[i], second.val[i]]));
  assert.strictEqual(f("indexBuild")(h, 7), undefined); assert.strictEqual(f("indexBuild")(h, 9), undefined);
  isCount(f("indexSize")(h, 7), col7.id.length, what);
  for (const [lo, hi] of [[-10, 20], [-50, 50], [51, 60], [0n, 0n]]) {
    const w = want(BigInt(lo), BigInt(hi)), got = f("scanRange")(h, 7, lo, hi);
    isType(got, BigUint64Array, w.length, what); assert.deepStrictEqual(sortedIds(got), w, what + " scanRange");
    isCount(f("scanCount")(h, 7, lo, hi), w.length, what);
    if (kind === "engine") {
      const pos = b.scanRangePos(h, 7, lo, hi), ids = b.indexIds(h, 7, 0, col7.id.length);
      isType(pos, Uint32Array, w.length, what); isType(ids, BigUint64Array, col7.id.length, what);
      assert.ok(pos.every((p, i) => i === 0 || pos[i - 1] < p), "positions ascend");
      assert.deepStrictEqual(sortedIds(Array.from(pos, (p) => ids[p])), w, what + " scanRangePos");
    }
    const w2 = w.filter((id) => val9.has(id) && val9.get(id) >= -20n && val9.get(id) <= 30n), got2 = f("scanFilter")(h, [[7, lo, hi], [9, -20, 30]]);
    isType(got2, BigUint64Array, w2.length, what); assert.deepStrictEqual(sortedIds(got2), w2, what + " scanFilter");
  }

  // n keys that are new to the table: every one is applied
  for (const n of SIZES) {
    const r = rows(base, n, 11); base += n; nRows += n;
    mergeResult(f("mergeBatch")(h, r.id, r.field, r.ts, r.val, b.INSERT_DELTA), n, nRows, kind === "engine", what + " mergeBatch " + n);
    assert.deepStrictEqual(Array.from(f("getRows")(h, r.id, r.field).found), seq(n).map(() => 1), what);
    isCount(f("rowCount")(h), nRows, what);
  }

  // argument errors
  const two = new BigUint64Array(2);
  throwsWith(() => f("loadRows")(h, two, F1, T1, V1), RangeError, LENGTHS); throwsWith(() => f("putRows")(h, I1, F1, new BigInt64Array(2), V1), RangeError, LENGTHS);
  throwsWith(() => f("mergeBatch")(h, I1, F1, T1, new BigInt64Array(0), 1), RangeError, LENGTHS); throwsWith(() => f("getRows")(h, two, F1), RangeError, LENGTHS);
  if (kind === "engine") throwsWith(() => b.mergeBatchAsync(h, two, F1, T1, V1, 1), RangeError, LENGTHS);
  const nine = seq(9).map(() => [7, 0, 1]);
  for (const terms of [[], nine]) {
    throwsWith(() => f("scanFilter")(h, terms), RangeError, "bmx: filter needs 1..8 terms");
    throwsWith(() => f("scanAggregate")(h, terms, null, null, 0, 0), RangeError, "bmx: aggregate needs 1..8 terms");
    throwsWith(() => f("scanTop")(h, terms, false, null, 1), RangeError, "bmx: top needs 1..8 terms");
  }
  isCount(f("rowCount")(h), nRows, what);

  if (kind === "engine") {
    // a rejected promise carries what a thrown error carries
    await assert.rejects(b.mergeBatchAsync(h, new BigUint64Array([2n ** 64n - 1n]), new Uint32Array([1]), new BigInt64Array([1n]), new BigInt64Array([1n]), b.INSERT_DELTA),
      (e) => Object.getPrototypeOf(e) === Error.prototype && e.code === -5 && e.message.startsWith("bmx error -5: "));
    // issue order: A, a synchronous read of A's keys, B, destroy; nothing awaited in between
    const A = rows(base, 65, 11), B = rows(base + 65, 65, 11);
    const pA = b.mergeBatchAsync(h, A.id, A.field, A.ts, A.val, b.INSERT_DELTA);
    assert.ok(pA instanceof Promise);
    assert.deepStrictEqual(Array.from(b.getRows(h, A.id, A.field).found), seq(65).map(() => 1), "a read issued after A sees A");
    const pB = b.mergeBatchAsync(h, B.id, B.field, B.ts, B.val, b.INSERT_DELTA);
    assert.strictEqual(b.destroy(h), undefined);
    throwsWith(() => b.mergeBatchAsync(h, B.id, B.field, B.ts, B.val, b.INSERT_DELTA), Error, CLOSED.engine);
    mergeResult(await pA, 65, nRows + 65, true, what + " async A"); mergeResult(await pB, 65, nRows + 130, true, what + " async B");
    checks += 3;
  } else {
    assert.strictEqual(f("destroy")(h), undefined);
  }
  refusedByAll(kind, h, "a closed handle");
  assert.strictEqual(f("destroy")(h), undefined);   // a second close is a no-op
  checks++;
}

async function vcContract() {
  const K = 2, what = "vc";
  const h = b.vcCreate(0, CAP, K, 0);
  const vcRows = (base, n) => ({ id: BigUint64Array.from(seq(n), (i) => BigInt(base + i)), field: new Uint32Array(n).fill(7),
    clocks: Uint32Array.from(seq(n * K), (i) => 1 + (i % 5)), val: BigInt64Array.from(seq(n), (i) => BigInt(((base + i) * 37) % 101 - 50)) });
  const updated = (r, n, nRows, async, w) => {
    isType(r.updated, Uint32Array, n, w); assert.deepStrictEqual(Array.from(r.updated), seq(n), w); isType(r.flags, Uint8Array, n, w); isCount(r.nRows, nRows, w);
    if (async) { isType(r.rows.clocks, Uint32Array, n * K, w); isType(r.rows.keysets, Uint32Array, n, w); } else assert.ok(!("rows" in r), w);
  };
  let nRows = 0, base = 1000;
  isCount(b.vcRowCount(h), 0, what);
  const stored = [];
  for (const n of SIZES) {
    const r = vcRows(base, n); base += n; nRows += n; stored.push(r);
    assert.strictEqual(b.vcLoadRows(h, r.id, r.field, r.clocks, r.val), undefined);
    const g = b.vcGetRows(h, r.id, r.field);
    isType(g.clocks, Uint32Array, n * K, what); isType(g.val, BigInt64Array, n, what); isType(g.state, Uint8Array, n, what); isType(g.keysets, Uint32Array, n, what);
    assert.deepStrictEqual([g.clocks, g.val], [r.clocks, r.val], "vcLoadRows " + n);
    isCount(b.vcRowCount(h), nRows, what);
  }
  const ids = stored.flatMap((r) => Array.from(r.id)), vals = stored.flatMap((r) => Array.from(r.val));
  for (const [lo, hi] of [[-10, 20], [-50, 50], [51, 60]]) {
    const w = sortedIds(ids.filter((_, i) => vals[i] >= BigInt(lo) && vals[i] <= BigInt(hi))), got = b.vcScanRange(h, 7, lo, hi);
    isType(got, BigUint64Array, w.length, what); assert.deepStrictEqual(sortedIds(got), w, "vcScanRange");
  }
  for (const n of SIZES) {
    const r = vcRows(base, n); base += n; nRows += n;
    updated(b.vcMergeBatch(h, r.id, r.field, r.clocks, r.val), n, nRows, false, "vcMergeBatch " + n);
  }
  const two = new BigUint64Array(2), VC_LENGTHS = LENGTHS + " (clocks must hold n*K counters)";
  throwsWith(() => b.vcGetRows(h, two, F1), RangeError, LENGTHS); throwsWith(() => b.vcLoadRows(h, two, F1, C2, V1), RangeError, VC_LENGTHS);
  throwsWith(() => b.vcMergeBatch(h, I1, F1, new Uint32Array(1), V1), RangeError, VC_LENGTHS); throwsWith(() => b.vcMergeBatchAsync(h, I1, F1, C2, new BigInt64Array(2)), RangeError, VC_LENGTHS);
  throwsWith(() => b.vcLoadRows(h, I1, F1, C2, V1, new Uint32Array(2)), RangeError, "bmx: keysets must hold one word per row");

  const A = vcRows(base, 65), B = vcRows(base + 65, 65);
  const pA = b.vcMergeBatchAsync(h, A.id, A.field, A.clocks, A.val);
  assert.ok(pA instanceof Promise);
  assert.ok(b.vcGetRows(h, A.id, A.field).state.every((s) => s !== b.VC_ABSENT), "a read issued after A sees A");
  const pB = b.vcMergeBatchAsync(h, B.id, B.field, B.clocks, B.val);
  assert.strictEqual(b.vcDestroy(h), undefined);
  throwsWith(() => b.vcMergeBatchAsync(h, B.id, B.field, B.clocks, B.val), Error, CLOSED.vc);
  updated(await pA, 65, nRows + 65, true, "vc async A"); updated(await pB, 65, nRows + 130, true, "vc async B");
  refusedByAll("vc", h, "a closed handle");
  assert.strictEqual(b.vcDestroy(h), undefined);
  checks += 4;
}

/* a live handle of another kind is refused like a closed one, and is none the worse for it */
function wrongKindContract() {
  const live = { engine: b.create(0, CAP), vc: b.vcCreate(0, CAP, 2, 0), comm: b.commCreate([0], CAP) };
  const count = { engine: b.rowCount, vc: b.vcRowCount, comm: b.commRowCount };
  for (const kind of Object.keys(CALLS)) for (const other of Object.keys(live)) {
    if (other === kind) continue;
    refusedByAll(kind, live[other], "a live " + other + " handle");
    assert.strictEqual(b[DESTROY[kind]](live[other]), undefined);
    isCount(count[other](live[other]), 0, other + " after " + kind + " calls");
  }
  for (const kind of Object.keys(live)) b[DESTROY[kind]](live[kind]);
}

async function gpu() {
  await tableContract("engine", () => b.create(0, CAP), "engine");
  await vcContract();
  await tableContract("comm", () => b.commCreate([0], CAP), "comm of 1 shard");
  await tableContract("comm", () => b.commCreate([0, 0], CAP), "comm of 2 shards");
  if (wrongKind) wrongKindContract();
  console.log(wrongKind ? "addon_contract gpu: handles of another kind checked" : "addon_contract gpu: handles of another kind NOT checked");
}

(async () => {
  if (mode === "host") host();
  else if (mode === "gpu") await gpu();
  else throw new Error("usage: addon_contract.js host | gpu [--no-wrong-kind] [--addon=PATH]");
  console.log("addon_contract ok (" + mode + ", " + checks + " checks)");
})().catch((e) => { console.error(e); process.exit(1); });
