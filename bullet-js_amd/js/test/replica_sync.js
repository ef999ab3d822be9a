"use strict";
/*
 * replica_sync.js — GPU test of DeviceGraph.digest / exportRows over the N-API addon (include/bmx.h "replica reconciliation"): digest totals against the
 * rowDigest sum of dumpRows(), the rows one graph exports merged into another through the graph's own batch merge (BMX_INSERT_DELTA), equal digests
 * afterwards; the same over a 4-shard communicator. Needs an MI355X.
 * Usage: node replica_sync.js
 */
const path = require("path");
const assert = require("assert");
const DeviceGraph = require("../device-graph");
const gen = require(path.join(__dirname, "..", "..", "..", "oracle", "gen_golden.js"));   // test infrastructure: key generator and rowDigest only

const M64 = (1n << 64n) - 1n;
const R = 20000, D = 6000;

function cols(n, row, ts, val) {
  const c = { id: new BigUint64Array(n), field: new Uint32Array(n), ts: new BigInt64Array(n), val: new BigInt64Array(n) };
  for (let i = 0; i < n; i++) { const r = row(i); c.id[i] = gen.rowId(r, 1); c.field[i] = gen.rowField(r, 1); c.ts[i] = BigInt(ts(i)); c.val[i] = BigInt(val(i)); }
  return c;
}
const total = (a) => a.reduce((s, x) => (s + x) & M64, 0n);
function dumpDigest(g) {
  const d = g.dumpRows();
  let s = 0n;
  for (let i = 0; i < d.id.length; i++) s = (s + gen.rowDigest(d.id[i], d.field[i], d.ts[i], d.val[i])) & M64;
  return { sum: s, n: d.id.length };
}
function same(a, b) {
  assert.strictEqual(a.sums.length, b.sums.length);
  for (let i = 0; i < a.sums.length; i++) { assert.strictEqual(a.sums[i], b.sums[i], "sums[" + i + "]"); assert.strictEqual(a.counts[i], b.counts[i], "counts[" + i + "]"); }
}

function run(optsA, optsB, label) {
  const a = new DeviceGraph(Object.assign({ capacityRows: 1 << 17 }, optsA)), b = new DeviceGraph(Object.assign({ capacityRows: 1 << 17 }, optsB));
  const DELTA = a.native.INSERT_DELTA;
  const base = cols(R, (i) => i, (i) => 1000 + (i * 7) % 500, (i) => (i * 31) % 1000 - 500);
  a.loadRows(base); b.loadRows(base);
  // a moves on: changed rows and new ones
  a.mergeBatch(cols(D, (i) => (i % 3 === 0 ? R + i : (i * 13) % R), (i) => 2000 + i % 100, (i) => i), DELTA);
  for (const L of [0, 4, 10, 13]) {
    for (const g of [a, b]) {
      const dg = g.digest(L), want = dumpDigest(g);
      assert.ok(dg.sums instanceof BigUint64Array && dg.counts instanceof BigUint64Array && dg.sums.length === (1 << L));
      assert.strictEqual(total(dg.sums), want.sum, label + ": digest total, L = " + L);
      assert.strictEqual(Number(total(dg.counts)), want.n);
    }
  }
  const da = a.digest(10, { tombstones: true }), db = b.digest(10, { tombstones: true });
  const bits = new BigUint64Array(16);
  let differing = 0;
  for (let i = 0; i < 1024; i++) if (da.sums[i] !== db.sums[i] || da.counts[i] !== db.counts[i]) { bits[i >> 6] |= 1n << BigInt(i & 63); differing++; }
  assert.ok(differing > 0);
  const all = a.exportRows(), part = a.exportRows({ log2Buckets: 10, bucketBits: bits }), late = a.exportRows({ since: 2000 });
  assert.strictEqual(all.n, a.rowCount()); assert.ok(part.n <= all.n && part.n > 0); assert.ok(late.n > 0 && late.n < all.n);
  for (let i = 0; i < late.n; i++) assert.ok(late.ts[i] >= 2000n);
  assert.strictEqual(a.exportRows({ onlyTombstones: true }).n, 0);
  b.mergeBatch({ id: part.id, field: part.field, ts: part.ts, val: part.val }, DELTA);
  same(a.digest(10, { tombstones: true }), b.digest(10, { tombstones: true }));
  same(a.digest(13), b.digest(13));
  assert.strictEqual(dumpDigest(a).sum, dumpDigest(b).sum);
  a.close(); b.close();
  console.log("replica_sync " + label + ": " + differing + " buckets differed, " + part.n + " of " + all.n + " rows shipped");
}

run({}, {}, "single context");
run({ shards: 4 }, { shards: 4 }, "4-shard communicator");
run({ shards: 4 }, {}, "communicator -> single context");
console.log("replica_sync ok");
