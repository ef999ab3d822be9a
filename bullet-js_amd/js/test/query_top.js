"use strict";
/*
 * query_top.js — test of GpuQuery.top and DeviceGraph.scanTop over the N-API addon (include/bmx_top.h) on the reference's example dataset
 * (tests/golden/g5_query_example.json) and on a larger collection with heavy ties: every page against a plain sort of the fixture's objects by
 * (value, 64-bit path hash), cursors, descending order, bounds and further terms.
 * Usage: node query_top.js <golden dir> [host]      "host": only the indexes that live on the host (non-integer values) — needs no GPU
 */
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const MiniBullet = require("./mini-bullet");
const GpuQuery = require("../gpu-query");
const { pathId } = require("../hash");

const GOLD = process.argv[2] || path.join(__dirname, "..", "..", "..", "tests", "golden");
const HOST_ONLY = process.argv[3] === "host";
const g = JSON.parse(fs.readFileSync(path.join(GOLD, "g5_query_example.json"), "utf8"));
let checks = 0;

const idOf = (p) => { const [l, h] = pathId(p); return (BigInt(h) << 32n) | BigInt(l); };
const cmpVal = (a, b) => {
  const na = typeof a === "number", nb = typeof b === "number";
  if (na && nb) return a < b ? -1 : a > b ? 1 : 0;
  if (na !== nb) return na ? -1 : 1;
  return String(a) < String(b) ? -1 : String(a) > String(b) ? 1 : 0;
};
/* the model: children of `coll` that carry `field` and pass `pred`, sorted by (value, path hash) */
function model(objs, coll, field, pred, desc) {
  const rows = Object.entries(objs).filter(([, o]) => o[field] !== undefined && o[field] !== null && pred(o)).map(([k, o]) => ({ key: k, v: o[field], id: idOf(coll + "/" + k) }));
  rows.sort((a, b) => (desc ? cmpVal(b.v, a.v) : cmpVal(a.v, b.v)) || (a.id < b.id ? -1 : a.id > b.id ? 1 : 0));
  return rows;
}
/* every page of size k, each behind the cursor of the one before, against the model */
function walk(query, b, objs, coll, field, k, opts, pred, kind) {
  const want = model(objs, coll, field, pred, !!opts.desc);
  let after = null, at = 0;
  for (;;) {
    const page = query.top(coll, field, k, Object.assign({}, opts, { after }));
    assert.strictEqual(query.lastPath, kind);
    assert.strictEqual(page.nEligible, want.length - at, `${coll}.${field} page at ${at}`);
    assert.strictEqual(page.length, Math.min(k, want.length - at));
    for (let i = 0; i < page.length; i++) {
      assert.strictEqual(page[i].path, coll + "/" + want[at + i].key, `${coll}.${field} record ${at + i}`);
      assert.strictEqual(page.values[i], want[at + i].v);
    }
    checks++;
    if (!page.length) { assert.strictEqual(page.cursor, null); break; }
    assert.strictEqual(BigInt(page.cursor[0]), want[at + page.length - 1].id);
    at += page.length; after = page.cursor;
  }
  assert.strictEqual(at, want.length);
}

const b = new MiniBullet("w");
let query;
if (HOST_ONLY) {   // no device behind the facade: every write is applied as it comes
  b.crt = { handleUpdate: (p, data) => ({ doUpdate: true, value: data, vectorClock: {} }) };
  query = new GpuQuery(b);
}
else ({ query } = require("..").attach(b, { capacityRows: 1 << 16 }));
for (const [k, v] of Object.entries(g.users)) b.get("users/" + k).put(v);
for (const [k, v] of Object.entries(g.products)) b.get("products/" + k).put(v);
/* a collection with fractional scores (host index) and few distinct integer ranks (device index): ties decided by the path hash */
const big = {};
for (let i = 0; i < 700; i++) big["n" + i] = { score: ((i * 37) % 11) / 4, rank: (i * 7) % 5, w: i % 3 };
for (const [k, v] of Object.entries(big)) b.get("big/" + k).put(v);

/* ---- indexes that live on the host: strings, fractions ---- */
const all = () => true;
for (const desc of [false, true]) {
  walk(query, b, g.users, "users", "name", 3, { desc }, all, "host");
  walk(query, b, g.users, "users", "role", 4, { desc }, all, "host");
  walk(query, b, g.products, "products", "category", 100, { desc }, all, "host");
  walk(query, b, big, "big", "score", 64, { desc }, all, "host");
  walk(query, b, big, "big", "score", 33, { desc, min: 0.5, max: 2 }, (o) => o.score >= 0.5 && o.score <= 2, "host");
  walk(query, b, big, "big", "score", 50, { desc, where: [{ field: "w", min: 1, max: 1 }] }, (o) => o.w === 1, "host");
}
assert.strictEqual(query.top("users", "name", 5, { min: "zzzz" }).length, 0);
assert.strictEqual(query.top("nothing", "here", 5).length, 0);

/* ---- integer indexes: on the device ---- */
if (!HOST_ONLY) {
  for (const desc of [false, true]) {
    walk(query, b, g.users, "users", "age", 3, { desc }, all, "device");
    walk(query, b, g.products, "products", "price", 4, { desc, min: 100, max: 1000 }, (p) => p.price >= 100 && p.price <= 1000, "device");
    walk(query, b, g.products, "products", "price", 2, { desc, where: [{ field: "stock", min: 0, max: 30 }] }, (p) => p.stock <= 30, "device");
    walk(query, b, big, "big", "rank", 97, { desc }, all, "device");
    walk(query, b, big, "big", "rank", 4096, { desc, min: 1, max: 3, where: [{ field: "w", min: 0, max: 1 }] }, (o) => o.rank >= 1 && o.rank <= 3 && o.w <= 1, "device");
  }
  assert.strictEqual(query.top("products", "price", 5, { min: 5, max: 4 }).length, 0);
  assert.throws(() => query.top("users", "age", 5, { where: [{ field: "role", min: 0, max: 1 }] }), (e) => e.code === "BMX_NOT_DEVICE_INDEX");
  assert.throws(() => query.top("users", "age", 0), RangeError);
  assert.throws(() => query.top("users", "age", 4097), RangeError);
  /* DeviceGraph.scanTop itself: ids and values as typed arrays, the count of eligible nodes */
  const ixRank = query.indices["big:rank"];
  const r = query.graph.scanTop([[ixRank.deviceField, 0, 4]], 10, { desc: true });
  assert.ok(r.ids instanceof BigUint64Array && r.vals instanceof BigInt64Array && r.ids.length === 10 && r.nEligible === 700);
  assert.deepStrictEqual(Array.from(r.vals, Number), new Array(10).fill(4));
  checks++;
}

if (b.close) b.close();
else query.close();
console.log("query_top ok: " + checks + " checks" + (HOST_ONLY ? " (host indexes only)" : ""));
