"use strict";
/*
 * query_aggregate.js — GPU test of GpuQuery.countBy / aggregateWhere and DeviceGraph.scanAggregate over the N-API addon (include/bmx.h "aggregate queries")
 * on the reference's example dataset (tests/golden/g5_query_example.json): per-value counts against the fixture's equals / range answers, sum / min / max
 * against a plain reduce over the fixture's objects, a sum beyond 2^53 as a BigInt. Needs an MI355X.
 * Usage: node query_aggregate.js <golden dir>
 */
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const { attach } = require("..");
const MiniBullet = require("./mini-bullet");

const GOLD = process.argv[2] || path.join(__dirname, "..", "..", "..", "tests", "golden");
const g = JSON.parse(fs.readFileSync(path.join(GOLD, "g5_query_example.json"), "utf8"));
let checks = 0;

const b = new MiniBullet("w");
const { query } = attach(b, { capacityRows: 4096 });
for (const [k, v] of Object.entries(g.users)) b.get("users/" + k).put(v);
for (const [k, v] of Object.entries(g.products)) b.get("products/" + k).put(v);

/* countBy against the keys the reference's equals / range queries on users.age return */
const byAge = query.countBy("users", "age", 0, 1000);
assert.ok(byAge instanceof Map);
assert.strictEqual(query.lastPath, "device");
const ages = Object.values(g.users).map((u) => u.age);
assert.strictEqual(byAge.size, new Set(ages).size, "only the values that occur");
for (const q of g.queries) {
  if (q.args[0] !== "users" || q.args[1] !== "age") continue;
  if (q.op === "equals") {
    assert.strictEqual(byAge.get(Number(q.args[2])) || 0, q.keys.length, JSON.stringify(q.args));
    checks++;
  } else if (q.op === "range") {
    let n = 0;
    for (const [v, c] of byAge) if (v >= q.args[2] && v <= q.args[3]) n += c;
    assert.strictEqual(n, q.keys.length, JSON.stringify(q.args));
    const part = query.countBy("users", "age", q.args[2], q.args[3]);
    assert.strictEqual([...part.values()].reduce((s, x) => s + x, 0), q.keys.length);
    checks += 2;
  } else if (q.op === "count") {
    assert.strictEqual(byAge.get(q.args[2]) || 0, q.n);
    checks++;
  }
}
assert.ok(checks >= 6);
for (const [v, c] of byAge) assert.strictEqual(c, ages.filter((a) => a === v).length);

/* aggregateWhere against a plain reduce over the fixture's objects */
function want(objs, pred, field) {
  const sel = objs.filter(pred), vals = sel.filter((o) => Number.isInteger(o[field])).map((o) => o[field]);
  return { matched: sel.length, count: vals.length, sum: vals.reduce((s, x) => s + x, 0), min: vals.length ? Math.min(...vals) : null, max: vals.length ? Math.max(...vals) : null };
}
const products = Object.values(g.products);
assert.deepStrictEqual(query.aggregateWhere("products", [{ field: "price", min: 0, max: 1e6 }], "stock"), want(products, (p) => p.price >= 0 && p.price <= 1e6, "stock"));
assert.strictEqual(query.lastPath, "device");
assert.deepStrictEqual(query.aggregateWhere("products", [{ field: "price", min: 200, max: 1e6 }, { field: "stock", min: 0, max: 12 }], "price"),
                       want(products, (p) => p.price >= 200 && p.stock <= 12, "price"));
assert.deepStrictEqual(query.aggregateWhere("products", [{ field: "price", min: 5, max: 4 }], "stock"), { matched: 0, count: 0, sum: 0, min: null, max: null });
assert.deepStrictEqual(query.aggregateWhere("users", [{ field: "age", min: 30, max: 40 }]), { matched: want(Object.values(g.users), (u) => u.age >= 30 && u.age <= 40, "age").matched, count: want(Object.values(g.users), (u) => u.age >= 30 && u.age <= 40, "age").matched, sum: 0, min: null, max: null });
checks += 4;

/* a string field is no device index: both throw exactly where filterWhere does */
for (const f of [() => query.aggregateWhere("users", [{ field: "role", min: 0, max: 1 }], "age"), () => query.aggregateWhere("users", [{ field: "age", min: 0, max: 99 }], "role"), () => query.countBy("users", "role", 0, 10),
                 () => query.filterWhere("users", [{ field: "role", min: 0, max: 1 }])]) {
  assert.throws(f, (e) => e.code === "BMX_NOT_DEVICE_INDEX");
  checks++;
}

/* a sum beyond 2^53 comes back as a BigInt, exact */
const BIG = Number.MAX_SAFE_INTEGER;
for (let i = 0; i < 5; i++) b.get("big/n" + i).put({ v: i < 4 ? BIG : 7, w: i });
const r = query.aggregateWhere("big", [{ field: "w", min: 0, max: 3 }], "v");
assert.strictEqual(typeof r.sum, "bigint");
assert.strictEqual(r.sum, 4n * BigInt(BIG));
assert.deepStrictEqual([r.matched, r.count, r.min, r.max], [4, 4, BIG, BIG]);
const small = query.aggregateWhere("big", [{ field: "w", min: 4, max: 4 }], "v");
assert.deepStrictEqual(small, { matched: 1, count: 1, sum: 7, min: 7, max: 7 });
checks += 2;

/* the graph's own call: groups + the record of everything outside the window */
const ixAge = query._fresh("users", "age");
const recs = query.graph.scanAggregate([[ixAge.deviceField, 0, 1000]], { measure: ixAge.deviceField, group: ixAge.deviceField, groupLo: 30, nGroups: 11 });
assert.strictEqual(recs.length, 12);
assert.strictEqual(recs.reduce((s, x) => s + x.nMatch, 0), ages.length);
assert.strictEqual(recs[11].nMatch, ages.filter((a) => a < 30 || a > 40).length);
for (let k = 0; k < 11; k++) assert.strictEqual(recs[k].sum, ages.filter((a) => a === 30 + k).reduce((s, x) => s + x, 0));
checks += 3;

b.close();
console.log("query_aggregate ok: " + checks + " checks");
