"use strict";
/*
 * query_where_diff.js — test of the {field, minus: "other", ...} term of GpuQuery.where / whereAggregate / whereTop / whereRows (include/bmx_where.h
 * BMX_LIT_MINUS): a comparison of two fields of the same child, against the reference-style filter(path, fn) callback written out by hand, on the reference's
 * example products (tests/golden/g5_query_example.json: price and stock are integers, name and category strings) with children that lack one side.
 * Usage: node query_where_diff.js <golden dir> [host]      "host": only the host evaluation (over: a string field) — needs no GPU
 */
const fs = require("fs");
const path = require("path");
const assert = require("assert");
const MiniBullet = require("./mini-bullet");
const GpuQuery = require("../gpu-query");

const GOLD = process.argv[2] || path.join(__dirname, "..", "..", "..", "tests", "golden");
const HOST_ONLY = process.argv[3] === "host";
const g = JSON.parse(fs.readFileSync(path.join(GOLD, "g5_query_example.json"), "utf8"));
let checks = 0;

const b = new MiniBullet("d");
let query;
if (HOST_ONLY) {   // no device behind the facade: every write is applied as it comes
  b.crt = { handleUpdate: (p, data) => ({ doUpdate: true, value: data, vectorClock: {} }) };
  query = new GpuQuery(b);
}
else ({ query } = require("..").attach(b, { capacityRows: 1 << 16 }));

const products = JSON.parse(JSON.stringify(g.products));
products.product11 = { name: "Gift card", price: 25, category: "other" };                 // no stock
products.product12 = { name: "Sample", stock: 40, category: "other" };                    // no price
products.product13 = { name: "Cable", price: 9, stock: 9, category: "electronics" };      // equal
products.product14 = { name: "Bulk screws", price: 3, stock: 5000, category: "hardware" };
for (const [k, v] of Object.entries(products)) b.get("products/" + k).put(v);
const all = Object.values(products);

/* the programs and the callbacks they stand for; both sides must be numbers for a comparison to hold, as on the reference (`undefined > x` is false) */
const both = (p) => typeof p.price === "number" && typeof p.stock === "number";
const CASES = [
  ["price > stock", [[{ field: "price", minus: "stock", min: 1 }]], (p) => p.price > p.stock],
  ["price <= stock", [[{ field: "price", minus: "stock", max: 0 }]], (p) => p.price <= p.stock],
  ["price === stock", [[{ field: "price", minus: "stock", eq: 0 }]], (p) => both(p) && p.price === p.stock],
  ["price !== stock", [[{ field: "price", minus: "stock", ne: 0 }]], (p) => !(both(p) && p.price === p.stock)],
  ["!(price > stock)", [[{ field: "price", minus: "stock", min: 1, not: true }]], (p) => !(p.price > p.stock)],
  ["price - stock <= 100", [[{ field: "price", minus: "stock", max: 100 }, { field: "price", min: 10 }]], (p) => p.price - p.stock <= 100 && p.price >= 10],
  ["stock - price in 0..50, or no price", [[{ field: "stock", minus: "price", min: 0, max: 50 }], [{ field: "price", not: true }]], (p) => (p.stock - p.price >= 0 && p.stock - p.price <= 50) || p.price === undefined],
  ["both present", [[{ field: "price", minus: "stock" }]], both],
  ["a side no child carries", [[{ field: "price", minus: "nobody", min: 1 }]], () => false],
  ["... negated", [[{ field: "price", minus: "nobody", min: 1, not: true }, { field: "stock", minus: "price", min: 1 }]], (p) => p.stock > p.price],
];

function run(over, kind) {
  const carry = (p) => p[over] !== undefined;
  for (const [what, clauses, fn] of CASES) {
    const want = query.filter("products", (p) => carry(p) && fn(p)).map((n) => n.path).sort();
    assert.deepStrictEqual(want, Object.keys(products).filter((k) => carry(products[k]) && fn(products[k])).map((k) => "products/" + k).sort(), what);
    // where
    const got = query.where("products", clauses, { over }).map((n) => n.path);
    assert.strictEqual(query.lastPath, kind, what);
    assert.deepStrictEqual(got.slice().sort(), want, what + " (where, over " + over + ")");
    // whereRows: the same children, each with both sides
    const r = query.whereRows("products", clauses, ["price", "stock"], { over });
    assert.strictEqual(query.lastPath, kind, what);
    assert.deepStrictEqual(r.paths.slice().sort(), want, what + " (whereRows)");
    assert.strictEqual(r.nMatch, want.length);
    r.paths.forEach((p, i) => { const c = products[p.slice(9)]; assert.deepStrictEqual(r.rows[i], { price: c.price, stock: c.stock }, what + " " + p); });
    // whereTop: all of them, ordered by `over`
    const top = query.whereTop("products", clauses, 100, { over });
    assert.strictEqual(query.lastPath, kind, what);
    assert.deepStrictEqual(Array.from(top).map((n) => n.path).sort(), want, what + " (whereTop)");
    const vals = Array.from(top).map((n) => products[n.path.slice(9)][over]);
    assert.deepStrictEqual(vals, vals.slice().sort((x, y) => (x < y ? -1 : x > y ? 1 : 0)), what + " (whereTop order)");
    // whereAggregate: the device's alone
    if (kind === "device") {
      const sel = all.filter((p) => carry(p) && fn(p));
      const st = sel.filter((p) => p.stock !== undefined).map((p) => p.stock);
      const a = query.whereAggregate("products", clauses, { over, field: "stock" });
      assert.deepStrictEqual(a, { matched: sel.length, count: st.length, sum: st.reduce((x, y) => x + y, 0), min: st.length ? Math.min(...st) : null, max: st.length ? Math.max(...st) : null }, what + " (whereAggregate)");
    } else {
      assert.throws(() => query.whereAggregate("products", clauses, { over, field: "stock" }), (e) => e.code === "BMX_NOT_DEVICE_INDEX");
    }
    checks += 4;
  }
}

run("name", "host");
assert.throws(() => query.where("products", [[{ field: "price", minus: "price", eq: 0 }]], { over: "name" }), RangeError);
checks++;
if (!HOST_ONLY) {
  run("price", "device");          // A is the column value
  run("stock", "device");          // B is
  /* DeviceGraph.scanWhere itself: the fifth entry of a literal */
  const ixP = query.indices["products:price"], ixS = query.indices["products:stock"];
  const ids = query.graph.scanWhere(ixP.deviceField, [[[ixP.deviceField, 1, Infinity, false, ixS.deviceField]]]);
  assert.ok(ids instanceof BigUint64Array);
  assert.strictEqual(ids.length, all.filter((p) => p.price > p.stock).length);
  assert.throws(() => query.graph.scanWhere(ixP.deviceField, [new Array(5).fill([ixP.deviceField, 0, 0, false, ixS.deviceField])]), RangeError);      // 10 entries in a clause
  assert.throws(() => query.graph.scanWhere(ixP.deviceField, [[[ixP.deviceField, 0, 0, false, ixP.deviceField]]]), /minus itself/);
  checks += 3;
}

if (b.close) b.close();
else query.close();
console.log("query_where_diff ok: " + checks + " checks" + (HOST_ONLY ? " (host indexes only)" : ""));
