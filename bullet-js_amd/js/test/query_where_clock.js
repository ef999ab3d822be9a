"use strict";
/*
 * query_where_clock.js — test of the {field, clock: "data" | "deleted" | "any", ...} term of GpuQuery.where / whereAggregate / whereTop / whereRows
 * (include/bmx_where.h BMX_LIT_CLOCK / BMX_LIT_CLOCK_TOMB): a range over the clock of the field's row in its index. Each form is held against a host filter
 * over the clocks and states that whereRows reports with {clocks: true}, on the reference's example products (tests/golden/g5_query_example.json) with
 * children that lack a field, before and after writes that patch the device indexes (a patched row's clock moves on).
 * Usage: node query_where_clock.js <golden dir> [host]      "host": only the host evaluation (over: a string field) — needs no GPU
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
for (const [k, v] of Object.entries(products)) b.get("products/" + k).put(v);

/* the terms; `in` says what the clock of a row that exists in a named state has to satisfy */
const TERMS = [
  ["stock has a row", { field: "stock", clock: "data" }, () => true],
  ["stock changed since the build", { field: "stock", clock: "data", min: 2 }, (c) => c >= 2],
  ["stock as built", { field: "stock", clock: "data", eq: 1 }, (c) => c === 1],
  ["stock not as built", { field: "stock", clock: "data", ne: 1 }, (c) => c === 1, true],
  ["stock in any state, clocks 1..2", { field: "stock", clock: "any", min: 1, max: 2 }, (c) => c >= 1 && c <= 2],
  ["stock not changed since the build", { field: "stock", clock: "data", min: 2, not: true }, (c) => c >= 2, true],
  ["stock deleted", { field: "stock", clock: "deleted" }, () => true],
  ["stock not deleted", { field: "stock", clock: "deleted", not: true }, () => true, true],
  ["an empty window", { field: "stock", clock: "any", min: 3, max: 2 }, () => false],
  ["a field no child carries", { field: "nobody", clock: "any" }, () => true],
  ["... negated", { field: "nobody", clock: "any", not: true }, () => true, true],
];
/* the truth of a term from what whereRows reported: the state of a row is "data" when it has a clock and a value, "deleted" when it has a clock and none */
function truth(t, inside, neg, row, ck) {
  const c = ck[t.field];
  const state = c === undefined ? null : row[t.field] === undefined ? "deleted" : "data";
  const pos = state !== null && (t.clock === "any" || t.clock === state) && inside(c);
  return pos !== !!neg;
}

function run(over, kind, stage) {
  // every candidate with the clocks and states of the fields the terms name
  const every = query.whereRows("products", [[{ field: over }]], ["stock", "nobody", over], { over, clocks: true });
  assert.strictEqual(query.lastPath, kind, stage);
  assert.strictEqual(every.paths.length, Object.values(products).filter((p) => p[over] !== undefined && p[over] !== null).length, stage);
  every.paths.forEach((p, i) => {
    const c = products[p.slice(9)];
    assert.strictEqual(every.rows[i].stock, c.stock, p);
    assert.strictEqual(every.clocks[i].stock === undefined, c.stock === undefined, p + " has a clock where it has a row");
    assert.strictEqual(every.clocks[i].nobody, undefined);
  });
  for (const [what, term, inside, neg] of TERMS) {
    for (const clauses of [[[term]], [[term, { field: over }]], [[{ field: "stock", min: 1 }, term]], [[term], [{ field: "stock", not: true }]]]) {
      const lit = (t, i) => (t === term ? truth(term, inside, neg, every.rows[i], every.clocks[i]) : (every.rows[i][t.field] !== undefined && (t.min === undefined || every.rows[i][t.field] >= t.min)) !== !!t.not);
      const sel = every.paths.map((p, i) => i).filter((i) => clauses.some((c) => c.every((t) => lit(t, i))));
      const want = sel.map((i) => every.paths[i]).sort();
      const tag = stage + ": " + what + " " + JSON.stringify(clauses);
      const got = query.where("products", clauses, { over }).map((n) => n.path);
      assert.strictEqual(query.lastPath, kind, tag);
      assert.deepStrictEqual(got.slice().sort(), want, tag + " (where)");
      const r = query.whereRows("products", clauses, ["stock"], { over, clocks: true });
      assert.deepStrictEqual(r.paths.slice().sort(), want, tag + " (whereRows)");
      assert.strictEqual(r.nMatch, want.length);
      r.paths.forEach((p, i) => { const k = every.paths.indexOf(p); assert.deepStrictEqual([r.rows[i].stock, r.clocks[i].stock], [every.rows[k].stock, every.clocks[k].stock], tag + " " + p); });
      const top = query.whereTop("products", clauses, 100, { over });
      assert.deepStrictEqual(Array.from(top).map((n) => n.path).sort(), want, tag + " (whereTop)");
      if (kind === "device") {
        const st = sel.map((i) => every.rows[i].stock).filter((x) => x !== undefined);
        const a = query.whereAggregate("products", clauses, { over, field: "stock" });
        assert.deepStrictEqual(a, { matched: sel.length, count: st.length, sum: st.reduce((x, y) => x + y, 0), min: st.length ? Math.min(...st) : null, max: st.length ? Math.max(...st) : null }, tag + " (whereAggregate)");
      } else {
        assert.throws(() => query.whereAggregate("products", clauses, { over, field: "stock" }), (e) => e.code === "BMX_NOT_DEVICE_INDEX");
      }
      checks += 4;
    }
  }
  return every;
}

function stages(over, kind, built) {      // built: no write has patched the indexes since they were built
  const first = run(over, kind, (built ? "as built" : "before a further write") + ", over " + over);
  if (built) assert.ok(first.clocks.every((c) => c.stock === undefined || c.stock === 1), "every row of a build has clock 1");
  // writes that change values: a device index is patched, and the rows it rewrote carry the patch's clock
  products.prod1.stock += 7; b.get("products/prod1").put(products.prod1);
  products.prod3.stock += 1; b.get("products/prod3").put(products.prod3);
  const patches = query.stats.patches;
  const second = run(over, kind, "after a write, over " + over);
  if (kind === "device" && query.stats.patches > patches) {
    const moved = second.paths.filter((p, i) => second.clocks[i].stock >= 2).sort();
    assert.deepStrictEqual(moved, ["products/prod1", "products/prod3"].filter((p) => second.paths.includes(p)), "the patched rows moved on");
    checks++;
  }
}

stages("name", "host", true);
assert.throws(() => query.where("products", [[{ field: "stock", clock: "sometimes" }]], { over: "name" }), RangeError);
assert.throws(() => query.where("products", [[{ field: "stock", clock: "data", minus: "price" }]], { over: "name" }), RangeError);
checks += 2;
if (!HOST_ONLY) {
  stages("price", "device", true);
  stages("stock", "device", false);       // the term on the field that defines the universe: the base field's own row
  /* DeviceGraph.scanWhere itself: the sixth entry of a literal, and tombstones, which only rows written to the table directly have */
  const ixP = query.indices["products:price"], ixS = query.indices["products:stock"];
  const nBoth = Object.values(products).filter((p) => p.price !== undefined && p.stock !== undefined).length;
  assert.strictEqual(query.graph.scanWhere(ixP.deviceField, [[[ixS.deviceField, -Infinity, Infinity, false, null, 3]]]).length, nBoth);
  assert.strictEqual(query.graph.scanWhere(ixP.deviceField, [[[ixS.deviceField, -Infinity, Infinity, false, null, 2]]]).length, 0);
  assert.strictEqual(query.graph.scanWhere(ixP.deviceField, [[[ixS.deviceField, -Infinity, Infinity, true, null, 1]]]).length, Object.values(products).filter((p) => p.price !== undefined).length - nBoth);
  assert.throws(() => query.graph.scanWhere(ixP.deviceField, [[[ixS.deviceField, 0, 0, false, null, 4]]]), RangeError);
  assert.throws(() => query.graph.scanWhere(ixP.deviceField, [[[ixS.deviceField, 0, 0, false, ixP.deviceField, 1]]]), /clock literal/);
  checks += 5;
}

if (b.close) b.close();
else query.close();
console.log("query_where_clock ok: " + checks + " checks" + (HOST_ONLY ? " (host indexes only)" : ""));
