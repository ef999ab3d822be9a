"use strict";
/*
 * query_where_agg.js — test of GpuQuery.whereAggregate / whereTop and DeviceGraph.whereAggregate / whereTop over the N-API addon (include/bmx_where_agg.h):
 * aggregates and ordered pages over boolean filters against filter(path, fn) followed by a reduce / a sort written out by hand — Example 8 of docs/querying.md
 * grouped by role codes ("count users by role among the active non-admins"), an OR of two equalities paged by name and by age.
 * The order of a page is by the value of `over`, then by the 64-bit hash of the path (js/hash.js pathId), as top() orders.
 * Usage: node query_where_agg.js <golden dir> [host]      "host": only the indexes that live on the host — needs no GPU
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

const b = new MiniBullet("wa");
let query;
if (HOST_ONLY) {   // no device behind the facade: every write is applied as it comes
  b.crt = { handleUpdate: (p, data) => ({ doUpdate: true, value: data, vectorClock: {} }) };
  query = new GpuQuery(b);
}
else ({ query } = require("..").attach(b, { capacityRows: 1 << 16 }));

const hashOf = (p) => { const [l, h] = pathId(p); return (BigInt(h) << 32n) | BigInt(l); };

/* filter(path, fn) + sort by (over, hash of the path), by hand */
function sorted(coll, fn, over, desc) {
  const rows = query.filter(coll, fn).map((n) => ({ path: n.path, v: b._getData(n.path)[over], id: hashOf(n.path) }));
  const cmp = (x, y) => (x < y ? -1 : x > y ? 1 : 0);
  rows.sort((x, y) => (desc ? cmp(y.v, x.v) : cmp(x.v, y.v)) || cmp(x.id, y.id));
  return rows;
}

/* whereTop paged with k against the hand-written order: the pages concatenate to it, nEligible falls by the page length, the cursor is the last record */
function paged(coll, clauses, over, fn, k, kind, what) {
  for (const desc of [false, true]) {
    const want = sorted(coll, fn, over, desc);
    let after = null, left = want.length;
    const got = [];
    for (;;) {
      const page = query.whereTop(coll, clauses, k, { over, desc, after });
      assert.strictEqual(query.lastPath, kind, what);
      assert.strictEqual(page.nEligible, left, what + " nEligible");
      if (page.length === 0) { assert.strictEqual(page.cursor, null); break; }
      assert.ok(page.length <= k);
      page.forEach((n, i) => got.push({ path: n.path, v: page.values[i] }));
      assert.strictEqual(BigInt(page.cursor[0]), hashOf(page[page.length - 1].path), what + " cursor id");
      assert.strictEqual(page.cursor[1], page.values[page.length - 1], what + " cursor value");
      left -= page.length; after = page.cursor;
    }
    assert.deepStrictEqual(got, want.map((r) => ({ path: r.path, v: r.v })), what + (desc ? " (desc)" : " (asc)"));
    checks++;
  }
}

/* ---- the reference's users: name / role are strings, active a boolean — host indexes; whereTop evaluates in JS ---- */
const users = JSON.parse(JSON.stringify(g.users));
users.user11 = { name: "Kim Nolan", age: 22, active: true };                        // no role at all
users.user12 = { name: "Lee Ortiz", age: 27, active: true, role: "admin" };
users.user13 = { name: "Lee Ortiz", age: 27, active: false, role: "editor" };       // a tie on name and on age: the hash of the path decides
for (const [k, v] of Object.entries(users)) b.get("users/" + k).put(v);

const ex8 = [[{ field: "active", eq: true }, { field: "age", max: 29 }, { field: "role", ne: "admin" }]];
const ex8fn = (u) => u.active === true && u.age < 30 && u.role !== "admin";
paged("users", ex8, "name", ex8fn, 2, "host", "example 8 by name");
assert.ok(sorted("users", ex8fn, "name", false).some((r) => r.path === "users/user11"), "a child without the field passes the negation");
const or2 = [[{ field: "role", eq: "admin" }], [{ field: "role", eq: "editor" }]];
const or2fn = (u) => u.role === "admin" || u.role === "editor";
paged("users", or2, "name", or2fn, 1, "host", "or by name, one per page");
paged("users", or2, "name", or2fn, 100, "host", "or by name, one page");
assert.ok(sorted("users", or2fn, "name", false).filter((r) => r.v === "Lee Ortiz").length === 2, "the tie is in the selection");
{ // a cursor that names no row
  const want = sorted("users", or2fn, "name", false).filter((r) => r.v > "Lee Ortiz" || (r.v === "Lee Ortiz" && r.id > 5n));
  const page = query.whereTop("users", or2, 100, { over: "name", after: [5n, "Lee Ortiz"] });
  assert.deepStrictEqual(page.map((n) => n.path), want.map((r) => r.path));
  assert.strictEqual(page.nEligible, want.length);
  assert.ok(want.length >= 2);
  checks++;
}
{ const none = query.whereTop("users", [], 5, { over: "age" }); assert.deepStrictEqual(Array.from(none), []); assert.strictEqual(none.cursor, null); assert.strictEqual(none.nEligible, 0); }
assert.throws(() => query.whereTop("users", or2, 5), TypeError);
assert.throws(() => query.whereAggregate("users", or2, {}), TypeError);
// an aggregate needs the device: a literal on a host index is refused like aggregateWhere refuses it
assert.throws(() => query.whereAggregate("users", or2, { over: "name", field: "age" }), (e) => e.code === "BMX_NOT_DEVICE_INDEX");
checks += 3;

/* ---- an integer-coded collection: every index lives on the device ---- */
if (!HOST_ONLY) {
  // an integer index as `over` with literals on host indexes: the host evaluates, ordered by age
  paged("users", or2, "age", or2fn, 2, "host", "host literals over an integer index");
  paged("users", ex8, "age", ex8fn, 100, "host", "example 8 by age");
  const people = {};
  for (let i = 0; i < 900; i++) {
    const p = { age: 18 + (i * 7) % 50, active: i % 3 === 0 ? 0 : 1, seq: i, score: (i * 37) % 1000 - 300 };
    if (i % 5 !== 1) p.role = (i * 3) % 4;            // 0 = admin; every code occurs; a fifth has no role
    if (i % 10 === 3) delete p.score;                 // a tenth has no score
    people["p" + i] = p;
  }
  for (const [k, v] of Object.entries(people)) b.get("people/" + k).put(v);
  const reduce = (fn, field) => {
    const sel = query.filter("people", fn).map((n) => b._getData(n.path));
    const vals = field ? sel.map((u) => u[field]).filter((x) => x !== undefined) : [];
    return { matched: sel.length, count: field ? vals.length : sel.length, sum: vals.reduce((a, x) => a + x, 0), min: vals.length ? Math.min(...vals) : null, max: vals.length ? Math.max(...vals) : null };
  };
  // Example 8's shape with role codes: active && age < 30 && role !== admin
  const e8 = [[{ field: "active", eq: 1 }, { field: "age", max: 29 }, { field: "role", ne: 0 }]];
  const e8fn = (u) => u.active === 1 && u.age < 30 && u.role !== 0;
  for (const field of [undefined, "score", "age", "seq"]) {
    assert.deepStrictEqual(query.whereAggregate("people", e8, { over: "seq", field }), reduce(e8fn, field), "example 8, measure " + field);
    assert.strictEqual(query.lastPath, "device");
    checks++;
  }
  // "count users by role among the active non-admins": grouped by role; the children without a role are in no group
  const byRole = query.whereAggregate("people", e8, { over: "seq", field: "score", groupBy: { field: "role", min: 0, max: 3 } });
  assert.ok(byRole instanceof Map && !byRole.has(0) && byRole.size === 3);
  for (const [role, rec] of byRole) assert.deepStrictEqual(rec, reduce((u) => e8fn(u) && u.role === role, "score"), "role " + role);
  let grouped = 0; for (const rec of byRole.values()) grouped += rec.matched;
  assert.strictEqual(grouped, reduce((u) => e8fn(u) && u.role !== undefined).matched);
  assert.ok(grouped < reduce(e8fn).matched, "children without a role match and are in no group");
  // a window wider than 65536 values, and one that holds nothing
  const wide = query.whereAggregate("people", e8, { over: "seq", groupBy: { field: "seq", min: -70000, max: 70000 } });
  assert.strictEqual(wide.size, reduce(e8fn).matched);
  assert.strictEqual(query.whereAggregate("people", e8, { over: "seq", groupBy: { field: "role", min: 10, max: 20 } }).size, 0);
  checks += 3;
  // "total ... in electronics OR computers": an OR of two equalities, a field no child carries, nothing left
  const orr = [[{ field: "role", eq: 1 }], [{ field: "role", eq: 3 }, { field: "nobody", not: true }]];
  assert.deepStrictEqual(query.whereAggregate("people", orr, { over: "seq", field: "score" }), reduce((u) => u.role === 1 || u.role === 3, "score"));
  assert.deepStrictEqual(query.whereAggregate("people", [[{ field: "nobody", eq: 3 }]], { over: "seq", field: "score" }), { matched: 0, count: 0, sum: 0, min: null, max: null });
  assert.deepStrictEqual(query.whereAggregate("people", [], { over: "seq" }), { matched: 0, count: 0, sum: 0, min: null, max: null });
  assert.strictEqual(query.whereAggregate("people", [[{ field: "nobody", eq: 3 }]], { over: "seq", groupBy: { field: "role", min: 0, max: 3 } }).size, 0);
  checks += 4;
  // the OR paged by age on the device; the 20 youngest who are not admins
  paged("people", [[{ field: "role", eq: 1 }], [{ field: "role", eq: 3 }]], "age", (u) => u.role === 1 || u.role === 3, 64, "device", "or by age on the device");
  paged("people", [[{ field: "role", ne: 0 }, { field: "score", min: 600 }]], "age", (u) => u.role !== 0 && u.score !== undefined && u.score >= 600, 20, "device", "not admins by age");
  {
    const young = query.whereTop("people", [[{ field: "role", ne: 0 }]], 20, { over: "age" });
    assert.deepStrictEqual(young.map((n) => n.path), sorted("people", (u) => u.role !== 0, "age", false).slice(0, 20).map((r) => r.path));
    assert.strictEqual(young.nEligible, reduce((u) => u.role !== 0).matched);
    assert.strictEqual(query.whereTop("people", [[{ field: "nobody", eq: 1 }]], 20, { over: "age" }).nEligible, 0);
    checks += 2;
  }
  /* a write is seen by the next query */
  b.get("people/p2").put(Object.assign({}, people.p2, { role: 0 })); people.p2.role = 0;
  assert.deepStrictEqual(query.whereAggregate("people", e8, { over: "seq", field: "score" }), reduce(e8fn, "score"), "after a write");
  /* DeviceGraph.whereAggregate / whereTop themselves */
  const ixSeq = query.indices["people:seq"], ixAge = query.indices["people:age"], ixRole = query.indices["people:role"];
  const prog = [[[ixAge.deviceField, 18, 18]], [[ixRole.deviceField, 0, 0, true], [ixSeq.deviceField, -Infinity, 9]]];
  const fn = (u) => u.age === 18 || (u.role !== 0 && u.seq <= 9);
  const r = query.graph.whereAggregate(ixSeq.deviceField, prog, { measure: ixAge.deviceField });
  assert.deepStrictEqual({ matched: r.nMatch, count: r.n, sum: r.sum, min: r.min, max: r.max }, reduce(fn, "age"));
  const recs = query.graph.whereAggregate(ixSeq.deviceField, prog, { group: ixRole.deviceField, groupLo: 0, nGroups: 4 });
  assert.strictEqual(recs.length, 5);
  assert.strictEqual(recs[4].nMatch, reduce((u) => fn(u) && u.role === undefined).matched);
  const t = query.graph.whereTop(ixSeq.deviceField, prog, 7, { desc: true });
  assert.ok(t.ids instanceof BigUint64Array && t.vals instanceof BigInt64Array && t.ids.length === 7 && t.nEligible === reduce(fn).matched);
  assert.deepStrictEqual(Array.from(t.vals, Number), sorted("people", fn, "seq", true).slice(0, 7).map((x) => x.v));
  assert.throws(() => query.graph.whereAggregate(ixSeq.deviceField, []), RangeError);
  assert.throws(() => query.graph.whereTop(ixSeq.deviceField, prog, 0), RangeError);
  assert.throws(() => query.graph.whereTop(ixSeq.deviceField, prog, 4097), RangeError);
  assert.throws(() => query.graph.whereAggregate(ixSeq.deviceField, prog, { nGroups: 4 }), RangeError);
  checks += 4;
}

if (b.close) b.close();
else query.close();
console.log("query_where_agg ok: " + checks + " checks" + (HOST_ONLY ? " (host indexes only)" : ""));
