"use strict";
/*
 * query_where.js — test of GpuQuery.where and DeviceGraph.scanWhere over the N-API addon (include/bmx_where.h): boolean filters against the reference-style
 * filter(path, fn) callback written out by hand — Example 8 of docs/querying.md (a negation that is true for a child without the field), an OR of two
 * equalities, a presence test — on the reference's example dataset (tests/golden/g5_query_example.json; strings and booleans: host indexes) and on an
 * integer-coded collection (device indexes). Every child carries the `over` field, so where() and filter() must agree as sets.
 * Usage: node query_where.js <golden dir> [host]      "host": only the indexes that live on the host — needs no GPU
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

const b = new MiniBullet("w");
let query;
if (HOST_ONLY) {   // no device behind the facade: every write is applied as it comes
  b.crt = { handleUpdate: (p, data) => ({ doUpdate: true, value: data, vectorClock: {} }) };
  query = new GpuQuery(b);
}
else ({ query } = require("..").attach(b, { capacityRows: 1 << 16 }));

/* where() against the callback: the same set of paths, and where()'s own order is the store's */
function same(coll, clauses, over, fn, kind, what) {
  const got = query.where(coll, clauses, { over }).map((n) => n.path);
  assert.strictEqual(query.lastPath, kind, what);
  const want = query.filter(coll, fn).map((n) => n.path);
  assert.deepStrictEqual(got.slice().sort(), want.slice().sort(), what);
  assert.deepStrictEqual(got, want, what + " (order)");
  checks++;
  return got;
}

/* ---- the reference's users: name / role are strings, active a boolean — host indexes; two children lose a field ---- */
const users = JSON.parse(JSON.stringify(g.users));
users.user11 = { name: "Kim Nolan", age: 22, active: true };                        // no role at all
users.user12 = { name: "Lee Ortiz", age: 27, active: true, role: "admin", address: { state: "CA" } };
users.user13 = { name: "Max Perez", age: 51, active: false, role: "editor", address: { state: "NY" } };
for (const [k, v] of Object.entries(users)) b.get("users/" + k).put(v);

// Example 8: user.active === true && user.age < 30 && user.role !== "admin" — true for user11, who has no role
const ex8 = same("users", [[{ field: "active", eq: true }, { field: "age", max: 29 }, { field: "role", ne: "admin" }]], "name",
  (u) => u.active === true && u.age < 30 && u.role !== "admin", "host", "example 8");
assert.ok(ex8.includes("users/user11") && !ex8.includes("users/user12") && ex8.length >= 2);
// an OR of two equalities
const or2 = same("users", [[{ field: "role", eq: "admin" }], [{ field: "role", eq: "editor" }]], "name", (u) => u.role === "admin" || u.role === "editor", "host", "or");
assert.ok(or2.length >= 3 && or2.length < Object.keys(users).length);
// presence: user.address && user.age > 40
const pres = same("users", [[{ field: "address" }, { field: "age", min: 41 }]], "name", (u) => !!u.address && u.age > 40, "host", "presence");
assert.deepStrictEqual(pres, ["users/user13"]);
same("users", [[{ field: "address", not: true }, { field: "active", eq: false }]], "name", (u) => !u.address && u.active === false, "host", "absence");
assert.deepStrictEqual(query.where("users", [], { over: "name" }), []);
assert.throws(() => query.where("users", [[{ field: "age", eq: 1 }]]), TypeError);
assert.deepStrictEqual(query.where("nothing", [[{ field: "x", not: true }]], { over: "here" }), []);

/* ---- an integer-coded collection: every index lives on the device ---- */
const people = {};
for (let i = 0; i < 900; i++) {
  const p = { age: 18 + (i * 7) % 50, active: i % 3 === 0 ? 0 : 1, seq: i };
  if (i % 4 !== 1) p.role = (i * 5) % 4;            // 0 = admin; a quarter has no role
  if (i % 10 === 3) p.zip = 90000 + (i % 7);        // a tenth has an address code
  people["p" + i] = p;
}
if (!HOST_ONLY) {
  same("users", [[{ field: "role", ne: "user" }, { field: "age", min: 25, max: 45 }], [{ field: "name", eq: "Carol Davis" }]], "age",
    (u) => (u.role !== "user" && u.age >= 25 && u.age <= 45) || u.name === "Carol Davis", "host", "host literals over an integer index");
  for (const [k, v] of Object.entries(people)) b.get("people/" + k).put(v);
  const e8 = same("people", [[{ field: "active", eq: 1 }, { field: "age", max: 29 }, { field: "role", ne: 0 }]], "seq",
    (u) => u.active === 1 && u.age < 30 && u.role !== 0, "device", "example 8 on the device");
  assert.ok(e8.some((p) => people[p.slice(7)].role === undefined), "a child without the field passes the negation");
  same("people", [[{ field: "role", eq: 1 }], [{ field: "role", eq: 3 }]], "seq", (u) => u.role === 1 || u.role === 3, "device", "or on the device");
  same("people", [[{ field: "zip" }, { field: "zip", eq: 90003 }]], "seq", (u) => u.zip !== undefined && u.zip === 90003, "device", "presence on the device");
  same("people", [[{ field: "zip", not: true }, { field: "age", min: 60 }], [{ field: "seq", max: 4 }]], "seq", (u) => (u.zip === undefined && u.age >= 60) || u.seq <= 4, "device", "absence on the device");
  same("people", [[{ field: "role", eq: "admin" }], [{ field: "age", eq: 20.5 }]], "seq", () => false, "device", "bounds no integer satisfies");
  same("people", [[{ field: "role", ne: "admin" }]], "seq", () => true, "device", "... and their negation");
  same("people", [[{ field: "nobody", not: true }, { field: "age", max: 20 }]], "seq", (u) => u.age <= 20, "device", "a field no child carries");
  same("people", [[{ field: "nobody", not: true }]], "seq", () => true, "device", "... alone in its clause: every candidate");
  same("people", [[{ field: "nobody" }, { field: "age", max: 20 }], [{ field: "seq", max: 4 }]], "seq", (u) => u.seq <= 4, "device", "... positive: its clause is gone");
  same("people", [[{ field: "nobody", eq: 3 }]], "seq", () => false, "device", "... and nothing is left");
  { /* the kind of a literal's field comes from its index: no walk over the store once the indexes exist */
    const real = b._getData.bind(b); let reads = 0;
    b._getData = (p) => { reads++; return real(p); };
    query.where("people", [[{ field: "role", eq: 1 }, { field: "zip", not: true }]], { over: "seq" });
    b._getData = real;
    assert.strictEqual(reads, 0, "where() on fresh indexes reads the store " + reads + " times");
    checks++;
  }
  /* a write is seen by the next query */
  b.get("people/p2").put(Object.assign({}, people.p2, { role: 0 })); people.p2.role = 0;
  same("people", [[{ field: "role", eq: 0 }, { field: "seq", max: 10 }]], "seq", (u) => u.role === 0 && u.seq <= 10, "device", "after a write");
  /* DeviceGraph.scanWhere itself: ids as a typed array */
  const ixSeq = query.indices["people:seq"], ixAge = query.indices["people:age"];
  const ids = query.graph.scanWhere(ixSeq.deviceField, [[[ixAge.deviceField, 18, 18]], [[ixSeq.deviceField, 0, 0, true], [ixSeq.deviceField, -Infinity, 1]]]);
  assert.ok(ids instanceof BigUint64Array);
  assert.strictEqual(ids.length, Object.values(people).filter((u) => u.age === 18 || (u.seq !== 0 && u.seq <= 1)).length);
  assert.throws(() => query.graph.scanWhere(ixSeq.deviceField, []), RangeError);
  assert.throws(() => query.graph.scanWhere(ixSeq.deviceField, [new Array(9).fill([ixAge.deviceField, 0, 1])]), RangeError);
  checks += 2;
}

if (b.close) b.close();
else query.close();
console.log("query_where ok: " + checks + " checks" + (HOST_ONLY ? " (host indexes only)" : ""));
