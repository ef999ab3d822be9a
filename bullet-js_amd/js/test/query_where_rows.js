"use strict";
/*
 * query_where_rows.js — test of GpuQuery.whereRows and DeviceGraph.whereRows over the N-API addon (include/bmx_rows.h): the children a boolean filter selects
 * together with some of their fields, against filter(path, fn) followed by a projection written out by hand — Example 8 of docs/querying.md and an OR of two
 * equalities, paged. A cell without data (the field absent or deleted) is undefined in rows[i].
 * Usage: node query_where_rows.js <golden dir> [host]      "host": only the indexes that live on the host — needs no GPU
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

const b = new MiniBullet("wr");
let query;
if (HOST_ONLY) {   // no device behind the facade: every write is applied as it comes
  b.crt = { handleUpdate: (p, data) => ({ doUpdate: true, value: data, vectorClock: {} }) };
  query = new GpuQuery(b);
}
else ({ query } = require("..").attach(b, { capacityRows: 1 << 16 }));

/* filter(path, fn) + the projection, by hand: path -> {name: value | undefined} */
function projected(coll, fn, names) {
  const want = new Map();
  for (const n of query.filter(coll, fn)) {
    const u = b._getData(n.path), row = {};
    for (const f of names) row[f] = u[f] === null ? undefined : u[f];
    want.set(n.path, row);
  }
  return want;
}
const asMap = (r) => { const m = new Map(); r.paths.forEach((p, i) => m.set(p, r.rows[i])); assert.strictEqual(m.size, r.paths.length, "a path twice"); return m; };
const sortedEntries = (m) => Array.from(m.entries()).sort((x, y) => (x[0] < y[0] ? -1 : 1));

/* one shot, then pages of `cap`: the pages concatenate to the one-shot answer, nMatch falls by the page length, next is null behind the last */
function check(coll, clauses, fn, names, over, cap, kind, what) {
  const want = projected(coll, fn, names);
  const one = query.whereRows(coll, clauses, names, { over });
  assert.strictEqual(query.lastPath, kind, what);
  assert.strictEqual(one.nMatch, want.size, what + " nMatch");
  assert.strictEqual(one.next, null, what);
  assert.deepStrictEqual(sortedEntries(asMap(one)), sortedEntries(want), what);
  for (const row of one.rows) assert.deepStrictEqual(Object.keys(row).sort(), Array.from(new Set(names)).sort(), what + ": every name is a key, undefined included");
  let start = null, left = want.size, pages = 0;
  const paths = [], rows = [];
  for (;;) {
    const page = query.whereRows(coll, clauses, names, { over, cap, start });
    assert.strictEqual(page.nMatch, left, what + " nMatch of a page");
    assert.ok(page.paths.length <= cap && page.paths.length === Math.min(cap, left));
    paths.push(...page.paths); rows.push(...page.rows); left -= page.paths.length; pages++;
    if (!page.next) break;
    start = page.next;
  }
  assert.deepStrictEqual(paths, one.paths, what + ": the pages concatenate, in order");
  assert.deepStrictEqual(rows, one.rows, what);
  assert.strictEqual(pages, Math.max(Math.ceil(want.size / cap), 1), what + " pages");
  checks++;
  return want.size;
}

/* ---- the reference's users: name / role are strings, active a boolean — host indexes; filter + projection in JS ---- */
const users = JSON.parse(JSON.stringify(g.users));
users.user11 = { name: "Kim Nolan", age: 22, active: true };                        // no role at all
users.user12 = { name: "Lee Ortiz", age: 27, active: true, role: "admin" };
users.user13 = { name: "Lee Ortiz", age: 27, active: false, role: "editor" };
for (const [k, v] of Object.entries(users)) b.get("users/" + k).put(v);

const ex8 = [[{ field: "active", eq: true }, { field: "age", max: 29 }, { field: "role", ne: "admin" }]];
const ex8fn = (u) => u.active === true && u.age < 30 && u.role !== "admin";
assert.ok(check("users", ex8, ex8fn, ["name", "role", "age"], "name", 2, "host", "example 8") >= 2);
assert.ok(projected("users", ex8fn, ["role"]).get("users/user11").role === undefined, "a child without the field passes the negation and projects undefined");
const or2 = [[{ field: "role", eq: "admin" }], [{ field: "role", eq: "editor" }]];
const or2fn = (u) => u.role === "admin" || u.role === "editor";
assert.ok(check("users", or2, or2fn, ["name", "age", "nobody", "name"], "name", 1, "host", "or, one per page") >= 3);
check("users", or2, or2fn, [], "name", 100, "host", "or, no fields");
{ const none = query.whereRows("users", [], ["name"], { over: "age" }); assert.deepStrictEqual(none, { paths: [], rows: [], nMatch: 0, next: null }); }
assert.throws(() => query.whereRows("users", or2, ["name"]), TypeError);
checks += 2;

/* ---- an integer-coded collection: every index lives on the device ---- */
if (!HOST_ONLY) {
  // an integer index as `over` with literals or projected fields on host indexes: the host answers
  check("users", or2, or2fn, ["age", "name"], "age", 2, "host", "host literals over an integer index");
  check("users", [[{ field: "age", max: 29 }]], (u) => u.age < 30, ["age", "name"], "age", 3, "host", "a projected field on a host index");
  const people = {};
  for (let i = 0; i < 900; i++) {
    const p = { age: 18 + (i * 7) % 50, active: i % 3 === 0 ? 0 : 1, seq: i, score: (i * 37) % 1000 - 300 };
    if (i % 5 !== 1) p.role = (i * 3) % 4;            // 0 = admin; every code occurs; a fifth has no role
    if (i % 10 === 3) delete p.score;                 // a tenth has no score
    people["p" + i] = p;
  }
  for (const [k, v] of Object.entries(people)) b.get("people/" + k).put(v);
  // Example 8's shape with role codes: active && age < 30 && role !== admin; name, role and age of the matches
  const e8 = [[{ field: "active", eq: 1 }, { field: "age", max: 29 }, { field: "role", ne: 0 }]];
  const e8fn = (u) => u.active === 1 && u.age < 30 && u.role !== 0;
  const n8 = check("people", e8, e8fn, ["role", "age", "score"], "seq", 7, "device", "example 8 on the device");
  assert.ok(n8 > 20);
  const w8 = projected("people", e8fn, ["role", "score"]);
  assert.ok(Array.from(w8.values()).some((r) => r.role === undefined) && Array.from(w8.values()).some((r) => r.score === undefined), "absent cells among the matches");
  // an OR of two equalities, paged; the base field, a repeated name and a field no child carries among the projected
  const orr = [[{ field: "role", eq: 1 }], [{ field: "role", eq: 3 }, { field: "nobody", not: true }]];
  const orfn = (u) => u.role === 1 || u.role === 3;
  check("people", orr, orfn, ["seq", "score", "seq", "nobody", "role"], "seq", 64, "device", "or on the device");
  check("people", orr, orfn, [], "seq", 1000, "device", "or on the device, no fields");
  check("people", [[{ field: "nobody", eq: 3 }]], () => false, ["age"], "seq", 5, "device", "nothing selected");
  /* a write is seen by the next query */
  b.get("people/p2").put(Object.assign({}, people.p2, { role: 1 })); people.p2.role = 1;
  check("people", orr, orfn, ["score", "role"], "seq", 100, "device", "after a write");
  /* DeviceGraph.whereRows itself: typed arrays, clocks, the cursor */
  const ixSeq = query.indices["people:seq"], ixAge = query.indices["people:age"], ixRole = query.indices["people:role"];
  const prog = [[[ixAge.deviceField, 18, 18]], [[ixRole.deviceField, 0, 0, true], [ixSeq.deviceField, -Infinity, 9]]];
  const fn = (u) => u.age === 18 || (u.role !== 0 && u.seq <= 9);
  const want = query.filter("people", fn).length;
  const all = query.graph.whereRows(ixSeq.deviceField, prog, [ixAge.deviceField, ixRole.deviceField], { ts: true });
  assert.ok(all.ids instanceof BigUint64Array && all.ids.length === want && all.nMatch === want && all.vals.length === 2 && all.ts.length === 2);
  assert.ok(all.vals.every((c) => c instanceof BigInt64Array && c.length === want) && all.ts.every((c) => c instanceof BigInt64Array && c.length === want));
  assert.ok(all.layout > 0 && all.nextShard === 0 && all.nextPos === query.graph.indexSize(ixSeq.deviceField));
  const NONE = -(2n ** 63n);
  for (let i = 0; i < want; i++) {
    assert.ok(all.vals[0][i] !== NONE && all.ts[0][i] >= 0n, "every child holds an age");
    assert.strictEqual(all.ts[1][i] === -1n, all.vals[1][i] === NONE, "no role: no clock (nothing was deleted there)");
  }
  const count = query.graph.whereRows(ixSeq.deviceField, prog, [], { cap: 0 });
  assert.ok(count.ids.length === 0 && count.nMatch === want && count.ts === undefined);
  const p1 = query.graph.whereRows(ixSeq.deviceField, prog, [ixAge.deviceField], { cap: 5 });
  const p2 = query.graph.whereRows(ixSeq.deviceField, prog, [ixAge.deviceField], { cap: want, start: p1.nextPos });
  assert.deepStrictEqual(Array.from(p1.ids).concat(Array.from(p2.ids)), Array.from(all.ids));
  assert.deepStrictEqual(Array.from(p1.vals[0]).concat(Array.from(p2.vals[0])), Array.from(all.vals[0]));
  assert.ok(p2.nMatch === want - 5 && p1.layout === all.layout && p2.layout === all.layout);
  assert.throws(() => query.graph.whereRows(ixSeq.deviceField, [], []), RangeError);
  assert.throws(() => query.graph.whereRows(ixSeq.deviceField, prog, new Array(9).fill(ixAge.deviceField)), RangeError);
  assert.throws(() => query.graph.whereRows(ixSeq.deviceField, prog, [], { cap: -1 }), RangeError);
  assert.throws(() => query.whereRows("people", orr, ["role"], { over: "seq", cap: 3, start: { at: 0, layout: all.layout + 1 } }), (e) => e.code === "BMX_STALE_CURSOR");
  checks += 5;
}

if (b.close) b.close();
else query.close();
console.log("query_where_rows ok: " + checks + " checks" + (HOST_ONLY ? " (host indexes only)" : ""));
