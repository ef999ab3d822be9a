"use strict";
/*
 * gpu-query.js — GpuQuery: drop-in for the reference's query engine behind `bullet.query`
 * (plug point: `new Bullet({enableIndexing: false}); bullet.query = new GpuQuery(bullet)`, SURVEY §8(b)).
 *
 * Interface mirrored (src/bullet-query.js): index :30, equals :186, range :221, filter :270, count :293,
 * map :322, find :342, the `indices` object keyed "path:field" (read by src/bullet-serializer.js:655-665),
 * and the setData hook of :13-21. Results are arrays of bullet.get(path) nodes, in the reference's order.
 *
 * Where the work happens:
 *   - an index whose values are all safe integers lives on the MI355X: index() loads the children's
 *     (node id, value) rows and bmx_index_build() compacts them into dense columns; equals/range/count and
 *     filterWhere() stream those columns (bmx_scan_*). Nothing on the host re-implements those scans.
 *   - an index over strings/booleans/objects (e.g. role === "admin") cannot be expressed in the device's
 *     integer domain and is kept as a host Map, like the reference does for everything.
 *   - filter/map/find take arbitrary JS callbacks and run on the host, as in the reference.
 *
 * Freshness: the reference maintains its indices incrementally and drifts (SURVEY §8(a) Q4); parity is defined
 * on the FRESH state: what _buildIndex would produce from the store at query time. A write under an indexed path is
 * remembered per CHILD; the next query re-reads only those children from the store, patches its host mirror and
 * sends their rows to the device, whose own change log brings the dense columns up to date (include/bmx.h
 * "Maintenance") — work proportional to what changed, not to the collection. Whenever the patched state could
 * differ from a fresh build (a child left the index or the integer domain, a child that existed without the field
 * gained it, an integer-like new key, a write at or above the indexed path) the index is rebuilt from the store.
 */
const { Columns, fieldId, isDeviceInt, pathId } = require("./hash");

function bucketKey(v) { return (typeof v === "object" && v !== null) ? JSON.stringify(v) : String(v); }

/* top() / whereTop() on a host index: numbers compare as numbers and come before everything else, which compares by its bucket key */
function cmpVal(a, b) {
  const na = typeof a === "number", nb = typeof b === "number";
  if (na && nb) return a < b ? -1 : a > b ? 1 : 0;
  if (na !== nb) return na ? -1 : 1;
  const ka = bucketKey(a), kb = bucketKey(b);
  return ka < kb ? -1 : ka > kb ? 1 : 0;
}

/* where() / whereTop() on the host: the truth of one normalised literal for one child of the store */
function literalTruth(child, t) {
  let x = child && typeof child === "object" ? child[t.field] : undefined;
  let pos = x !== null && x !== undefined;
  if (t.minus !== undefined) {             // field - minus: both present; anything but two numbers gives NaN, inside no bounds (`undefined > x` is false)
    const y = child && typeof child === "object" ? child[t.minus] : undefined;
    pos = pos && y !== null && y !== undefined;
    x = pos && typeof x === "number" && typeof y === "number" ? x - y : NaN;
  }
  if (t.clock !== undefined) {             // the clock of the row: a host index is built, never patched, so a present field is a data row of clock 1 (HOST_CLOCK)
    pos = pos && t.clock !== "deleted";    // and an absent or deleted field is no row at all
    x = HOST_CLOCK;
  }
  if (pos) pos = t.eq ? x === t.min : (t.min === -Infinity || x >= t.min) && (t.max === Infinity || x <= t.max);
  return pos !== t.not;
}

const HOST_CLOCK = 1;                 // the clock of every row of an index as built (_buildDevice loads with clock 1); patches of a device index use 2, 3, ...
const CLOCK_STATES = { data: 1, deleted: 2, any: 3 };      // the sixth entry of a native literal (bmx_where.h BMX_LIT_CLOCK = data, BMX_LIT_CLOCK_TOMB = deleted)
const ORDERED_AUTO = 0xffffffff;      // BMX_INDEX_ORDERED_AUTO: the engine weighs a sort against the scans it saves
const orderedOpt = (v) => (v === "auto" ? ORDERED_AUTO : v >>> 0);

class GpuQuery {
  /** @param {object} bullet @param {object} [opts] { graph: DeviceGraph shared with GpuCRT, device, capacityRows } */
  constructor(bullet, opts = {}) {
    this.bullet = bullet;
    this.indices = {};
    this.indexedPaths = new Set();
    this.lastPath = null;           // 'device' | 'host': which side answered the last indexed query (for tests/ops)
    this._opts = opts;
    this._graph = opts.graph || null;
    this._gen = 0;
    this._byBase = new Map();       // indexed path -> its index records
    this.stats = { builds: 0, patches: 0 };
    this._hookWrites();
  }

  get graph() {
    if (!this._graph) {
      const DeviceGraph = require("./device-graph");
      this._graph = new DeviceGraph(this._opts);
      this._ownsGraph = true;
    }
    return this._graph;
  }

  _hookWrites() {
    const inner = this.bullet.setData.bind(this.bullet);
    this.bullet.setData = (path, data, broadcast = true) => {
      inner(path, data, broadcast);            // like the reference's hook, the return value is dropped
      this._touch(path);
    };
  }

  _touch(path) {
    for (const [base, list] of this._byBase) {
      if (path.length > base.length && path.charCodeAt(base.length) === 47 && path.startsWith(base)) {
        // below the indexed path: only this child has to be looked at again
        const cut = path.indexOf("/", base.length + 1);
        const child = cut < 0 ? path.slice(base.length + 1) : path.slice(base.length + 1, cut);
        for (const ix of list) {
          if (ix.stale === true) continue;
          if (!ix.stale) { ix.stale = "partial"; ix.dirty = new Set(); }
          ix.dirty.add(child);
        }
      } else if (path === base || base.startsWith(path + "/")) {
        for (const ix of list) { ix.stale = true; ix.dirty = null; }
      }
    }
  }

  static keyOf(path, field) { return field ? `${path}:${field}` : path; }

  /**
   * index(path, field) as in the reference. opts.source === 'device' indexes the rows that already live on the GPU
   * (ingested through GpuCRT.mergeEntries / mergeBatch under the same (collection, field) hash) instead of uploading the
   * children found in the JS store: the sync -> device -> query flow then never re-sends values.
   * opts.ordered = N >= 1 or "auto" (the engine sorts once the scans since the last write have cost what a sort costs): the device also keeps a VALUE-ORDERED view of the index — the shape of the reference's own index, a Map keyed by value
   * (src/bullet-query.js:30-73) —, so equals / range / count cost O(log R + matches) instead of one pass over the column while the field is not written;
   * a stale view is sorted again by the N-th query after a write (bmx_index_set_ordered); on a sharded graph every shard keeps its own.
   * attach(bullet, {orderedIndexes: N}) makes N the default for every index of this engine (the reference's own calls pass no options).
   */
  index(path, field = null, opts = {}) {
    const key = GpuQuery.keyOf(path, field);
    if (this.indices[key]) return this;
    this.indices[key] = { path, field, stale: true, dirty: null, kind: null, source: opts.source === "device" ? "device" : "store", ordered: orderedOpt(opts.ordered !== undefined ? opts.ordered : this._opts.orderedIndexes) };
    this.indexedPaths.add(path);
    if (!this._byBase.has(path)) this._byBase.set(path, []);
    this._byBase.get(path).push(this.indices[key]);
    this._build(this.indices[key]);
    return this;
  }

  /* device-sourced index: nothing to upload; rows are the ones merge batches put there */
  _buildFromDevice(ix) {
    const g = this.graph;
    ix.kind = "device";
    ix.deviceField = g.keys.fieldOf(ix.path, ix.field);
    g.indexBuild(ix.deviceField);
    if (ix.ordered && typeof g.indexSetOrdered === "function") g.indexSetOrdered(ix.deviceField, ix.ordered === ORDERED_AUTO ? ORDERED_AUTO : 2 * ix.ordered);   // opts.ordered: the device keeps a value-ordered view too (a query here = a count + a fetch on the device)
    ix.paths = null; ix.values = null; ix.stale = false; ix.dirty = null; ix.rank = null; ix._posByPath = null;
  }

  /* scan the direct children of `path` (one level, as _buildIndex does) and materialise the index */
  _build(ix) {
    if (ix.source === "device") { this._buildFromDevice(ix); return; }
    const base = this.bullet._getData(ix.path);
    const paths = [], values = [];
    this.stats.builds++;
    ix.allChildren = new Set(typeof base === "object" && base !== null ? Object.keys(base) : []);
    if (typeof base === "object" && base !== null) {
      for (const [child, v] of Object.entries(base)) {
        let x;
        if (ix.field) {
          if (typeof v !== "object" || v === null || !(ix.field in v)) continue;
          x = v[ix.field];
        } else {
          x = v;
        }
        if (x === null || x === undefined) continue;
        paths.push(`${ix.path}/${child}`);
        values.push(x);
      }
    }
    ix.paths = paths;
    ix.values = values;
    ix.stale = false;
    ix.dirty = null;
    ix.rank = null;
    ix._posByPath = null;
    ix.ordOfPos = null;
    if (values.length > 0 && values.every(isDeviceInt)) this._buildDevice(ix);
    else this._buildHost(ix);
  }

  _buildHost(ix) {
    ix.kind = "host";
    const buckets = new Map();
    ix.values.forEach((v, i) => {
      const k = bucketKey(v);
      if (!buckets.has(k)) buckets.set(k, []);
      buckets.get(k).push(i);
    });
    ix.buckets = buckets;
  }

  _buildDevice(ix) {
    const g = this.graph;                       // throws when the addon / GPU is missing: no host scan for integer indices
    ix.kind = "device";
    if (ix.deviceField !== undefined) g.indexDrop(ix.deviceField);
    // rows of an older build of this index stay behind under their own field hash and are never scanned again
    ix.deviceField = g.keys.fieldOf(ix.path + "#" + (++this._gen), ix.field);
    const n = ix.paths.length;
    const cols = new Columns(n);
    for (let i = 0; i < n; i++) cols.set(i, g.keys.idOf(ix.paths[i]), ix.deviceField, 1, ix.values[i]);
    g.loadRows(cols);
    g.indexBuild(ix.deviceField);
    if (ix.ordered && typeof g.indexSetOrdered === "function") g.indexSetOrdered(ix.deviceField, ix.ordered === ORDERED_AUTO ? ORDERED_AUTO : 2 * ix.ordered);   // opts.ordered: value-ordered view on the device (bmx_index_set_ordered)
    ix.seq = 1;                                 // ts of the device rows of this build; patches use 2, 3, ...
  }

  /*
   * Q4 (_updateIndices, src/bullet-query.js:139-174) without its drift: re-read the children written since the last query and patch the
   * index instead of rebuilding it. Returns false when only a fresh build is guaranteed to give the reference's state.
   */
  _applyDirty(ix) {
    if (ix.kind !== "device" || ix.source === "device" || !ix.dirty || !ix.paths) return false;
    const base = this.bullet._getData(ix.path);
    if (typeof base !== "object" || base === null) return false;
    const pos = ix._posByPath || (ix._posByPath = new Map(ix.paths.map((p, i) => [p, i])));
    const changed = [];                          // ordinals whose device row has to be rewritten (a bail-out below rebuilds the mirror: nothing to roll back)
    for (const child of ix.dirty) {
      const v = base[child];
      let x, present = true;
      if (ix.field) {
        if (typeof v !== "object" || v === null || !(ix.field in v)) present = false; else x = v[ix.field];
      } else x = v;
      if (present && (x === null || x === undefined)) present = false;
      const p = `${ix.path}/${child}`;
      const at = pos.get(p);
      if (at !== undefined) {
        if (!present || !isDeviceInt(x)) return false;              // left the index, or the integer domain
        if (ix.values[at] !== x) { ix.values[at] = x; changed.push(at); }
      } else {
        if (!present) { if (v !== undefined) ix.allChildren.add(child); continue; }
        if (!isDeviceInt(x)) return false;                           // the index stops being an integer index
        if (ix.allChildren.has(child)) return false;                 // it existed without the field: a fresh scan lists it where it was created, not last
        if (/^(0|[1-9][0-9]*)$/.test(child)) return false;           // integer-like keys are enumerated before all others, in numeric order
        ix.allChildren.add(child);
        pos.set(p, ix.paths.length); ix.paths.push(p); ix.values.push(x); changed.push(ix.paths.length - 1);
      }
    }
    if (changed.length) {
      const g = this.graph;
      const cols = new Columns(changed.length);
      const ts = ++ix.seq;
      for (let k = 0; k < changed.length; k++) cols.set(k, g.keys.idOf(ix.paths[changed[k]]), ix.deviceField, ts, ix.values[changed[k]]);
      g.loadRows(cols);                          // newer ts: plain LWW on the device; its change log updates the dense columns at the next scan
      ix.rank = null;
    }
    ix.stale = false; ix.dirty = null;
    this.stats.patches++;
    return true;
  }

  _fresh(path, field) {
    const key = GpuQuery.keyOf(path, field);
    if (!this.indices[key]) this.index(path, field);
    const ix = this.indices[key];
    const crt = this.bullet.crt;
    if (crt && typeof crt._flushDeviceWrites === "function") crt._flushDeviceWrites();   // single writes queued for the device (GpuCRT write-through)
    if (ix.stale === "partial" && this._applyDirty(ix)) return ix;
    if (ix.stale) this._build(ix);
    return ix;
  }

  /* device-sourced index: ids -> nodes, ordered by path (the store holds no scan order for them) */
  _nodesFromIds(ids) {
    const u32 = new Uint32Array(ids.buffer, ids.byteOffset, ids.length * 2);
    const paths = [];
    for (let i = 0; i < ids.length; i++) {
      const p = this.graph.keys.pathOf(u32[2 * i], u32[2 * i + 1]);
      if (p !== undefined) paths.push(p);
    }
    paths.sort();
    return paths.map((p) => this.bullet.get(p));
  }

  /* device ids -> child ordinals of the build scan */
  _ordinals(ix, ids) {
    const u32 = new Uint32Array(ids.buffer, ids.byteOffset, ids.length * 2);
    const out = new Array(ids.length);
    const pos = ix._posByPath || (ix._posByPath = new Map(ix.paths.map((p, i) => [p, i])));
    for (let i = 0; i < ids.length; i++) {
      const p = this.graph.keys.pathOf(u32[2 * i], u32[2 * i + 1]);
      out[i] = pos.get(p);
    }
    return out;
  }

  /* Matches of lo..hi as child ordinals of the build scan, through index POSITIONS (bmx_scan_range_pos): the device gathers no ids, and the host
   * turns a position into an ordinal with one typed-array read instead of an id -> path -> ordinal lookup per match. ordOfPos is fetched once
   * per build of the device columns (bmx_index_ids) and extended when rows were appended; a full rebuild renumbers the positions (detected by
   * the engine's own count of full builds). Sharded graphs number positions per shard: they keep the id path. */
  _matches(ix, lo, hi) {
    const g = this.graph;
    if (g.comm) return this._ordinals(ix, g.scanRange(ix.deviceField, lo, hi));
    const pos = g.scanRangePos(ix.deviceField, lo, hi);
    const builds = g.indexRefreshCounts().fullBuilds;
    if (!ix.ordOfPos || ix.posBuilds !== builds) { ix.ordOfPos = []; ix.posBuilds = builds; }
    const n = g.indexSize(ix.deviceField);
    if (ix.ordOfPos.length < n) {
      const have = ix.ordOfPos.length;
      const ords = this._ordinals(ix, g.indexIds(ix.deviceField, have, n - have));
      for (let i = 0; i < ords.length; i++) ix.ordOfPos.push(ords[i]);
    }
    const out = new Array(pos.length);
    for (let i = 0; i < pos.length; i++) out[i] = ix.ordOfPos[pos[i]];
    return out;
  }

  /* reference order of a result set: distinct values in first-seen order of the build scan, children of one value in scan order */
  _inReferenceOrder(ix, ordinals) {
    if (!ix.rank) {
      const seen = new Map();
      ix.rank = ix.values.map((v) => { const k = bucketKey(v); if (!seen.has(k)) seen.set(k, seen.size); return seen.get(k); });
    }
    return ordinals.sort((a, b) => (ix.rank[a] - ix.rank[b]) || (a - b));
  }

  _nodes(ix, ordinals) { return ordinals.map((i) => this.bullet.get(ix.paths[i])); }

  equals(path, field, value) {
    if (arguments.length === 2) { value = field; field = null; }
    const ix = this._fresh(path, field);
    this.lastPath = ix.kind;
    if (ix.kind === "host") {
      const hit = ix.buckets.get(bucketKey(value));
      return hit ? this._nodes(ix, hit) : [];
    }
    // the reference compares String(value): 30 and "30" are the same bucket
    const n = typeof value === "string" && value.trim() !== "" ? Number(value) : value;
    if (!isDeviceInt(n) || String(n) !== String(value)) return [];
    if (ix.source === "device") return this._nodesFromIds(this.graph.scanRange(ix.deviceField, n, n));
    return this._nodes(ix, this._matches(ix, n, n).sort((a, b) => a - b));
  }

  range(path, field, min, max) {
    if (arguments.length === 3) { max = min; min = field; field = null; }
    const ix = this._fresh(path, field);
    this.lastPath = ix.kind;
    if (typeof min === "undefined" || typeof max === "undefined") return [];
    if (ix.kind === "device" && typeof min === "number" && typeof max === "number" && !Number.isNaN(min) && !Number.isNaN(max)) {
      // integer column: lo = ceil(min), hi = floor(max) select exactly the values with min <= v <= max
      if (ix.source === "device") return this._nodesFromIds(this.graph.scanRange(ix.deviceField, Math.ceil(min), Math.floor(max)));
      return this._nodes(ix, this._inReferenceOrder(ix, this._matches(ix, Math.ceil(min), Math.floor(max))));
    }
    if (ix.source === "device") return [];   // non-numeric bounds cannot match integer rows
    // host index, or bounds the device cannot express (strings): JS comparison semantics on the host
    this.lastPath = "host";
    const out = [];
    const groups = new Map();
    ix.values.forEach((v, i) => { const k = bucketKey(v); if (!groups.has(k)) groups.set(k, []); groups.get(k).push(i); });
    for (const [k, members] of groups) {
      let v = Number(k);
      if (Number.isNaN(v)) v = k;
      if (v >= min && v <= max) out.push(...members);
    }
    return this._nodes(ix, out);
  }

  count(path, field, value) {
    if (arguments.length === 2) { value = field; field = null; }
    const ix = this._fresh(path, field);
    this.lastPath = ix.kind;
    if (ix.kind === "host") {
      const hit = ix.buckets.get(bucketKey(value));
      return hit ? hit.length : 0;
    }
    const n = typeof value === "string" && value.trim() !== "" ? Number(value) : value;
    if (!isDeviceInt(n) || String(n) !== String(value)) return 0;
    return this.graph.scanCount(ix.deviceField, n, n);
  }

  /**
   * Declarative filter on the device: AND of range terms over integer fields of the same child node.
   * terms: [{field, min, max}]  (equality: min === max). The arbitrary-callback form stays in filter().
   */
  filterWhere(path, terms) {
    if (!terms || terms.length === 0) return [];
    const ixs = terms.map((t) => this._fresh(path, t.field));
    if (!ixs.every((ix) => ix.kind === "device")) {
      const err = new Error("bmx: filterWhere needs integer-valued fields on every term");
      err.code = "BMX_NOT_DEVICE_INDEX";
      throw err;
    }
    this.lastPath = "device";
    const native = terms.map((t, k) => [ixs[k].deviceField, Math.ceil(t.min), Math.floor(t.max)]);
    const ids = this.graph.scanFilter(native);
    return this._nodes(ixs[0], this._ordinals(ixs[0], ids).sort((a, b) => a - b));
  }

  /* "device" / "host" / "absent" (no child carries the field): the kind of the index of (path, field). An index that exists answers, brought up to date as for
   * any query (work proportional to what was written since). Only a field without an index costs one walk over the children of path; its result is recorded as
   * an index where that needs no device (host, absent), and by the device build that follows where the query goes to the device. */
  _fieldKind(path, field) {
    if (this.indices[GpuQuery.keyOf(path, field)]) {
      const ix = this._fresh(path, field);
      return ix.kind === "device" ? "device" : (ix.values && ix.values.length ? "host" : "absent");
    }
    const base = this.bullet._getData(path);
    let kind = "absent";
    if (typeof base === "object" && base !== null) {
      for (const v of Object.values(base)) {
        if (typeof v !== "object" || v === null) continue;
        const x = v[field];
        if (x === null || x === undefined) continue;
        if (!isDeviceInt(x)) { kind = "host"; break; }
        kind = "device";
      }
    }
    if (kind !== "device") this.index(path, field);      // a host index (empty for "absent"): built from the store, the next query asks it
    return kind;
  }

  /**
   * Boolean filter: OR of AND-clauses over fields of the same child node, with NOT and with defined behaviour for absent fields — the shapes of
   * filter(path, fn) that an AND of ranges cannot say (docs/querying.md Example 8: `user.active === true && user.age < 30 && user.role !== "admin"`).
   * clauses: [[{field, min, max, not}, ...], ...]; {field, eq: v} is min = max = v and {field, ne: v} is its negation; a bound left out (or +-Infinity) is
   * not checked, so {field} alone tests presence and {field, not: true} absence. {field, minus: "other", ...} compares two fields of the child: the bounds
   * are on field - other (`o.shipped > o.due` is {field: "shipped", minus: "due", min: 1} on integers), true iff both are present and the difference is
   * inside; its negation is true when either is missing. {field, clock: "data" | "deleted" | "any", ...} ranges over the CLOCK of the field's row in the
   * index, with the same bound keys: true iff the row exists in the named state and its clock is inside. The clock of an index GpuQuery built is its patch
   * sequence — 1 for every row of a build, 2, 3, ... for the rows each later patch rewrote ("what changed since patch N" is {clock: "data", min: N + 1}) —
   * and a field that is deleted leaves the index at the next build, so "deleted" selects only in a device-sourced index, whose rows carry the table's own
   * clocks and tombstones. whereRows(..., {clocks: true}) reports the clocks a term ranges over.
   * opts.over (required) names the field that defines the universe: only children that carry it are candidates — the children filter() would iterate,
   * provided every child the caller cares about carries it. A literal is true iff the child's field is present (not null / undefined) and inside its bounds;
   * a negated literal is the exact complement, so it is true for a child WITHOUT the field, as `undefined !== "admin"` is.
   * When every index involved is an integer index the device answers (bmx_scan_where); when one lives on the host (strings, booleans, objects, fractions)
   * the same semantics are evaluated over the host mirror, as top() does for host indexes. -> the BulletNodes in the scan order of `over`'s index.
   * Host cost: the kind of every literal's field comes from its index (O(1) while nothing was written); the FIRST query that names a field without an index
   * walks the children once to build it, like index(). The host evaluation is one loop over the children that carry `over`.
   */
  where(path, clauses, opts = {}) {
    if (opts.over === undefined || opts.over === null) throw new TypeError("bmx: where needs opts.over, the field that defines the universe");
    if (!clauses || clauses.length === 0) return [];
    const { norm, base, native } = this._whereProgram(path, clauses, opts.over);
    if (native) {
      this.lastPath = "device";
      if (native.length === 0) return [];
      const ids = this.graph.scanWhere(base.deviceField, native);
      if (base.source === "device") return this._nodesFromIds(ids);
      return this._nodes(base, this._ordinals(base, ids).sort((a, b) => a - b));
    }
    const selected = this._whereHost(path, norm, base);
    this.lastPath = "host";
    return this._nodes(base, selected);
  }

  /* The program of where(), whereAggregate() and whereTop(), normalised: {field, eq: v} is min = max = v, {field, ne: v} its negation, a bound left out (or
   * +-Infinity) is open. -> {norm, base (the index of `over`), native}: native is the program as the device takes it ([[[field, lo, hi, not(, field2)], ...], ...], possibly
   * empty: no clause can be true) when every index involved is an integer index, and null when one lives on the host. */
  _whereProgram(path, clauses, over) {
    const open = (x) => x === undefined || x === null || x === Infinity || x === -Infinity;
    const norm = clauses.map((c) => c.map((t) => {
      const minus = t.minus === undefined || t.minus === null ? undefined : t.minus;      // {field, minus: other, ...}: the bounds are on field - other
      if (minus !== undefined && minus === t.field) throw new RangeError("bmx: where compares a field with another field, not with itself");
      const clock = t.clock === undefined || t.clock === null ? undefined : t.clock;      // {field, clock: state, ...}: the bounds are on the clock of the field's row
      if (clock !== undefined && !(clock in CLOCK_STATES)) throw new RangeError('bmx: a clock term names "data", "deleted" or "any"');
      if (clock !== undefined && minus !== undefined) throw new RangeError("bmx: a clock term takes no minus");
      if ("eq" in t) return { field: t.field, minus, clock, min: t.eq, max: t.eq, eq: true, not: !!t.not };
      if ("ne" in t) return { field: t.field, minus, clock, min: t.ne, max: t.ne, eq: true, not: !t.not };
      return { field: t.field, minus, clock, min: open(t.min) ? -Infinity : t.min, max: open(t.max) ? Infinity : t.max, eq: false, not: !!t.not };
    }));
    const base = this._fresh(path, over);
    // Which side answers is decided before a DEVICE index of a literal's field is built (it needs the device; the host evaluation reads the store and
    // needs none): "device" = every child that carries the field has a safe integer there, "absent" = no child carries it (_fieldKind).
    const kinds = new Map();
    for (const c of norm) for (const t of c) for (const f of t.minus === undefined ? [t.field] : [t.field, t.minus]) if (!kinds.has(f)) kinds.set(f, this._fieldKind(path, f));
    const onDevice = base.kind === "device" && Array.from(kinds.values()).every((k) => k !== "host");
    if (!onDevice) return { norm, base, native: null };
    const num = (x) => typeof x === "number" && !Number.isNaN(x);
    // A field no child carries is decided here: its positive literals are false (their clause goes), its negated ones true (the literal goes); a clause
    // left without a literal is true for every candidate, which a presence literal on the base field says. A pair with such a side is decided the same way.
    const absent = (t) => kinds.get(t.field) === "absent" || (t.minus !== undefined && kinds.get(t.minus) === "absent");
    const native = [];
    for (const c of norm) {
      if (c.some((t) => absent(t) && !t.not)) continue;
      const lits = c.filter((t) => !absent(t)).map((t) => {
        const f = this._fresh(path, t.field).deviceField;
        // [f, lo, hi, not, f2]: lo <= f - f2 <= hi; [f, lo, hi, not, null, states]: lo <= clock of f's row <= hi
        const tail = t.clock !== undefined ? [null, CLOCK_STATES[t.clock]] : t.minus === undefined ? [] : [this._fresh(path, t.minus).deviceField];
        // bounds no integer satisfies (a string against an integer field, a fraction as eq): the empty range, whose negation is always true
        if (!num(t.min) || !num(t.max)) return [f, 1, 0, t.not, ...tail];
        return [f, Math.ceil(t.min), Math.floor(t.max), t.not, ...tail];
      });
      native.push(lits.length ? lits : [[base.deviceField, -Infinity, Infinity, false]]);
    }
    return { norm, base, native };
  }

  /* the program over the host mirror of `over`'s index: the ordinals of the children it selects, in scan order */
  _whereHost(path, norm, base) {
    if (!base.paths) {
      const err = new Error("bmx: where over a device-sourced index needs integer-valued fields on every literal");
      err.code = "BMX_NOT_DEVICE_INDEX";
      throw err;
    }
    const store = this.bullet._getData(path);
    const out = [];
    base.paths.forEach((p, i) => {
      const child = store[p.slice(path.length + 1)];
      if (norm.some((c) => c.every((t) => literalTruth(child, t)))) out.push(i);
    });
    return out;
  }

  /* device indexes of the fields an aggregate names, or BMX_NOT_DEVICE_INDEX exactly where filterWhere throws it */
  _deviceIndexes(path, fields, what) {
    const ixs = fields.map((f) => this._fresh(path, f));
    if (!ixs.every((ix) => ix.kind === "device")) {
      const err = new Error(`bmx: ${what} needs integer-valued fields on every term`);
      err.code = "BMX_NOT_DEVICE_INDEX";
      throw err;
    }
    return ixs;
  }

  /**
   * Aggregate on the device (the reduction that query.map(path, fn).reduce(...) does on the host, src/bullet-query.js:322-333): over the children of path
   * that satisfy every term [{field, min, max}], the number matched, and count / sum / min / max of `field` over those that carry it.
   * -> {matched, count, sum, min, max}; sum is a Number while it is a safe integer, a BigInt otherwise; min and max are null when count === 0.
   */
  aggregateWhere(path, terms, field) {
    if (!terms || terms.length === 0) return { matched: 0, count: 0, sum: 0, min: null, max: null };
    const ixs = this._deviceIndexes(path, terms.map((t) => t.field).concat(field === undefined || field === null ? [] : [field]), "aggregateWhere");
    this.lastPath = "device";
    const native = terms.map((t, k) => [ixs[k].deviceField, Math.ceil(t.min), Math.floor(t.max)]);
    const r = this.graph.scanAggregate(native, { measure: ixs.length > terms.length ? ixs[terms.length].deviceField : null });
    return { matched: r.nMatch, count: r.n, sum: r.sum, min: r.min, max: r.max };
  }

  /**
   * "count users by role" in one call (the reference: one count(path, field, value) per distinct value, src/bullet-query.js:293-313): a Map from each
   * integer value of `field` in [min, max] that occurs among the children of path to the number of children that carry it.
   */
  countBy(path, field, min, max) {
    const [ix] = this._deviceIndexes(path, [field], "countBy");
    this.lastPath = "device";
    const out = new Map();
    const lo = Math.ceil(min), hi = Math.floor(max);
    for (let base = lo; base <= hi; base += 65536) {          // windows of BMX_AGG_MAX_GROUPS values
      const n = Math.min(65536, hi - base + 1);
      const recs = this.graph.scanAggregate([[ix.deviceField, base, base + n - 1]], { group: ix.deviceField, groupLo: base, nGroups: n });
      for (let g = 0; g < n; g++) if (recs[g].nMatch) out.set(base + g, recs[g].nMatch);
    }
    return out;
  }

  /**
   * "The 20 highest scores", "the next page of products by price between 10 and 50" (docs/querying.md: fields used for sorting are the first reason to index;
   * the reference answers with range() and a sort of every match on the host): the first k children of path ordered by `field`, then by the 64-bit hash of
   * their path (js/hash.js pathId, the device's node id) — a total order, so pages never overlap.
   * opts: desc (value descending, hash still ascending), min / max (bounds on `field`), where ([{field, min, max}]: further terms, as filterWhere takes them),
   * after (the .cursor of the page before). -> the BulletNodes in order, as an array that also carries .cursor ([id, value] of its last record, null when
   * empty: the next page's `after`), .values and .nEligible (children that satisfy the terms and lie behind `after`).
   * An integer index answers on the device (bmx_scan_top); an index that lives on the host (non-integer values) applies the same order in JS.
   */
  top(path, field, k, opts = {}) {
    const ix = this._fresh(path, field);
    this.lastPath = ix.kind;
    const where = opts.where || [];
    const desc = !!opts.desc, after = opts.after || null;
    if (ix.kind === "device") {
      const ixs = this._deviceIndexes(path, where.map((t) => t.field), "top");
      const lo = opts.min === undefined ? -Infinity : Math.ceil(opts.min), hi = opts.max === undefined ? Infinity : Math.floor(opts.max);
      const native = [[ix.deviceField, lo, hi]].concat(where.map((t, j) => [ixs[j].deviceField, Math.ceil(t.min), Math.floor(t.max)]));
      return this._topFromDevice(ix, this.graph.scanTop(native, k, { desc, after }));
    }
    // host index: the same total order in JS
    const base = this.bullet._getData(path);
    const rows = [];
    ix.values.forEach((v, i) => {
      if (opts.min !== undefined && !(v >= opts.min)) return;
      if (opts.max !== undefined && !(v <= opts.max)) return;
      if (where.length) {
        const child = base[ix.paths[i].slice(path.length + 1)];
        for (const t of where) { const x = child && child[t.field]; if (x === null || x === undefined || !(x >= t.min && x <= t.max)) return; }
      }
      rows.push(i);
    });
    return this._topOnHost(ix, rows, k, desc, after);
  }

  /* the answer of top() / whereTop(): the nodes, carrying .values, .cursor and .nEligible */
  _topDone(nodes, values, cursor, nEligible) { nodes.values = values; nodes.cursor = cursor; nodes.nEligible = nEligible; return nodes; }

  /* r: {ids, vals, nEligible} of scanTop / whereTop on the index ix */
  _topFromDevice(ix, r) {
    const n = r.ids.length;
    const values = Array.from(r.vals, Number);
    let nodes;
    if (ix.source === "device") {
      const u32 = new Uint32Array(r.ids.buffer, r.ids.byteOffset, n * 2);
      nodes = [];
      for (let i = 0; i < n; i++) nodes.push(this.bullet.get(this.graph.keys.pathOf(u32[2 * i], u32[2 * i + 1])));
    } else nodes = this._nodes(ix, this._ordinals(ix, r.ids));
    return this._topDone(nodes, values, n ? [r.ids[n - 1], values[n - 1]] : null, r.nEligible);
  }

  /* ordinals: the selected children of the host mirror of ix -> the first k behind `after` by (value, hash of the path) */
  _topOnHost(ix, ordinals, k, desc, after) {
    const rows = ordinals.map((i) => { const [l, h] = pathId(ix.paths[i]); return { i, v: ix.values[i], id: (BigInt(h) << 32n) | BigInt(l) }; });
    const cmp = (a, b) => (desc ? cmpVal(b.v, a.v) : cmpVal(a.v, b.v)) || (a.id < b.id ? -1 : a.id > b.id ? 1 : 0);
    const eligible = after ? rows.filter((r) => cmp(r, { v: after[1], id: BigInt(after[0]) }) > 0) : rows;
    eligible.sort(cmp);
    const page = eligible.slice(0, k);
    const last = page.length ? page[page.length - 1] : null;
    return this._topDone(this._nodes(ix, page.map((r) => r.i)), page.map((r) => r.v), last ? [last.id, last.v] : null, eligible.length);
  }

  /**
   * aggregateWhere() for a boolean program (bmx_where_aggregate): over the children of path that where(path, clauses, {over}) selects, the number matched, and
   * count / sum / min / max of opts.field over those that carry it. -> {matched, count, sum, min, max} as aggregateWhere gives it. With
   * opts.groupBy = {field, min, max}: a Map from each integer value of groupBy.field in [min, max] that occurs among the selected children to that record
   * ("count users by role among the active non-admins"), asked in windows of 65536 values as countBy does.
   * The device answers; an index involved that lives on the host throws BMX_NOT_DEVICE_INDEX, as aggregateWhere does.
   */
  whereAggregate(path, clauses, opts = {}) {
    if (opts.over === undefined || opts.over === null) throw new TypeError("bmx: whereAggregate needs opts.over, the field that defines the universe");
    const groupBy = opts.groupBy || null;
    const zero = () => (groupBy ? new Map() : { matched: 0, count: 0, sum: 0, min: null, max: null });
    if (!clauses || clauses.length === 0) return zero();
    const { base, native } = this._whereProgram(path, clauses, opts.over);
    const hasMeasure = opts.field !== undefined && opts.field !== null;
    const extra = native ? this._deviceIndexes(path, (hasMeasure ? [opts.field] : []).concat(groupBy ? [groupBy.field] : []), "whereAggregate") : null;
    if (!native) {
      const err = new Error("bmx: whereAggregate needs integer-valued fields on every literal");
      err.code = "BMX_NOT_DEVICE_INDEX";
      throw err;
    }
    this.lastPath = "device";
    if (native.length === 0) return zero();
    const measure = hasMeasure ? extra[0].deviceField : null;
    const rec = (r) => ({ matched: r.nMatch, count: r.n, sum: r.sum, min: r.min, max: r.max });
    if (!groupBy) return rec(this.graph.whereAggregate(base.deviceField, native, { measure }));
    const group = extra[extra.length - 1].deviceField;
    const out = new Map();
    const lo = Math.ceil(groupBy.min), hi = Math.floor(groupBy.max);
    for (let g0 = lo; g0 <= hi; g0 += 65536) {                // windows of BMX_AGG_MAX_GROUPS values
      const n = Math.min(65536, hi - g0 + 1);
      const recs = this.graph.whereAggregate(base.deviceField, native, { measure, group, groupLo: g0, nGroups: n });
      for (let g = 0; g < n; g++) if (recs[g].nMatch) out.set(g0 + g, rec(recs[g]));
    }
    return out;
  }

  /**
   * top() for a boolean program (bmx_where_top): the first k of the children that where(path, clauses, {over}) selects, ordered by the value of `over`, then
   * by the 64-bit hash of their path ("the 20 youngest users who are not admins": over = "age"). opts: over (required), desc, after (the .cursor of the page
   * before). -> the BulletNodes in order, carrying .cursor, .values and .nEligible like top().
   * When every index involved is an integer index the device answers; when one lives on the host, where()'s literal truth and top()'s comparator run in JS.
   */
  whereTop(path, clauses, k, opts = {}) {
    if (opts.over === undefined || opts.over === null) throw new TypeError("bmx: whereTop needs opts.over, the field that defines the universe and the order");
    const desc = !!opts.desc, after = opts.after || null;
    if (!clauses || clauses.length === 0) return this._topDone([], [], null, 0);
    const { norm, base, native } = this._whereProgram(path, clauses, opts.over);
    if (native) {
      this.lastPath = "device";
      if (native.length === 0) return this._topDone([], [], null, 0);
      return this._topFromDevice(base, this.graph.whereTop(base.deviceField, native, k, { desc, after }));
    }
    const selected = this._whereHost(path, norm, base);
    this.lastPath = "host";
    return this._topOnHost(base, selected, k, desc, after);
  }

  /**
   * where() that also reads (bmx_where_rows): the children that where(path, clauses, {over}) selects, each with the values of fieldNames — what
   * filter(path, fn) followed by .value() on every node, or map(path, fn) (src/bullet-query.js:322-333), does on the host.
   * opts: over (required), cap (children per page; left out: all of them), start (the .next of the page before).
   * opts.clocks: the answer also carries clocks[i] = {name: clock} — the clock of the field's row in its index (see where()), undefined where there is no row.
   * -> {paths, rows, nMatch, next}: paths[i] is the path of the i-th delivered child, rows[i] = {name: value} with undefined for a cell without data (the
   * field is absent, null or deleted); nMatch counts the selected children from the cursor on; next is the cursor of the following page, null behind the last.
   * When every index involved — the program's and the projected fields' — is an integer index the device answers, in index order of `over`; a cursor is bound
   * to the layout of that index and a page asked with a cursor of an older layout throws BMX_STALE_CURSOR (start over). When an index lives on the host
   * (strings, booleans) the same answer comes from where()'s host evaluation and a projection from the store, in the scan order of `over`'s index.
   */
  whereRows(path, clauses, fieldNames, opts = {}) {
    if (opts.over === undefined || opts.over === null) throw new TypeError("bmx: whereRows needs opts.over, the field that defines the universe");
    const names = Array.from(new Set(fieldNames));
    const withClocks = !!opts.clocks;          // also clocks[i] = {name: clock of the field's row, undefined where there is none}
    let clocks = withClocks ? [] : undefined;
    const done = (paths, rows, nMatch, next) => (withClocks ? { paths, rows, clocks, nMatch, next } : { paths, rows, nMatch, next });
    if (!clauses || clauses.length === 0) return done([], [], 0, null);
    const { norm, base, native } = this._whereProgram(path, clauses, opts.over);
    const kinds = names.map((f) => this._fieldKind(path, f));
    const cap = opts.cap === undefined || opts.cap === null ? null : opts.cap;
    const start = opts.start || null;
    if (native && kinds.every((k) => k !== "host")) {
      this.lastPath = "device";
      if (native.length === 0) return done([], [], 0, null);
      const present = names.filter((f, j) => kinds[j] === "device");       // (a field no child carries is undefined everywhere: nothing to ask)
      if (present.length > 8) throw new RangeError("bmx: whereRows projects 8 distinct fields at most");
      const r = this.graph.whereRows(base.deviceField, native, present.map((f) => this._fresh(path, f).deviceField), { cap, start: start ? start.at : null, ts: withClocks });
      if (start && start.layout !== r.layout) {
        const err = new Error("bmx: the cursor belongs to an older layout of the index; start over");
        err.code = "BMX_STALE_CURSOR";
        throw err;
      }
      const n = r.ids.length;
      const u32 = new Uint32Array(r.ids.buffer, r.ids.byteOffset, n * 2);
      const paths = new Array(n), rows = new Array(n);
      const NONE = -(2n ** 63n);
      for (let i = 0; i < n; i++) {
        paths[i] = this.graph.keys.pathOf(u32[2 * i], u32[2 * i + 1]);
        const row = {};
        for (const f of names) row[f] = undefined;
        present.forEach((f, j) => { const v = r.vals[j][i]; if (v !== NONE) row[f] = Number(v); });
        rows[i] = row;
        if (withClocks) {
          const ck = {};
          for (const f of names) ck[f] = undefined;
          present.forEach((f, j) => { const c = r.ts[j][i]; if (c >= 0n) ck[f] = Number(c); });      // (NO_CLOCK = -1: no row)
          clocks.push(ck);
        }
      }
      const more = r.nMatch > n;
      return done(paths, rows, r.nMatch, more ? { at: this.graph.comm ? [r.nextShard, r.nextPos] : r.nextPos, layout: r.layout } : null);
    }
    const selected = this._whereHost(path, norm, base);
    this.lastPath = "host";
    const from = start ? start.at : 0;
    const page = selected.slice(from, cap === null ? undefined : from + cap);
    const store = this.bullet._getData(path);
    const paths = page.map((i) => base.paths[i]);
    const rows = paths.map((p) => {
      const child = store[p.slice(path.length + 1)];
      const row = {};
      for (const f of names) { const v = child ? child[f] : undefined; row[f] = v === null ? undefined : v; }
      return row;
    });
    if (withClocks) clocks = rows.map((row) => { const ck = {}; for (const f of names) ck[f] = row[f] === undefined ? undefined : HOST_CLOCK; return ck; });
    const end = from + page.length;
    return done(paths, rows, selected.length - from, end < selected.length ? { at: end, layout: 0 } : null);
  }

  filter(path, fn) {
    const base = this.bullet._getData(path);
    const out = [];
    if (typeof base === "object" && base !== null) {
      for (const [k, v] of Object.entries(base)) if (fn(v, k)) out.push(this.bullet.get(`${path}/${k}`));
    }
    return out;
  }

  map(path, fn) {
    const base = this.bullet._getData(path);
    const out = [];
    if (typeof base === "object" && base !== null) {
      for (const [k, v] of Object.entries(base)) out.push(fn(v, k));
    }
    return out;
  }

  find(path, fn) {
    const base = this.bullet._getData(path);
    if (typeof base === "object" && base !== null) {
      for (const [k, v] of Object.entries(base)) if (fn(v, k)) return this.bullet.get(`${path}/${k}`);
    }
    return null;
  }

  close() {
    if (this._ownsGraph && this._graph) this._graph.close();
    this._graph = null;
  }
}

module.exports = GpuQuery;
