"""The build gate of the field-to-field literals: register, scratch and occupancy figures of every kernel that embeds the where program (PredWhere), before and
after, from two compiler logs. No GPU needed.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Iinclude -Rpass-analysis=kernel-resource-usage -c -o /dev/null bullet-js_amd/csrc/bmx.hip 2> LOG

once on the parent commit and once on this tree, then

  python bench_micro/where_diff_resources.py BEFORE.log AFTER.log ["what the tree adds" ["what the new kernels run"]] > profiles/where_diff_resources.txt

Exit status 1 if a kernel gained scratch or lost a wave of occupancy."""
import re
import subprocess
import sys

FAMILIES = ["k_scan_mask", "k_scan_emit", "k_where_agg", "k_group_sweep", "k_watch_mask", "k_rows_emit", "k_semi_build", "k_join_group_sweep", "k_jrows_emit",
            "k_upd_emit", "k_mgroup_sweep", "k_reach_prepare", "k_first_sweep", "k_quant0"]
CLOCKED = ("k_first_sweep", "k_group_sweep", "k_join_build", "k_join_group_sweep", "k_jrows_build", "k_mgroup_sweep", "k_reach_prepare", "k_reach_seed",
           "k_semi_build", "k_where_agg")      # families whose last template argument says whether the clock literals are compiled in
EXPR = {"k_where_agg": 4, "k_group_sweep": 3, "k_quant0": 4}      # families whose last template argument (of this many) says whether the measure is computed (bmx_expr.h)
KEYS = [("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy")]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    try:
        return dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(pretty):
    return re.sub(r"^void bmx::", "", pretty.replace("(anonymous namespace)::", "")).split("(")[0]


def family(s):
    m = re.match(r"(k_[a-z0-9_]+)", s)
    return m.group(1) if m else None


def embeds(n, s):
    return "PredWhere" in n or family(s) in ("k_scan_mask", "k_scan_emit", "k_rows_emit", "k_jrows_emit", "k_upd_emit")      # (every mask pass: some wrap the program)


def table(path):
    """short demangled name -> figures, of the kernels that take the program (and of the listed emit kernels, which read the mask pass's words instead)"""
    raw = parse(path)
    names = [n for n in raw if re.match(r"_ZN3bmx\d+k_", n)]
    pretty = demangle(names)
    return {short(pretty[n]): raw[n] for n in names if embeds(n, short(pretty[n]))}


def before_name(s):
    """the parent's name of a kernel of this tree; None: the kernel is new. PredWhere's second argument (the pair path compiled in) defaults to true; the
    kernels built both ways carry it as `false` when it is off, and their `true` build runs programs with a pair only, which the parent refuses."""
    # A tree with the computed measures: the build without them is held against the parent's build of the same name less the flag; the build with them is new.
    if family(s) in EXPR and s.count(",") + 1 == EXPR[family(s)]:
        if s.endswith(", true>"):
            return None
        return re.sub(r", false>$", ">", s)      # (the parent of that tree has the clock literals: its names are this tree's less the last flag)
    # A tree with the clock literals: every build of a kernel is held against the parent's build that ran the same programs.
    #   Pred{RowsFrom,JRowsFrom,Semi,Upd}<T, CLOCKS>        -> <T>           (the parent had the one build)
    #   k_x<..., CLOCKS> of the CLOCKED families             -> k_x<...>      (the same)
    #   k_scan_mask<PredWhere<T, PAIRS, CLOCKS>, ...>        -> <T, true>     (the parent's id scan had the one build, pair path in it, for every program;
    #                                                                          so <T, false, false>, the plain programs' build, shows fewer registers)
    #   k_watch_mask<PredWhere<T, PAIRS, CLOCKS>>            -> <T, PAIRS>    (built both ways by the parent already)
    t = re.sub(r"(Pred(?:RowsFrom|JRowsFrom|Semi|Upd)<\w+), (?:true|false)>", r"\1>", s)
    if family(t) in CLOCKED:
        t = re.sub(r", (?:true|false)>$", ">", t)
    t = re.sub(r"PredWhere<(\w+), (true|false), (?:true|false)>", (lambda m: "PredWhere<%s, true>" % m.group(1)) if family(t) == "k_scan_mask" else r"PredWhere<\1, \2>", t)
    if t != s:
        return t
    if family(s) in ("k_quant0", "k_where_top0"):
        return re.sub(r", false>$", ">", s) if s.endswith(", false>") else None
    if "PredWhere<int, false>" in s or "PredWhere<long, false>" in s:
        return re.sub(r"PredWhere<(\w+), false>", r"PredWhere<\1>", s)
    if family(s) == "k_watch_mask":
        return None
    return re.sub(r"PredWhere<(\w+), true>", r"PredWhere<\1>", s)


def main(before_path, after_path, what="field-to-field literals", new="programs with a field pair only"):
    before, after = table(before_path), table(after_path)
    bad, seen = [], set()
    print("kernel resource usage, gfx950, -O3: before (parent commit) -> after (%s)" % what)
    print("%-9s %-9s %-8s %-10s kernel" % tuple(k for _, k in KEYS))
    for s in sorted(after):
        seen.add(family(s))
        a, b = after[s], before.get(s) or before.get(before_name(s) or "")      # (a parent that builds kernels both ways already knows this tree's names)
        cells = ["%s->%d" % ("new" if b is None else b[k], a[k]) for k, _ in KEYS]
        print("%-9s %-9s %-8s %-10s %s%s" % (*cells, s, "" if b else "   (%s)" % new))
        if b is not None and (a[KEYS[2][0]] > b[KEYS[2][0]] or a[KEYS[3][0]] < b[KEYS[3][0]]):
            bad.append(s)
    missing = [f for f in FAMILIES if f not in seen]
    print("listed families without a kernel in the log: %s" % (", ".join(missing) or "none"))
    print("kernels that gained scratch or lost a wave of occupancy: %s" % (", ".join(bad) or "none"))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
