"""The build gate of a change that must leave every kernel as it was: the figures of ALL kernels of two compiler logs, held against each other by mangled
name. No GPU needed. The logs are made as where_diff_resources.py says (its parse() reads them), once on the parent commit and once on this tree, then

  python bench_micro/kernel_resources.py BEFORE.log AFTER.log > profiles/kernel_sharing_resources.txt

Prints every kernel whose VGPR or SGPR count, or count of spilled registers (scalar registers kept in lanes of a vector register: no scratch), moved.
Exit status 1 on a new or missing kernel name, a scratch gain, an occupancy loss or an LDS change."""
import sys

from where_diff_resources import demangle, parse, short

KEYS = [("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"),
        ("LDS Size [bytes/block]", "LDS"), ("SGPRs Spill", "SGPR spill"), ("VGPRs Spill", "VGPR spill")]


def main(before_path, after_path):
    before, after = parse(before_path), parse(after_path)
    pretty = demangle(sorted(set(before) | set(after)))
    new, gone = sorted(set(after) - set(before)), sorted(set(before) - set(after))
    moved, bad = [], []
    for n in sorted(set(before) & set(after)):
        b, a = before[n], after[n]
        if any(a[k] != b[k] for k, _ in KEYS):
            moved.append(n)
        if a[KEYS[2][0]] > b[KEYS[2][0]] or a[KEYS[3][0]] < b[KEYS[3][0]] or a[KEYS[4][0]] != b[KEYS[4][0]]:
            bad.append(n)
    print("kernel resource usage, gfx950, -O3: before (parent commit) -> after (this tree), every kernel by mangled name")
    print("kernels: %d before, %d after, %d with a figure that moved" % (len(before), len(after), len(moved)))
    print("%-9s %-9s %-8s %-10s %-14s %-11s %-11s kernel" % tuple(k for _, k in KEYS))
    for n in moved:
        cells = ["%d->%d" % (before[n][k], after[n][k]) if before[n][k] != after[n][k] else "%d" % after[n][k] for k, _ in KEYS]
        print("%-9s %-9s %-8s %-10s %-14s %-11s %-11s %s" % (*cells, short(pretty[n])))
    print("new kernel names: %s" % (", ".join(short(pretty[n]) for n in new) or "none"))
    print("missing kernel names: %s" % (", ".join(short(pretty[n]) for n in gone) or "none"))
    print("kernels that gained scratch, lost a wave of occupancy or changed LDS size: %s" % (", ".join(short(pretty[n]) for n in bad) or "none"))
    return 1 if new or gone or bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
