#!/usr/bin/env python3
"""Per-kernel resource listing of a build: reads the compiler's -Rpass-analysis=kernel-resource-usage remarks (the
build's stderr, e.g. `make -C flink_amd/csrc EXTRA=-Rpass-analysis=kernel-resource-usage 2> build.log`) and prints one
line per kernel instantiation, sorted by name: SGPRs, VGPRs, AGPRs, scratch bytes per lane, occupancy in waves per
SIMD, spills and LDS bytes per block.  Two such listings compare with diff: line numbers and source positions are left
out, so only a kernel whose numbers moved (or that is new) shows.

    tools/kernel_resources.py build.log > listing.txt
    tools/kernel_resources.py --compare parent.txt this.txt     # exit 1 if a kernel of parent.txt moved or is gone
"""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"),
          ("LDS Size [bytes/block]", "lds")]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, res.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def listing(path):
    k = parse(path)
    dm = demangle(sorted(k))
    lines = []
    for name in sorted(k, key=lambda n: dm[n]):
        short = re.sub(r"\(anonymous namespace\)::", "", dm[name]).replace("  ", " ")
        lines.append(short + "  " + " ".join(f"{tag}={k[name].get(f, '?')}" for f, tag in FIELDS))
    return lines


def main(argv):
    if len(argv) == 4 and argv[1] == "--compare":
        a = dict(l.split("  ", 1) for l in open(argv[2]).read().splitlines() if l)
        b = dict(l.split("  ", 1) for l in open(argv[3]).read().splitlines() if l)
        moved = [n for n in a if b.get(n) != a[n]]
        for n in moved:
            print(f"MOVED {n}\n  parent: {a[n]}\n  this:   {b.get(n, '(gone)')}")
        print(f"{len(a)} kernels at the parent, {len(a) - len(moved)} identical, {len(moved)} moved or gone, "
              f"{len([n for n in b if n not in a])} new")
        return 1 if moved else 0
    if len(argv) != 2:
        print(__doc__)
        return 2
    print("\n".join(listing(argv[1])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
