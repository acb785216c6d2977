"""Compare kernel resource usage between two builds.

    python tools/kernel_resources_diff.py BASE.txt HEAD.txt [HEAD2.txt ...]

Each file is the stderr of a gfx950 compile with
-Rpass-analysis=kernel-resource-usage.  Every kernel of BASE must appear
exactly once in the HEAD files together, with the same SGPRs, VGPRs, AGPRs,
scratch, spills and LDS.  Kernels whose name contains `sort_big` are listed
and compared as a set of resource rows, not by name (template instances may
differ in name and number).  Exit status 1 on any difference.
"""

import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def parse(path):
    out, name = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out.append((name, {}))
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name and m.group(1) in FIELDS:
            out[-1][1][m.group(1)] = m.group(2)
    return out


def main():
    base = parse(sys.argv[1])
    head = [k for p in sys.argv[2:] for k in parse(p)]
    bad = 0
    skip = lambda n: "sort_big" in n
    seen = {}
    for n, r in head:
        seen.setdefault(n, []).append(r)
    for n, r in base:
        if skip(n):
            continue
        got = seen.get(n, [])
        if len(got) != 1:
            print(f"{n}: {len(got)} times in head")
            bad += 1
        elif got[0] != r:
            print(f"{n}: {r} -> {got[0]}")
            bad += 1
    names = {n for n, _ in base}
    for n in seen:
        if n not in names and not skip(n):
            print(f"{n}: only in head")
            bad += 1
    # the rank sorts: names differ, so the distinct resource rows must be the same
    rows = [{tuple(sorted(r.items())) for n, r in ks if skip(n)} for ks in (base, head)]
    for who, ks in (("base", base), ("head", head)):
        for n, r in ks:
            if skip(n):
                print(f"({who} sort) {n}: {r}")
    if rows[0] != rows[1]:
        print(f"rank sorts differ: {len(rows[0] ^ rows[1])} resource rows in one build only")
        bad += 1
    print(f"{len(base)} kernels in base, {len(head)} in head, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
