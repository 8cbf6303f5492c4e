#!/usr/bin/env python3
"""The loops of one kernel in a gfx950 assembly listing, with their instruction counts by class - how DESIGN.md section 4.12 compares
the inner four-column loops of `levenshtein_fuzzy_matches_count_kernel` and `levenshtein_fuzzy_scan_kernel`.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S stringzilla_amd/csrc/hip/myers_fuzzy_scan.hip -o scan.s
    python scripts/loop_opcodes.py scan.s levenshtein_fuzzy_scan_kernel

One line per backward branch: first line, last line, instructions, VALU (`v_*`), LDS (`ds_*`), global memory (`global_*`, `flat_*`),
scalar (`s_*`).  A loop is the stretch from a label to a later branch back to it, so nested loops appear inside their parents.  The
walk of `listed_walk` shows per width as a pair: the unpredicated four-column loop (without and with its look-ahead load), then the
predicated one.
"""
import re
import sys

if len(sys.argv) != 3:
    sys.exit(__doc__)
lines = open(sys.argv[1]).read().split("\n")
starts = [at for at, line in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(sys.argv[2]), line)]
if not starts:
    sys.exit(f"no kernel named like {sys.argv[2]} in {sys.argv[1]}")
end = next(at for at in range(starts[0], len(lines)) if lines[at].startswith(".Lfunc_end"))
labels = {}
print("first last instructions valu lds global scalar")
for at in range(starts[0], end):
    label = re.match(r"^(\.LBB\d+_\d+):", lines[at])
    if label:
        labels[label.group(1)] = at
    branch = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[at])
    if not branch or branch.group(1) not in labels:
        continue
    body = [line.strip() for line in lines[labels[branch.group(1)]:at + 1] if line.startswith("\t") and not line.strip().startswith((".", ";"))]
    count = lambda *prefixes: sum(1 for line in body if line.startswith(prefixes))
    print(labels[branch.group(1)] + 1, at + 1, len(body), count("v_"), count("ds_"), count("global_", "flat_"), count("s_"))
