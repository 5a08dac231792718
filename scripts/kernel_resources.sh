#!/bin/bash
# CPU container: VGPR / SGPR / spill / scratch of the kernels whose demangled name matches PATTERN, from the
# .amdhsa metadata of the device assembly of the given csrc units (default: kernels merkle ntt, and columns where the tree has it).
#   scripts/kernel_resources.sh PATTERN [SRCROOT] [unit ...]
# SRCROOT: a tree holding xfg-stark_amd/csrc (default: this one; a `git archive` of another revision for
# the parent's side of a comparison, as profiles/r15/kernel_resources.txt)
set -e -o pipefail
PAT=${1:?pattern}
ROOT=${2:-$(cd "$(dirname "$0")/.." && pwd)}
shift || true
shift || true
UNITS=${*:-kernels merkle ntt $([ -f "$ROOT/xfg-stark_amd/csrc/columns.hip" ] && echo columns)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
TMP=$(mktemp -d /tmp/xfg_res.XXXX)
for u in $UNITS; do
    $HIPCC -O3 -std=c++17 --offload-arch=gfx950 --offload-device-only -S -o "$TMP/$u.s" "$ROOT/xfg-stark_amd/csrc/$u.hip"
done
python3 - "$PAT" "$TMP"/*.s <<'EOF'
import re, subprocess, sys
pat, rows = re.compile(sys.argv[1]), []
for path in sys.argv[2:]:
    cur, meta = {}, False
    for line in open(path):
        meta = meta or line.startswith("amdhsa.kernels:")
        # a kernel's own fields sit at four spaces (its arguments' deeper), in alphabetical order
        m = meta and re.match(r"    \.(name|sgpr_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_spill_count":
            rows.append(cur)
            cur = {}
names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), text=True,
                       capture_output=True, check=True).stdout.splitlines()
for r, nm in sorted(zip(rows, names), key=lambda x: x[1]):
    nm = re.sub(r"^void xfg::", "", nm).split("(")[0]
    if pat.search(nm):
        v = int(r["vgpr_count"])
        print(f"{nm:<46}vgpr {v:3d} sgpr {int(r['sgpr_count']):3d} spill {r['vgpr_spill_count']} scratch "
              f"{r['private_segment_fixed_size']} waves {min(8, 512 // ((v + 7) // 8 * 8))}")
EOF
rm -rf "$TMP"
