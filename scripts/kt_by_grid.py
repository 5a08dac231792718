"""Mean isolated duration (us) per (kernel, grid) of the NTT and constant-column kernels in kernel traces of
scripts/stage_kernels.py (one 64-proof unit, every kernel alone on the GPU): the trace's launch sets
(grid y = 448 polynomials x cosets) beside the composition / DEEP ones (64 polynomials), so that a launch
set whose blocks mostly return at once can be held against a dense one with as many live polynomials.
usage: kt_by_grid.py DIR [DIR2 ...]   (each DIR: one rocprofv3 --kernel-trace output tree)"""
import collections, csv, glob, sys

for d in sys.argv[1:]:
    acc = collections.defaultdict(list)
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"].split("(")[0]
            if "ntt_pass" in k or "const_" in k:
                wg = int(r["Workgroup_Size_X"])
                key = (k[:44], int(r["Grid_Size_X"]) // wg, int(r["Grid_Size_Y"]))
                acc[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(d)
    for key in sorted(acc):
        v = sorted(acc[key])
        print(f"  {key[0]:44s} blocks {key[1]:5d} x {key[2]:5d}  launches {len(v):3d}  mean {sum(v) / len(v):8.1f}  min {v[0]:8.1f}")
