"""Regenerates ntt_launches.json: the two ntt_pass_* dispatches (kernel, grid, workgroup, LDS) of every
debug_lde / debug_interpolate call over the shapes below, as a kernel trace of the library records them.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tests/golden/make_ntt_launches.py run OUT/shapes.json
    python tests/golden/make_ntt_launches.py convert OUT/*/*_kernel_trace.csv OUT/shapes.json [LDS.txt] > tests/golden/ntt_launches.json

The committed file was recorded from the commit before the launch planner (csrc/ntt_plan.hpp) existed;
tests/test_ntt_plan.py holds the planner to it. The trace's LDS_Block_Size counts static LDS only (0 for
these kernels), so the dynamic LDS bytes of that commit were logged by a build of it patched to append the
`lds` argument of every NTT launch to a file (LDS.txt: one number per dispatch, in order, same run of
shapes); without the file the trace's figure is kept. The patch to that commit's csrc/ntt.hip, in full:

    static void xfg_log_lds(size_t lds) {              // in front of "// ---- dispatch"; #include <cstdio>
        if (const char* f = getenv("XFG_NTT_LDS_LOG")) {
            FILE* fp = fopen(f, "a");
            fprintf(fp, "%zu\\n", lds);
            fclose(fp);
        }
    }
    XFG_NTT_LAUNCH:                 xfg_log_lds(lds); before hipLaunchKernelGGL(KERNEL, ...)
    ntt_pass_a_r1024 / _b_r1024:    xfg_log_lds(la); xfg_log_lds(lb); before the two launches
    ntt_pass_a_cos2 / ntt_pass_a_cos: xfg_log_lds(lds_a); after a.tq_b = 1;
    ntt_pass_b_pers:                xfg_log_lds(lds_b); before its launch
    ntt_pass_b_tq:                  xfg_log_lds(l); before its launch

and the run: XFG_NTT_LDS_LOG=LDS.txt python tests/golden/make_ntt_launches.py run shapes.json (no profiler)."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shapes():
    s = [("fwd", logn, blowup, 1) for logn in range(3, 23) for blowup in (2, 4, 8, 16)]
    # launch sets on either side of the all-coset pass A's threshold (512 blocks of 16 columns)
    for logn, nps in ((16, (31, 32)), (17, (15, 16)), (18, (7, 8))):
        s += [("fwd", logn, blowup, npoly) for npoly in nps for blowup in (2, 4, 8, 16)]
    return s + [("inv", logn, 0, 1) for logn in range(3, 23)]


def run(out):
    sys.path.insert(0, os.path.join(ROOT, "xfg-stark_amd"))
    import numpy as np
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    for d, logn, blowup, npoly in shapes():
        z = np.zeros((npoly, 1 << logn), dtype=np.uint64)
        r = pr.debug_lde(z, 1 << logn, blowup) if d == "fwd" else pr.debug_interpolate(z, 1 << logn, False)
        assert not r.any(), (d, logn, blowup, npoly)
    pr.close()
    json.dump(shapes(), open(out, "w"))


def convert(trace, shape_file, lds_log=None):
    rows = [r for r in csv.DictReader(open(trace)) if "ntt_pass_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    sh = json.load(open(shape_file))
    assert len(rows) == 2 * len(sh), (len(rows), len(sh))
    if lds_log:
        logged = [int(x) for x in open(lds_log).read().split()]
        assert len(logged) == len(rows)
        for r, v in zip(rows, logged):
            r["LDS_Block_Size"] = v

    def disp(r):
        name = r["Kernel_Name"].replace("void ", "").replace("xfg::", "").split("(")[0]
        return {"kernel": name, "grid": [int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])],
                "workgroup": int(r["Workgroup_Size_X"]), "lds": int(r["LDS_Block_Size"])}
    calls = [{"dir": d, "logn": logn, "blowup": blowup, "npoly": npoly, "a": disp(rows[2 * i]), "b": disp(rows[2 * i + 1])}
             for i, (d, logn, blowup, npoly) in enumerate(sh)]
    # grid: work-items, as the trace reports it; lds: bytes of dynamic LDS asked for at the launch
    print(json.dumps({"grid_unit": "work-items", "lds_granule": 1, "compute_units": 256, "calls": calls},
                     separators=(",", ":")).replace('{"dir"', '\n{"dir"'))


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else convert(*sys.argv[2:5])
