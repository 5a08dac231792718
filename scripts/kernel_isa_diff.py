"""Which kernels' machine code differs between two builds: python3 scripts/kernel_isa_diff.py DIR_A DIR_B,
each a directory of gfx950 assembly listings, one per translation unit (the Makefile's flags plus
--cuda-device-only -S). For every .amdhsa_kernel symbol, wherever in its directory it lies, it compares the
instruction text between the symbol's label and its .Lfunc_end and the .amdhsa_* descriptor lines (VGPRs, SGPRs,
LDS, scratch). Local labels .LBB<k>_<m> carry the function's index k within its file, which changes when a kernel
moves: k is dropped. A long branch's .Lpost_getpc<j> label counts the file's long branches, so j changes as
well: inside a kernel the labels are renumbered from 0 in the order they first appear. Comments are dropped too.
Prints the counts and every differing or unmatched kernel by name; exit status 1 when there is one."""
import glob
import os
import re
import sys


def kernels(directory):
    """symbol -> (instruction lines, descriptor lines) over every .s file of the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        body, desc, cur, in_desc = {}, {}, None, None
        for line in lines:
            text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
            m = re.match(r"^(\w+):", text)
            if m and not text.startswith(".L"):  # labels inside a function are all local
                cur = m.group(1)
                body[cur] = []
            elif text.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and text:
                body[cur].append(text)
            if text.startswith(".amdhsa_kernel "):
                in_desc = text.split()[1]
                desc[in_desc] = []
            elif text.startswith(".end_amdhsa_kernel"):
                in_desc = None
            elif in_desc is not None and text:
                desc[in_desc].append(text)
        for sym, d in desc.items():
            if sym in out:
                raise SystemExit(f"{sym} defined twice in {directory}")
            seen = {}
            renumber = lambda m: ".Lpost_getpc_%d" % seen.setdefault(m.group(0), len(seen))
            out[sym] = ([re.sub(r"\.Lpost_getpc\d+", renumber, t) for t in body[sym]], d, os.path.basename(path))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    differing = []
    for sym in both:
        what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if a[sym][i] != b[sym][i]]
        if what:
            differing.append((sym, what))
    moved = [s for s in both if a[s][2] != b[s][2]]
    print(f"kernels in {sys.argv[1]}: {len(a)}, in {sys.argv[2]}: {len(b)}")
    print(f"compared: {len(both)}  identical: {len(both) - len(differing)}  differing: {len(differing)}")
    print(f"only in the first: {len(only_a)}  only in the second: {len(only_b)}  in another file: {len(moved)}")
    for sym, what in differing:
        print(f"DIFFERS {sym} ({a[sym][2]} -> {b[sym][2]}): {', '.join(what)}")
    for sym in only_a:
        print(f"ONLY IN THE FIRST {sym} ({a[sym][2]})")
    for sym in only_b:
        print(f"ONLY IN THE SECOND {sym} ({b[sym][2]})")
    for sym in moved:
        print(f"moved {sym}: {a[sym][2]} -> {b[sym][2]} ({len(a[sym][0])} lines)")
    sys.exit(1 if differing or only_a or only_b else 0)


if __name__ == "__main__":
    main()
