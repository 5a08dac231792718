"""The per-proof hoists that a trace's constant columns allow, on the CPU: the round-1 prefix of the trace leaf
hash (xfg-stark_amd/csrc/blake3.hpp b3_row7_prefix / b3_hash_row7) and the uniform part of the constraint sums
(xfg-stark_amd/csrc/air.hpp ce_uniform_of / ce_live_sums).

tests/sanitize/leaf_prefix.cpp, built host-only with ASan + UBSan by `make -C xfg-stark_amd sanitize`, checks for
all 128 constant-column masks that the resumed hash equals b3_hash_elems<7>, that the planner's uniform-G set is
the one brute force finds, and that uniform part + per-point rest equals the full constraint sums in both fields
on constants that do not satisfy the AIR (see its header). Here it is run and its summary line read back."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "xfg-stark_amd", "build", "asan", "leaf_prefix")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")


def test_prefix_and_uniform_part_hold_for_every_mask():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "xfg-stark_amd"), "sanitize"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.fullmatch(r"leaf_prefix ok: masks=(\d+) reps=(\d+) hoisted_nonzero=(\d+)\s*", r.stdout)
    assert m, r.stdout[-400:]
    masks, reps, hoisted = map(int, m.groups())
    assert masks == 128 and reps >= 1
    # every mask but the empty one hoists at least one non-zero term in each field
    assert hoisted >= 2 * 127 * reps
