"""The instantiation dispatchers (xfg-stark_amd/csrc/dispatch.hpp) and the one kernel launcher
(xfg-stark_amd/csrc/hip_util.hpp launch_kernel / XFG_LAUNCH), on the CPU.

tests/sanitize/launch_dispatch.cpp, a HIP program whose host code is built with ASan + UBSan by
`make -C xfg-stark_amd sanitize`, checks that every dispatcher reaches the right integral constants for every value
that has a kernel and throws std::invalid_argument, naming the value and calling nothing, for ext 0 and 3, fold 0, 1,
3 and 32, column counts 0, 3, 8 and log2 blowup 0 and 8 (see its header). Where the process can reach no GPU it also
sends two launches, which the runtime refuses, and checks that each throws a HipError with the kernel's name; with a
GPU in reach it sends none. Here it is run and its lines read back."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "xfg-stark_amd", "build", "asan", "launch_dispatch")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")


def test_dispatchers_refuse_what_has_no_kernel_and_a_refused_launch_names_its_kernel():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "xfg-stark_amd"), "sanitize"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    m = re.fullmatch(r"dispatch ok: (\d+)", lines[0])
    # 2 + 6 ext, 4 + 16 fold, 2 bool, 21 + 7 (columns, blowup), 9 + 24 refused pairs, 8 + 15 (ext, fold)
    assert m and int(m.group(1)) == 114, r.stdout[-400:]
    if lines[1:] == ["launcher: a GPU is in reach, no launch sent"]:
        assert os.path.exists("/dev/kfd")
    else:  # the reason is the runtime's own text, whatever it is; the name is the launcher's
        assert len(lines) == 3, r.stdout[-400:]
        assert re.fullmatch(r"launcher: launch of empty_kernel: .+", lines[1]), lines[1]
        assert re.fullmatch(r"launcher: launch of \(probe_kernel<2, true>\): .+", lines[2]), lines[2]
