"""The lane scheduler (xfg-stark_amd/csrc/unit_queue.hpp) and the host thread pool (csrc/host_pool.hpp), on the CPU.

tests/sanitize/unit_queue.cpp is plain C++ with its own main: it drives both with a dummy batch type and checks
exactly-once coverage, the halving rule (one worker, held workers, idle workers, the whole-units switch), pinned
units, a throwing work function, tickets / busy / drain / stop, and parallel_for from seven threads (see its
header). Here it is built with ASan + UBSan (`make -C xfg-stark_amd sanitize`) and with TSan
(`build/tsan/unit_queue`), and each binary is run directly: exit 0, nothing from a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "xfg-stark_amd")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78",
               TSAN_OPTIONS="halt_on_error=1:exitcode=79")


@pytest.mark.parametrize("target", ["build/asan/unit_queue", "build/tsan/unit_queue"])
def test_driver_is_clean_under_the_sanitizer(target):
    subprocess.run(["make", "-s", "-C", LIB, target], check=True)
    r = subprocess.run([os.path.join(LIB, target)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert r.stdout == "unit_queue ok\n"


def test_sanitize_target_builds_the_driver():
    subprocess.run(["make", "-s", "-C", LIB, "sanitize"], check=True)
    assert os.path.exists(os.path.join(LIB, "build", "asan", "unit_queue"))
