"""The verifiers' policy header (xfg-stark_amd/csrc/acceptable.hpp) under a sanitizer, on the CPU.

tests/sanitize/acceptable.cpp is plain C++ with its own main over that header alone: the conjectured security
level over the whole option domain check_options admits and on every header a parsed proof can state, set
membership at 1 and at 32 entries, the minimum's error text, the refusals, and the per-folding-factor ranges of
a GPU batch's queries over every split of small counts (see its header). Here it is built with ASan + UBSan
(`make -C xfg-stark_amd sanitize`) and the binary is run directly: exit 0, nothing from a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "xfg-stark_amd")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")
TARGET = "build/asan/acceptable"


def test_driver_is_clean_under_the_sanitizer():
    subprocess.run(["make", "-s", "-C", LIB, TARGET], check=True)
    r = subprocess.run([os.path.join(LIB, TARGET)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert r.stdout == "acceptable ok\n"


def test_sanitize_target_builds_the_driver():
    subprocess.run(["make", "-s", "-C", LIB, "sanitize"], check=True)
    assert os.path.exists(os.path.join(LIB, "build", "asan", "acceptable"))
