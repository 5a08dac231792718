"""The proof-of-work search planner (xfg-stark_amd/csrc/grind_plan.hpp) and the seed fixture, on the CPU.

tests/sanitize/grind_plan.cpp, built host-only with ASan + UBSan by `make -C xfg-stark_amd sanitize`, walks
grinding factor 0..32 x B = 1..4096 x four compute-unit counts and checks the planner's invariants itself
(grid within its cap and within the expected work, chunk_log in range, max_nonce without a shift overflow,
chunks tiling [first, max_nonce]; see its header). Here its printed plans of the prover's shapes are read back,
the library is asked for the two entry points, and tests/golden/grind_seeds.json is re-derived with
tests/grind_ref.py."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import grind_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "xfg-stark_amd", "build", "asan", "grind_plan")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")
LINE = re.compile(r"grind=(\d+) B=(\d+) cus=(\d+) : chunk_log=(\d+) blocks=(\d+) block=(\d+) max_nonce=(\d+)")


@pytest.fixture(scope="module")
def plans():
    """{(grind, B): (chunk_log, blocks, block, max_nonce)} at 256 compute units"""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "xfg-stark_amd"), "sanitize"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        g, B, cus, cl, blocks, block, mx = map(int, LINE.fullmatch(line).groups())
        assert cus == 256
        out[(g, B)] = (cl, blocks, block, mx)
    return out


def test_planner_invariants_hold_over_its_domain(plans):
    assert len(plans) == 33 * 4


def test_plans_of_the_provers_shapes(plans):
    """the rule at the top of the header, worked by hand"""
    for (g, B), (cl, blocks, block, mx) in plans.items():
        assert mx == 1 << (g + 8) and block == 256
        assert blocks == min(2048, max(1, -(-(B << g) // 1024)))
        per = max(1, blocks // B)
        assert cl == min(14, max(8, g - 2 - (per - 1).bit_length()))
    assert plans[(4, 32)][:2] == (8, 1)        # 512 hashes: one block
    assert plans[(16, 32)][:2] == (8, 2048)    # 64 blocks per proof: 2^14 nonces in flight of 2^16 expected
    assert plans[(20, 64)][:2] == (13, 2048)
    assert plans[(20, 1)][:2] == (8, 1024)
    assert plans[(32, 1)][:2] == (14, 2048)


def test_library_exports_the_search_entry_points():
    import xfgstark
    lib = C.CDLL(xfgstark.LIB_PATH)
    assert hasattr(lib, "xfg_debug_grind") and hasattr(lib, "xfg_grind_probe")
    assert hasattr(xfgstark.XfgBurnMintProver, "debug_grind") and hasattr(xfgstark.XfgBurnMintProver, "grind_probe")
    # without a context the probe reports an argument error and touches nothing
    assert lib.xfg_grind_probe(None, None, None, None) == 9


def test_seed_fixture_is_what_its_generator_says():
    """every recorded nonce is the smallest one of its seed at its factor, and the targets are the chunk
    positions the GPU test needs"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "grind_seeds.json")))
    c = fx["chunk"]
    assert c == 256
    assert [s["nonce"] for s in fx["seeds"]] == [1, 2, c, c + 1, 2 * c, 2 * c + 1, 3 * c, 3 * c + 1, 6 * c + 1]
    for s in fx["seeds"]:
        assert 8 <= s["grind"] <= 11
        assert G.min_nonce(bytes.fromhex(s["seed"]), s["grind"]) == s["nonce"]
