"""The NTT launch planner (xfg-stark_amd/csrc/ntt_plan.hpp) on the CPU.

tests/sanitize/ntt_plan.cpp, built host-only with ASan + UBSan by `make -C xfg-stark_amd sanitize`, walks the
planner's whole domain and checks its invariants itself (kernel list, unsupported sizes, LDS, grids, table
and LDS layouts; see its header). Here its printed plans are compared with tests/golden/ntt_launches.json,
the dispatches a kernel trace recorded on an MI355X from the commit before the planner existed, and with
the shapes the GPU parity tests run (tests/ntt_shapes.py)."""
import json
import os
import re
import subprocess

import pytest

import ntt_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "xfg-stark_amd", "build", "asan", "ntt_plan")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")
LINE = re.compile(r"(fwd|inv) logn=(\d+) logbeta=(\d+) npoly=(\d+) : (.*)")
PASS = re.compile(r"(\S.*?) grid=(\d+)x(\d+) block=(\d+) lds=(\d+)$")


@pytest.fixture(scope="module")
def plans():
    """{(direction, logn, logbeta, npoly): None (unsupported) or the two passes}"""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "xfg-stark_amd"), "sanitize"], check=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        d, logn, logbeta, npoly, rest = LINE.fullmatch(line).groups()
        passes = None
        if rest != "unsupported":
            passes = []
            for part in rest.split(" ; "):
                name, gx, gy, block, lds = PASS.fullmatch(part).groups()
                passes.append(dict(kernel=name, grid=[int(gx), int(gy)], workgroup=int(block), lds=int(lds)))
        out[(d, int(logn), int(logbeta), int(npoly))] = passes
    return out


def test_unsupported_sizes(plans):
    """sizes 2 and 4 and sizes from 2^23 have no kernel, in either direction; everything between has"""
    bad = {(d, logn) for (d, logn, _, _), p in plans.items() if p is None}
    assert bad == {(d, logn) for d in ("fwd", "inv") for logn in (1, 2, 23, 24)}
    assert {logn for (_, logn, _, _), p in plans.items() if p is not None} == set(range(3, 23))


def test_plans_equal_recorded_launches(plans):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "ntt_launches.json")))
    assert gold["grid_unit"] == "work-items" and gold["compute_units"] == 256
    g = gold["lds_granule"]
    assert len(gold["calls"]) == 124
    for c in gold["calls"]:
        key = (c["dir"], c["logn"], c["blowup"].bit_length() - 1 if c["dir"] == "fwd" else 0, c["npoly"])
        got = plans[key]
        assert got is not None, key
        for p, want in zip(got, (c["a"], c["b"])):
            mine = dict(p, grid=[p["grid"][0] * p["workgroup"], p["grid"][1]], lds=-(-p["lds"] // g) * g)
            assert mine == want, (key, mine, want)


def test_gpu_parity_shapes_reach_every_kernel(plans):
    listed = {p["kernel"] for ps in plans.values() if ps for p in ps}
    assert len(listed) == 48
    reached = set()
    for key in ntt_shapes.launches():
        assert plans.get(key) is not None, key
        reached |= {p["kernel"] for p in plans[key]}
    assert listed - reached == set()


KERNEL = re.compile(r"ntt_pass_([ab])(\w*)(?:<(.*)>)?")


def _steps(name):
    """(pass, Stockham steps) of a kernel the planner names: Plan<LOGS, LOGE> of ntt.hip. The generic kernels
    carry <LOGS, INV, LOGT, LOGE>; the dedicated ones are 16 x 16 (R or C = 256) or 32 x 32 (1024)"""
    which, special, args = KERNEL.fullmatch(name).groups()
    if special:
        assert special in ("_cos", "_cos2", "_r1024", "_tq", "_pers"), name
        return which, 2
    logs, _, _, loge = [a.strip() for a in args.split(",")]
    return which, -(-int(logs) // int(loge))


def test_adversarial_shapes_reach_every_kernel(plans):
    """the adversarial inputs (tests/ntt_adversarial.py) run on every kernel, and every kernel whose pass has
    more than one step gets targets at the outputs of its first step (B_step) at a shape that plans it"""
    listed = {p["kernel"] for ps in plans.values() if ps for p in ps}
    assert len(listed) == 48
    cases = ntt_shapes.adversarial_cases()
    reached, stepped = set(), set()
    for shape in ntt_shapes.ADVERSARIAL:
        d, logn, logbeta, npoly, subject = shape
        assert plans.get((d, logn, logbeta, npoly)) is not None, shape
        a, b = (p["kernel"] for p in plans[(d, logn, logbeta, npoly)])
        reached |= {a, b}
        # the Python restatement of the planner that the generators model the kernels by
        logr, logc = ntt_shapes.ntt_split(logn)
        ea, eb = ntt_shapes.pass_loge(logn)
        variant = {"ntt_pass_a_cos2": "cos2", "ntt_pass_a_r1024": "r1024"}.get(a, "plain")
        assert ntt_shapes.pass_a_variant(d, logn, logbeta, npoly) == variant, shape
        for name, which, logs, loge in ((a, "a", logr, ea), (b, "b", logc, eb)):
            assert _steps(name) == (which, ntt_shapes.step_plan(logs, loge)[0]), (shape, name)
            if "<" in name and not name.startswith(("ntt_pass_a_cos<", "ntt_pass_b_pers<")):
                args = name[name.index("<") + 1:-1].split(",")
                assert (int(args[0]), int(args[-1])) == (logs, loge), (shape, name)
            if (shape, "step_" + which) in cases:
                stepped.add(name)
            assert ((shape, "in_" + which) in cases) == (which in subject and logn <= 20), shape
        assert (shape, "out") in cases and (shape, "pass") in cases
    assert listed - reached == set()
    assert {k for k in listed if _steps(k)[1] > 1} - stepped == set()
    # every shape is the smallest of the printed domain that plans the kernel it is listed for
    cost = lambda key: (key[3] << (key[1] + key[2]), key[1], key[2], key[3])
    smallest = {}
    for key, ps in plans.items():
        for p in ps or []:
            if p["kernel"] not in smallest or cost(key) < cost(smallest[p["kernel"]]):
                smallest[p["kernel"]] = key
    assert set(smallest.values()) == {s[:4] for s in ntt_shapes.ADVERSARIAL}
