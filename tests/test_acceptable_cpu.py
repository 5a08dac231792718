"""The verifiers' policy argument on the host (no GPU): xfg_security_level, and xfg_verify_acceptable /
xfg_verify_batch_acceptable under AcceptableOptions::OptionSet and ::MinConjecturedSecurity -- what they accept,
the error texts, the order of the policy among the checks, and the refusals. The oracle makes every proof
(fold_cases.oracle_proof, verifier_faults.proofs); a case is (n, blowup, remainder max degree, queries, fold, ext)."""
import ctypes as C
import struct

import pytest

import fold_cases as FC
import proof_mutants as PM
import verifier_faults as VF
from test_verifier import _flip, _sections

A = (64, 8, 31, 42, 8, 1)  # the reference options at n = 64
B = (256, 4, 7, 42, 4, 1)
CC = (1024, 16, 31, 24, 16, 2)
# one shape per folding factor, both extensions; each has a FRI layer whose node vectors the mutants rearrange
PARITY = [(256, 8, 7, 42, 2, 1), (256, 4, 7, 42, 4, 2), (1024, 8, 31, 42, 8, 2), (1024, 16, 31, 24, 16, 1)]
UNACCEPTABLE = "UnacceptableProofOptions"


@pytest.fixture(scope="module")
def X():
    import xfgstark
    return xfgstark


def level(n, o):
    """winter-air 0.8 get_conjectured_security for a 64-bit field and Blake3_256, restated: o = (queries, blowup,
    grinding, extension degree, ...)"""
    q, blowup, grinding, ext = o[:4]
    field_security = 64 * ext - (n * blowup).bit_length() + 1
    query_security = (blowup.bit_length() - 1) * q
    if query_security >= 80:
        query_security += grinding
    return min(min(field_security, query_security) - 1, 128)


def options_tuple(o):
    return (o.num_queries, o.blowup_factor, o.grinding_factor, o.field_extension, o.fri_folding_factor,
            o.fri_remainder_max_degree)


def set_of(X, cases):
    return X.AcceptableOptions.option_set([FC.product_options(X, c) for c in cases])


def verifier(X, policy):
    return X.XfgBurnMintVerifier(acceptable=policy)


def item(X, case):
    kw, air, proof = FC.oracle_proof(case)
    return proof, X.air_consts(**kw)


# ------------------------------------------------------------------ levels
def test_pinned_levels(X):
    """hand-derived: 64 - 9 = 55 against 126 + 4; 64 - 19 = 45; 128 - 24 = 104 against 96 + 4 = 100; and 64 - 6 = 58
    against 21 bits of query security, below the floor of 80, so the grinding factor is not counted"""
    none, quad = X.FieldExtension.NONE, X.FieldExtension.QUADRATIC
    for o, n, want in [((42, 8, 4, none, 8, 31), 64, 54), ((42, 8, 4, none, 8, 31), 1 << 16, 44),
                       ((24, 16, 4, quad, 8, 31), 1 << 20, 99), ((7, 8, 4, none, 8, 7), 8, 20)]:
        assert X.ProofOptions(*o).security_level(n) == want
        assert level(n, o) == want


def test_levels_against_the_formula(X):
    """the grid: queries one below and at the grinding floor of each blowup, two grinding factors. The cap of 128
    bits (Blake3_256) is unreachable without the cubic extension: the field term is at most 128 - 4 = 124"""
    admitted = refused = 0
    for n in (8, 64, 1 << 16, 1 << 20):
        for blowup in (2, 8, 16, 128):
            floor_q = -(-80 // (blowup.bit_length() - 1))
            for ext in (1, 2):
                for q in (floor_q - 1, floor_q):
                    for grinding in (4, 16):
                        o = (q, blowup, grinding, ext, 8, 31)
                        # what check_options admits of this grid: the queries fit the LDE domain, which above
                        # blowup 16 has at most 2^24 points
                        ok = q < n * blowup and (blowup <= 16 or n * blowup <= 1 << 24)
                        if not ok:
                            with pytest.raises(X.XfgStarkError) as e:
                                X.ProofOptions(*o).security_level(n)
                            assert e.value.status == 9
                            refused += 1
                            continue
                        got = X.ProofOptions(*o).security_level(n)
                        assert got == level(n, o), (n, o)
                        assert got < 128
                        admitted += 1
    assert admitted >= 100 and refused >= 8
    # both sides of the floor are in the grid: the same options one query apart differ by more than a query's bits
    assert level(64, (27, 8, 4, 2, 8, 31)) - level(64, (26, 8, 4, 2, 8, 31)) == 3 + 4


def test_security_level_refusals(X):
    lib, bits = X._lib, C.c_uint32(77)
    o = X.ProofOptions.reference()._c()
    assert lib.xfg_security_level(64, None, C.byref(bits)) == 9
    assert lib.xfg_security_level(64, C.byref(o), None) == 9
    assert lib.xfg_security_level(48, C.byref(o), C.byref(bits)) == 9      # no power of two
    assert lib.xfg_security_level(1 << 22, C.byref(o), C.byref(bits)) == 9
    o.field_extension = 3
    assert lib.xfg_security_level(64, C.byref(o), C.byref(bits)) == 9
    assert bits.value == 77


@pytest.mark.parametrize("case", [A, B, CC], ids=FC.case_id)
def test_proof_security_level(X, case):
    kw, air, proof = FC.oracle_proof(case)
    p = X.StarkProof.from_bytes(proof)
    o = FC.product_options(X, case)
    assert p.security_level() == o.security_level(case[0]) == level(case[0], options_tuple(o))


# ------------------------------------------------------------------ sets
def test_set_membership(X):
    proof, air = item(X, A)
    assert verifier(X, set_of(X, [B, A])).verify_with_details(proof, air) == (True, None, len(proof))
    last = set_of(X, [(64, 8, 31, q, 8, 1) for q in range(1, 32)] + [A])
    assert len(last.options) == 32
    assert verifier(X, last).verify_with_details(proof, air) == (True, None, len(proof))
    assert verifier(X, set_of(X, [B, CC])).verify_with_details(proof, air) == (False, UNACCEPTABLE, len(proof))
    near = FC.product_options(X, A)
    near.grinding_factor += 1  # A in everything but the grinding factor
    policy = X.AcceptableOptions.option_set([near, FC.product_options(X, B)])
    assert verifier(X, policy).verify_with_details(proof, air) == (False, UNACCEPTABLE, len(proof))


@pytest.mark.parametrize("case", PARITY, ids=FC.case_id)
def test_one_element_set_is_xfg_verify(X, case):
    """the one-element set against the entry without a policy: the same verdict and text on the honest proof, on
    openings whose node vectors do not fit, and on a forgery that commits consistently"""
    proof, air = item(X, case)
    plain = X.XfgBurnMintVerifier(proof_options=FC.product_options(X, case))
    policy = verifier(X, set_of(X, [case]))
    assert plain.acceptable is None and policy.acceptable is not None
    mutants = PM.node_vector_mutants(proof)
    assert len(mutants) >= 15
    for m, ok in [(proof, True)] + mutants:
        want = plain.verify_with_details(m, air)
        assert want[0] == ok
        assert policy.verify_with_details(m, air) == want
    k, kw, oair, faults, st, forged = VF.proofs(case)[VF.STATEMENTS + 4]
    assert st == 0 and faults
    fair = X.air_consts(**kw)
    want = plain.verify_with_details(forged, fair)
    assert want[:2] == (False, VF.expected(case, faults)[0])
    assert policy.verify_with_details(forged, fair) == want
    # a proof of other options: the same refusal from both
    other, oa = item(X, A)
    assert plain.verify_with_details(other, oa) == policy.verify_with_details(other, oa) == (False, UNACCEPTABLE, len(other))


# ------------------------------------------------------------------ minimum
def minimum(X, bits):
    return verifier(X, X.AcceptableOptions.min_conjectured_security(bits))


def test_minimum_threshold(X):
    proof, air = item(X, A)
    lvl = X.StarkProof.from_bytes(proof).security_level()
    assert lvl == 54
    assert minimum(X, lvl).verify_with_details(proof, air) == (True, None, len(proof))
    assert minimum(X, 0).verify_with_details(proof, air) == (True, None, len(proof))
    too_low = f"InsufficientConjecturedSecurity({lvl + 1}, {lvl})"
    assert minimum(X, lvl + 1).verify_with_details(proof, air) == (False, too_low, len(proof))
    # the policy comes before the transcript: a tampered proof below the minimum reports the policy ...
    tampered = _flip(proof, _sections(proof)["trace_rows"][0] + 3)
    assert minimum(X, lvl + 1).verify_with_details(tampered, air)[1] == too_low
    assert minimum(X, lvl).verify_with_details(tampered, air)[1] == "TraceQueryDoesNotMatchCommitment"
    # ... and after StarkProof::from_bytes: a truncated one reports its deserialisation error
    cut = proof[:-5]
    plain = X.XfgBurnMintVerifier(proof_options=FC.product_options(X, A)).verify_with_details(cut, air)
    assert plain[0] is False and plain[1].startswith("ProofDeserializationError")
    assert minimum(X, lvl + 1).verify_with_details(cut, air) == plain


def test_library_limits_come_after_the_policy(X):
    """a header patched to the cubic extension: any minimum lets it through (its level only rises), the
    library's own limits then refuse it as unacceptable options"""
    proof, air = item(X, A)
    at = 5 + struct.unpack_from("<H", proof, 3)[0] + 9 + 3
    assert proof[at - 3:at + 3] == bytes([42, 8, 4, 1, 8, 31])
    cubic = proof[:at] + b"\x03" + proof[at + 1:]
    assert X.StarkProof.from_bytes(cubic).options.field_extension == X.FieldExtension.CUBIC
    assert minimum(X, 0).verify_with_details(cubic, air) == (False, UNACCEPTABLE, len(cubic))
    assert minimum(X, 54).verify_with_details(cubic, air) == (False, UNACCEPTABLE, len(cubic))


# ------------------------------------------------------------------ refusals
def bad_policies(X):
    """[(what, xfg_acceptable pointer or None)]: everything the entries refuse with XFG_INVALID_ARGUMENT"""
    o = FC.product_options(X, A)._c()
    many = (X._Options * 33)(*[o] * 33)
    mk = lambda kind, opts, num: X._Acceptable(kind, 0, opts, num)  # noqa: E731
    one = C.pointer(o)
    out = [("null policy", None), ("kind 2 (reserved for MinProvenSecurity)", mk(2, one, 1)), ("kind 3", mk(3, one, 1)),
           ("kind 2^32 - 1", mk(0xFFFFFFFF, one, 1)), ("set without options", mk(0, None, 1)),
           ("set of 0", mk(0, one, 0)), ("set of 33", mk(0, many, 33))]
    return [(what, None if a is None else C.pointer(a)) for what, a in out], (o, many)


def test_refusals(X):
    lib = X._lib
    proof, air = item(X, A)
    from xfgstark._marshal import air_struct, bytes_ptr
    a = air_struct(air)
    ptrs, lens = (X._u8p * 1)(bytes_ptr(proof)), (C.c_size_t * 1)(len(proof))
    policies, keep = bad_policies(X)
    for what, p in policies:
        err = C.create_string_buffer(b"untouched", 64)
        assert lib.xfg_verify_acceptable(bytes_ptr(proof), len(proof), C.byref(a), p, err, 64) == 9, what
        assert err.value == b"untouched", what
        res = (C.c_int * 1)(-5)
        assert lib.xfg_verify_batch_acceptable(1, ptrs, lens, C.byref(a), p, res, 1) == 9, what
        assert res[0] == -5, what  # nothing verified
    good = set_of(X, [A])._c()
    res = (C.c_int * 1)(-5)
    assert lib.xfg_verify_batch_acceptable(1, ptrs, lens, C.byref(a), C.byref(good), res, 1) == 0 and res[0] == 0
    assert lib.xfg_verify_acceptable(None, len(proof), C.byref(a), C.byref(good), None, 0) == 9
    assert lib.xfg_verify_acceptable(bytes_ptr(proof), len(proof), None, C.byref(good), None, 0) == 9
    assert lib.xfg_verify_batch_acceptable(1, ptrs, lens, C.byref(a), C.byref(good), None, 1) == 9


# ------------------------------------------------------------------ batch
@pytest.mark.parametrize("policy", ["set", "minimum"])
def test_threaded_batch_is_the_single_entry(X, policy):
    """a mixed list -- four folding factors, both extensions, misfit openings, a truncated proof, options outside
    the policy -- through xfg_verify_batch_acceptable on 1, 3 and all threads: item for item xfg_verify_acceptable"""
    items = []
    for case in PARITY + [A]:
        proof, air = item(X, case)
        items.append((proof, air))
        items += [(m, air) for m, ok in PM.node_vector_mutants(proof)[:4]] if case != A else [(proof[:-9], air)]
    if policy == "set":
        v = verifier(X, set_of(X, PARITY[:3]))  # PARITY[3] and A are outside
    else:
        v = minimum(X, 55)  # above A (54) and the base-field shapes, below the quadratic ones
    single = [v.verify_with_details(p, a)[:2] for p, a in items]
    want = [ok for ok, err in single]
    assert want.count(True) >= 2 and want.count(False) >= 8
    texts = {err for ok, err in single}
    assert (UNACCEPTABLE in texts) == (policy == "set")
    assert any(t and t.startswith("InsufficientConjecturedSecurity(55, ") for t in texts) == (policy == "minimum")
    for threads in (1, 3, 0):
        assert v.batch_verify(items, threads=threads) == want
