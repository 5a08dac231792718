"""Finished proofs taken apart and put back wrong, for the verifier tests (CPU and GPU): Merkle node
vectors that parse but do not fit their opening, and proofs broken in two places at once, which tell the
order of the verifier's checks.

TEST INFRASTRUCTURE ONLY. Section names and offsets are those of test_verifier._sections."""
import struct

TRACE = "TraceQueryDoesNotMatchCommitment"
CONSTRAINT = "ConstraintQueryDoesNotMatchCommitment"
LAYER_SIZE = "FriVerificationFailed(InvalidLayerCommitment)"
LAYER_COMMITMENT = "FriVerificationFailed(LayerCommitmentMismatch)"
REMAINDER_FOLDING = "FriVerificationFailed(InvalidRemainderFolding)"


def node_vectors(raw):
    """BatchMerkleProof node vectors of a paths section: u8 vector count, per vector u8 count + digests"""
    m, p, vecs = raw[0], 1, []
    for _ in range(m):
        c = raw[p]
        vecs.append([raw[p + 1 + 32 * i:p + 33 + 32 * i] for i in range(c)])
        p += 1 + 32 * c
    assert p == len(raw)
    return vecs


def with_node_vectors(proof, at, vecs):
    body = bytes([len(vecs)]) + b"".join(bytes([len(v)]) + b"".join(v) for v in vecs)
    start, ln = at
    return proof[:start - 4] + struct.pack("<I", len(body)) + body + proof[start + ln:]


def node_vector_mutants(proof):
    """(mutant, accepted) pairs: openings whose node vectors still parse but do not fit the opening,
    for the trace, constraint and first FRI layer paths -- a digest moved to the next vector (both
    directions), one node dropped, two vectors swapped (all rejected) -- and one node appended to a
    vector, which winter-crypto 0.8's get_root never reads (accepted, as by the oracle's restatement)"""
    from test_verifier import _sections
    sec = _sections(proof)
    out = []
    for name in ("trace_paths", "constraint_paths", "fri_paths0"):
        at = sec[name]
        vecs = node_vectors(proof[at[0]:at[0] + at[1]])
        i = next(k for k in range(len(vecs) - 1) if len(vecs[k]) and len(vecs[k + 1]))
        v = [list(x) for x in vecs]
        v[i + 1].insert(0, v[i].pop())  # last digest of vector i moved to the front of vector i + 1
        out.append((with_node_vectors(proof, at, v), False))
        v = [list(x) for x in vecs]
        v[i].append(v[i + 1].pop(0))  # first digest of vector i + 1 moved to the end of vector i
        out.append((with_node_vectors(proof, at, v), False))
        v = [list(x) for x in vecs]
        v[i].append(v[i][-1])  # one node appended: never read by the walk
        out.append((with_node_vectors(proof, at, v), True))
        v = [list(x) for x in vecs]
        v[i].insert(0, v[i][-1])  # one node prepended: shifts every node the walk reads
        out.append((with_node_vectors(proof, at, v), False))
        v = [list(x) for x in vecs]
        v[i].pop()  # one node dropped
        out.append((with_node_vectors(proof, at, v), False))
        if vecs[i] != vecs[i + 1]:
            v = [list(x) for x in vecs]
            v[i], v[i + 1] = v[i + 1], v[i]  # two vectors swapped
            out.append((with_node_vectors(proof, at, v), False))
    return out


# Reference options (fold 8, base field: an opened FRI row is 64 bytes, a remainder coefficient 8), one
# FRI layer at n = 256 and two at n = 1024. A FRI section of the wrong size is a structural error; the
# second break, a flipped byte in a section the verifier opens earlier, tells where in its walk each
# verifier reports the structural one. (n, shortened section, bytes cut, section with a flipped byte or
# None, xfg_verify's error): the host reports the size at its place in the walk, after every opening
# that comes before it. The batched GPU verifier reports the size first (test_gpu_parity.py).
CHECK_ORDER = [
    (256, "fri_vals0", 64, None, LAYER_SIZE),
    (256, "fri_vals0", 64, "trace_rows", TRACE),
    (256, "fri_vals0", 64, "constraint_rows", CONSTRAINT),
    (256, "remainder", 8, None, REMAINDER_FOLDING),
    (256, "remainder", 8, "fri_vals0", LAYER_COMMITMENT),
    (256, "remainder", 8, "trace_rows", TRACE),
    (1024, "fri_vals1", 64, None, LAYER_SIZE),
    (1024, "fri_vals1", 64, "fri_vals0", LAYER_COMMITMENT),
    (1024, "fri_vals1", 64, "trace_rows", TRACE),
]


def check_order_id(c):
    n, short, cut, flip, err = c
    return f"n{n}-{short}-{flip or 'alone'}"


def doubly_broken(proof, short, cut, flip):
    """`proof` with the last `cut` bytes of section `short` removed (its length prefix adjusted: u16 for
    the remainder, u32 otherwise) and, if named, one flipped byte in section `flip`, which lies before it"""
    from test_verifier import _flip, _sections
    sec = _sections(proof)
    if flip is not None:
        assert sec[flip][0] < sec[short][0]
        proof = _flip(proof, sec[flip][0] + 3)
    at, ln = sec[short]
    fmt = "<H" if short == "remainder" else "<I"
    out = proof[:at - struct.calcsize(fmt)] + struct.pack(fmt, ln - cut) + proof[at:at + ln - cut] + proof[at + ln:]
    _sections(out)  # still a proof, structurally
    return out
