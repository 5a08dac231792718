"""The option sets of the folding-factor tests (CPU and GPU) and the oracle's proof of each, made once
per process and shared by every test that needs it.

TEST INFRASTRUCTURE ONLY. A case is (n, blowup, remainder max degree, queries, fold, ext); every listed
one keeps the last FRI layer at 8 points or more and at the blowup or more, the shapes the prover takes
(the oracle is not called on any other shape: it is not reliable there)."""
import functools

import oracle_lib as O
import synthetic

NEW_FACTORS = (2, 4, 16)
# (n, blowup, remainder max degree, queries)
ANY_FACTOR = [(64, 8, 31, 42), (1024, 16, 31, 24), (4096, 8, 31, 42), (4096, 2, 255, 42), (32, 4, 1, 20),
              (2048, 16, 127, 42),
              (8, 8, 7, 7)]  # no FRI layer: the factor reaches only the context
FACTORS_2_4 = [(256, 4, 7, 42), (1024, 8, 0, 42)]
FACTOR_4 = [(16, 2, 7, 8)]
FACTOR_2_DEEP = [(8192, 8, 0, 42), (16384, 16, 1, 42)]  # 13 FRI layers


def shapes():
    """[(n, blowup, remdeg, queries, fold)]"""
    out = [s + (f,) for s in ANY_FACTOR for f in NEW_FACTORS]
    out += [s + (f,) for s in FACTORS_2_4 for f in (2, 4)]
    out += [s + (4,) for s in FACTOR_4]
    out += [s + (2,) for s in FACTOR_2_DEEP]
    return out


CASES = [s + (ext,) for s in shapes() for ext in (1, 2)]


def case_id(c):
    n, beta, remdeg, q, fold, ext = c
    return f"n{n}-b{beta}-r{remdeg}-q{q}-f{fold}-e{ext}"


def num_layers(n, beta, remdeg, fold):
    """(FRI layers, size of the last one) by the rule of winter-fri's FriOptions::num_fri_layers"""
    D, nl = n * beta, 0
    while D > (remdeg + 1) * beta:
        D //= fold
        nl += 1
    return nl, D


def oracle_options(c):
    n, beta, remdeg, q, fold, ext = c
    return O.options(num_queries=q, blowup=beta, field_extension=ext, fri_folding=fold, fri_rem_max_deg=remdeg)


def product_options(X, c):
    n, beta, remdeg, q, fold, ext = c
    o = X.ProofOptions.reference()
    o.num_queries, o.blowup_factor, o.field_extension = q, beta, ext
    o.fri_folding_factor, o.fri_remainder_max_degree = fold, remdeg
    return o


def inputs(c):
    """the burn inputs of a case (seeded by the case)"""
    n, beta, remdeg, q, fold, ext = c
    return synthetic.burn_inputs(9000 + n + 7 * beta + 3 * remdeg + 11 * fold + ext)


def oracle_air(kw):
    st, air = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                                kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])
    assert st == 0
    return air


@functools.lru_cache(maxsize=None)
def oracle_proof(c):
    """(burn inputs, oracle AIR, proof bytes): orc_prove's proof of the case, accepted by orc_verify"""
    n = c[0]
    assert num_layers(*c[:3], c[4])[1] >= max(8, c[1]), "not a shape the oracle is called on"
    kw = inputs(c)
    air = oracle_air(kw)
    opts = oracle_options(c)
    st, proof = O.prove(air, n, opts)
    assert st == 0
    assert O.verify(air, proof, opts) == 0
    return kw, air, proof
