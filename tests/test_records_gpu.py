"""GPU: burn statements as packed records (xfg_prove_records / _submit, xfg_air_consts_from_records) from host
arrays and from device tensors, and the record kernel's Keccak-256 alone (xfg_debug_keccak256).

  * the lane-spread Keccak against the oracle's at every single-block length,
  * the record kernel's constants and statuses against the host path and the oracle,
  * whole batches against prove_batch and the CPU oracle's bytes, proof by proof,
  * pipelining with a batch of traces, the round trip through the GPU verifier, and the refusals.
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest
# before the first import of xfgstark, as tests/test_trace_batch_gpu.py does: one HIP runtime for torch and the
# library, so that a tensor's data_ptr() is a device pointer the library's calls know
import torch

import fold_cases as F
import oracle_lib as O
import synthetic
import trace_check_ref as T

pytestmark = pytest.mark.gpu

STD, LARGE = 8_000_000, 8_000_000_000
# the lengths of the four messages of a statement (burn_record.hpp): recipient, nullifier, recipient-full, commitment
KERNEL_LENGTHS = (29, 25, 46, 130)


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _dev(rec):
    return torch.from_numpy(np.ascontiguousarray(rec)).to("cuda:0")


def _status_of(f):
    import xfgstark
    try:
        f()
    except xfgstark.XfgStarkError as e:
        return e.status
    return 0


def _oracle_air(kw):
    return O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                             kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])


# ---------------------------------------------------------------- the permutation alone
def test_keccak_hook_matches_the_oracle_at_every_length(prover):
    """all 136 single-block lengths 0..135, contents 0x00, 0xFF and random: the padding byte moves through every
    position of every lane's word, meets the final 0x80 in one word at 128..134 and in one byte (0x81) at 135.
    408 messages, two to a wave"""
    rng = random.Random(23)
    assert all(k < 136 for k in KERNEL_LENGTHS)
    msgs = [fill(k) for k in range(136) for fill in (bytes, lambda k: b"\xff" * k, rng.randbytes)]
    got = prover.debug_keccak256(msgs)
    for m, g in zip(msgs, got):
        assert g == O.keccak256(m), (len(m), m[:4])
    # Keccak's padding, not SHA-3's
    assert got[0] == bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")
    assert got[0] != O.sha3_256(b"")


@pytest.mark.parametrize("count", [1, 2, 3])
def test_keccak_hook_at_odd_counts(prover, count):
    """the last wave's second half has no message at an odd count"""
    rng = random.Random(count)
    msgs = [rng.randbytes(KERNEL_LENGTHS[i % 4]) for i in range(count)]
    assert prover.debug_keccak256(msgs) == [O.keccak256(m) for m in msgs]


def test_keccak_hook_refusals(prover):
    import xfgstark
    assert _status_of(lambda: prover.debug_keccak256([])) == 9
    lens, out = np.array([136], dtype=np.uint32), np.zeros(32, dtype=np.uint8)
    msgs = np.zeros(136, dtype=np.uint8)
    u8p, u32p = xfgstark._u8p, C.POINTER(C.c_uint32)
    assert xfgstark._lib.xfg_debug_keccak256(prover._ctx, 1, msgs.ctypes.data_as(u8p), lens.ctypes.data_as(u32p),
                                             out.ctypes.data_as(u8p)) == 9


# ---------------------------------------------------------------- constants and statuses
EDGE_STATUS = [0, 0, 3, 0, 0, 0, 2, 1, 9, 2]


def _edge_records(count):
    """count records, record i the edge case i % 10 on the synthetic statement i: (records [count, 128], statuses)"""
    import xfgstark
    kws = [dict(synthetic.burn_inputs(100 + i)) for i in range(count)]
    for i, kw in enumerate(kws):
        e = i % 10
        if e == 1:
            kw.update(burn_amount=LARGE, mint_amount=LARGE)                     # the other burn amount
        elif e == 2:
            kw.update(tx_prefix_hash=bytes(8) + kw["tx_prefix_hash"][8:])       # tx[0..8] == 0: status 3
        elif e == 3:
            kw.update(tx_prefix_hash=bytes(4) + b"\x00\x00\x00\x01" + kw["tx_prefix_hash"][8:])  # valid, pub[2] == 0
        elif e == 4:
            kw.update(tx_prefix_hash=b"\xff" * 32, recipient_address=b"\xff" * 20, secret=b"\xff" * 32)
        elif e == 5:
            kw.update(network_id=0, target_chain_id=0xFFFFFFFF, commitment_version=0xFFFFFFFF)
        elif e == 6:
            kw.update(mint_amount=STD + 1)                                      # mint != burn: status 2
        elif e == 7:
            kw.update(burn_amount=STD + 1, mint_amount=7)                       # and a mismatch behind it: status 1
        elif e == 9:
            kw.update(burn_amount=LARGE, mint_amount=STD)                       # status 2 with the large amount
    rec = xfgstark.pack_records(kws)
    for i in range(count):
        if i % 10 == 8:
            rec[i, 112 + i % 16] = 1                                            # a reserved byte: status 9
    return rec, kws, [EDGE_STATUS[i % 10] for i in range(count)]


def _consts(prover, where, count, flags):
    """xfg_air_consts_from_records through ctypes: ([(pub, nullifier, commitment)], [status]), the constants of
    invalid records included"""
    import xfgstark
    airs, sts = (xfgstark._abi._AirConsts * count)(), (C.c_int * count)()
    ctx = prover._ctx if prover is not None else None
    assert xfgstark._lib.xfg_air_consts_from_records(ctx, count, where, flags, airs, sts) == 0
    return [(list(a.pub_inputs), a.nullifier, a.commitment) for a in airs], list(sts)


# one wave (a 64-thread block) per record: the grid is the count and has no other boundary; the counts straddle
# the unit size (32) and two units (64) all the same, and 10 holds every edge record once
@pytest.mark.parametrize("count", [1, 2, 10, 31, 32, 33, 64, 65])
def test_device_constants_match_host_and_oracle(prover, count):
    rec, kws, want_st = _edge_records(count)
    t = _dev(rec)
    dev, dev_st = _consts(prover, t.data_ptr(), count, 1)
    host, host_st = _consts(None, rec.ctypes.data, count, 0)
    assert dev_st == host_st == want_st
    assert dev == host
    for kw, st, d in zip(kws, want_st, dev):
        ost, air = _oracle_air(kw)
        assert ost == (0 if st == 9 else st)  # the reserved bytes are the record's own rule
        if ost == 0:
            assert d == (list(air.pub), air.nullifier, air.commitment)
    assert all(v < 1 << 32 for d in dev for v in d[0] + [d[1], d[2]])
    if count >= 10:
        assert dev[3][0][2] == 0 and dev_st[3] == 0
    assert torch.equal(t.cpu(), torch.from_numpy(rec))
    # the wrapper: errors in the places of the invalid records
    got = prover.air_consts_from_records(t)
    assert [g.status if isinstance(g, Exception) else 0 for g in got] == want_st
    assert [g for g in got if not isinstance(g, Exception)] == [d for d, st in zip(dev, want_st) if st == 0]


# ---------------------------------------------------------------- proofs
@functools.lru_cache(maxsize=None)
def _proof_batch():
    """35 records: one 32-proof unit and a remainder; invalid at 0 (the unit's proof 0), 17 and 34 (the last). The
    valid ones burn the standard amount: the large one is proven like any other but, its public input being the
    amount's low 32 bits as in the reference, no verifier takes that proof (the constants test covers the amount)"""
    import xfgstark
    kws = [dict(synthetic.burn_inputs(300 + i)) for i in range(35)]
    kws[0].update(burn_amount=STD - 1, mint_amount=STD - 1)
    kws[17].update(mint_amount=LARGE)
    kws[34].update(tx_prefix_hash=bytes(8) + kws[34]["tx_prefix_hash"][8:])
    rec = xfgstark.pack_records(kws)
    want = []
    for kw in kws:
        st, air = _oracle_air(kw)
        want.append(O.prove(air, 64, O.options())[1] if st == 0 else st)
    return rec, kws, want


def _as_bytes(results):
    """proofs as bytes, errors as their status"""
    return [r.status if isinstance(r, Exception) else r.to_bytes() for r in results]


def test_record_proofs_match_prove_batch_and_the_oracle(prover):
    rec, kws, want = _proof_batch()
    assert [w for w in want if isinstance(w, int)] == [1, 2, 3]
    struct = _as_bytes(prover.prove_batch(kws, 64))
    t = _dev(rec)
    dev = _as_bytes(prover.prove_records(t, 64))
    host = _as_bytes(prover.prove_records(rec.copy(), 64))
    assert [len(d) if isinstance(d, bytes) else d for d in dev] == [len(s) if isinstance(s, bytes) else s for s in struct]
    assert dev == struct
    assert host == dev
    assert dev == want
    assert torch.equal(t.cpu(), torch.from_numpy(rec))


def test_record_entry_statuses_and_lengths(prover):
    """through ctypes: statuses as xfg_prove_batch gives them, out_lens the proofs' lengths and 0 for an invalid
    record, from device and from host records alike"""
    import xfgstark
    rec, kws, want = _proof_batch()
    k = len(kws)
    o, cap = prover._options._c_and_bound(64)
    t = _dev(rec)
    for where, flags in ((t.data_ptr(), 1), (rec.ctypes.data, 0)):
        buf = C.create_string_buffer(cap * k)
        outs, lens, sts = xfgstark._marshal.out_slots(k, cap, C.addressof(buf))
        assert xfgstark._lib.xfg_prove_records(prover._ctx, k, where, 0, C.byref(o), flags, outs, lens, sts) == 0
        assert list(sts) == [w if isinstance(w, int) else 0 for w in want]
        assert list(lens) == [0 if isinstance(w, int) else len(w) for w in want]  # trace_length 0 means 64
        assert buf.raw[cap:cap + lens[1]] == want[1]


@pytest.mark.parametrize("status,change", [
    (1, dict(burn_amount=5, mint_amount=5)), (2, dict(mint_amount=123456789)),
    (2, dict(burn_amount=LARGE, mint_amount=(1 << 64) - 1)), (3, dict(tx_prefix_hash=bytes(8) + b"\x07" * 24))])
def test_error_text_is_the_host_paths(prover, status, change):
    import xfgstark
    kws = [dict(synthetic.burn_inputs(400)), dict(synthetic.burn_inputs(401), **change)]
    want = prover.prove_batch(kws, 64)
    text = prover.last_error()
    assert want[1].status == status and text
    rec = xfgstark.pack_records(kws)
    for records in (_dev(rec), rec):
        got = prover.prove_records(records, 64)
        assert got[1].status == status and prover.last_error() == text
        assert got[0].to_bytes() == want[0].to_bytes()


def test_reserved_bytes_are_refused_per_record(prover):
    import xfgstark
    kws = [dict(synthetic.burn_inputs(410 + i)) for i in range(3)]
    rec = xfgstark.pack_records(kws)
    rec[1, 127] = 0x80
    want = prover.prove_batch(kws, 64)
    for records in (_dev(rec), rec):
        got = prover.prove_records(records, 64)
        assert got[1].status == 9 and prover.last_error() == "record: the reserved bytes must be zero"
        assert [g.to_bytes() for g in (got[0], got[2])] == [w.to_bytes() for w in (want[0], want[2])]


def test_records_at_n8_in_the_quadratic_extension():
    """n = 8 with no FRI layer, 7 queries, blowup 8, the quadratic extension (a case of tests/fold_cases.py)"""
    import xfgstark
    case = (8, 8, 7, 7, 4, 2)
    assert case in F.CASES
    pr = xfgstark.XfgBurnMintProver.with_options(128, F.product_options(xfgstark, case))
    try:
        kws = [dict(synthetic.burn_inputs(500 + i)) for i in range(5)]
        kws[2].update(mint_amount=1)
        rec = xfgstark.pack_records(kws)
        struct = _as_bytes(pr.prove_batch(kws, 8))
        assert _as_bytes(pr.prove_records(_dev(rec), 8)) == struct
        assert _as_bytes(pr.prove_records(rec, 8)) == struct
        for kw, s in zip(kws, struct):
            st, air = _oracle_air(kw)
            assert s == (O.prove(air, 8, F.oracle_options(case))[1] if st == 0 else st)
    finally:
        pr.close()


def test_record_batches_pipeline_with_a_trace_batch(prover):
    """two record batches and a batch of caller-supplied traces in flight together, waited for out of order"""
    import xfgstark
    rec, kws, want = _proof_batch()
    rec2 = xfgstark.pack_records([dict(synthetic.burn_inputs(600 + i)) for i in range(7)])
    traces, airs = zip(*[T.valid_trace(64, 700 + i) for i in range(3)])
    traces = np.stack(traces)
    alone = [_as_bytes(prover.prove_records(_dev(rec2), 64)), _as_bytes(prover.prove_traces(traces, list(airs)))]
    t1, t2 = _dev(rec), _dev(rec2)
    a = prover.submit_records(t1, 64)
    b = prover.submit_traces(traces, list(airs))
    c = prover.submit_records(t2, 64)
    assert _as_bytes(c.result()) == alone[0]
    assert _as_bytes(a.result()) == want
    assert _as_bytes(b.result()) == alone[1]


def test_record_proofs_verify_on_the_gpu_against_the_records_constants(prover):
    import xfgstark
    rec, kws, want = _proof_batch()
    t = _dev(rec)
    proofs = prover.prove_records(t, 64)
    airs = prover.air_consts_from_records(t)
    pairs = [(p, a) for p, a in zip(proofs, airs) if not isinstance(p, Exception)]
    assert len(pairs) == 32 and not any(isinstance(a, Exception) for _, a in pairs)
    v = xfgstark.XfgBurnMintVerifier()
    assert v.batch_verify(pairs, gpu=prover) == [True] * 32
    swapped = [(pairs[0][0], pairs[1][1])] + pairs[1:3]
    assert v.batch_verify(swapped, gpu=prover) == [False, True, True]


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(prover):
    import xfgstark
    lib = xfgstark._lib
    rec = xfgstark.pack_records([dict(synthetic.burn_inputs(800 + i)) for i in range(3)])
    t = _dev(rec)
    o, cap = prover._options._c_and_bound(64)
    buf = C.create_string_buffer(cap * 3)
    outs, lens, sts = xfgstark._marshal.out_slots(3, cap, C.addressof(buf))
    airs = (xfgstark._abi._AirConsts * 3)()
    ticket = C.c_uint64(0)

    def submit(where, count, flags, opts=C.byref(o)):
        return lib.xfg_prove_records_submit(prover._ctx, count, where, 64, opts, flags, outs, lens, sts, C.byref(ticket))

    def consts(where, count, flags):
        return lib.xfg_air_consts_from_records(prover._ctx, count, where, flags, airs, sts)

    # the device flag with host memory
    assert submit(rec.ctypes.data, 3, 1) == 9 and "records is not" in prover.last_error()
    assert consts(rec.ctypes.data, 3, 1) == 9 and "records is not" in prover.last_error()
    # a tensor shorter than 128 * count: torch gives a request of this size a segment of its own, rounded up to
    # 2 MB, once no cached segment is left to carve it from; twice its records are asked for
    torch.cuda.empty_cache()
    big = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda:0")
    assert submit(big.data_ptr(), 2 * (16 << 20) // 128, 1) == 9 and "allocation" in prover.last_error()
    assert consts(big.data_ptr(), 2 * (16 << 20) // 128, 1) == 9 and "allocation" in prover.last_error()
    # a base that is not 8-byte aligned
    assert submit(big.data_ptr() + 4, 3, 1) == 9 and prover.last_error() == "records is not 8-byte aligned"
    assert consts(big.data_ptr() + 4, 3, 1) == 9 and prover.last_error() == "records is not 8-byte aligned"
    assert _status_of(lambda: prover.prove_records(big[4:4 + 256], 64)) == 9
    # count 0, null pointers, an unknown flag
    assert submit(t.data_ptr(), 0, 1) == 9 and prover.last_error() == "empty batch"
    assert consts(t.data_ptr(), 0, 1) == 9
    assert _status_of(lambda: prover.prove_records(t[:0], 64)) == 9
    assert _status_of(lambda: prover.prove_records(rec[:0], 64)) == 9
    assert submit(None, 3, 1) == 9 and prover.last_error() == "null argument"
    assert submit(t.data_ptr(), 3, 1, opts=None) == 9
    assert submit(t.data_ptr(), 3, 2) == 9 and prover.last_error() == "unknown record flag"
    assert consts(t.data_ptr(), 3, 4) == 9
    # a tensor elsewhere, of another type, or no whole number of records
    assert _status_of(lambda: prover.prove_records(torch.from_numpy(rec), 64)) == 9
    assert _status_of(lambda: prover.prove_records(t.view(torch.int8), 64)) == 9
    assert _status_of(lambda: prover.prove_records(t.reshape(-1)[:200], 64)) == 9
    assert ticket.value == 0
    # the record kernel on lane 0 while a batch is pending
    pending = prover.submit_records(t, 64)
    assert _status_of(lambda: prover.air_consts_from_records(t)) == 9
    assert "pending" in prover.last_error()
    assert all(not isinstance(p, Exception) for p in pending.result())
    assert len(prover.air_consts_from_records(t)) == 3
