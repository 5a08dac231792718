"""Packed burn records on the CPU (xfg-stark_amd/csrc/burn_record.hpp and the host side of the record entries).

tests/sanitize/burn_statement.cpp is a stand-alone program: the record's size and offsets, record_to_inputs, the
validation order of both statement forms, the length rules of xfg_burn_inputs, the four Keccak message layouts and
the one host marshaller (marshal.hpp) against its own hand-written marshalling, the padding words (see its header).
Here it is built with ASan + UBSan (`make -C xfg-stark_amd sanitize`) and the binary is run directly: exit 0,
nothing from a sanitizer. The rest needs no device: pack_records / unpack_records, and
xfg_air_consts_from_records on host records against xfg_burn_air_consts, the oracle and the golden vectors."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "xfg-stark_amd")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")
TARGET = "build/asan/burn_statement"
IDS = dict(network_id=1, target_chain_id=42161, commitment_version=1)


def test_driver_is_clean_under_the_sanitizer():
    subprocess.run(["make", "-s", "-C", LIB, TARGET], check=True)
    r = subprocess.run([os.path.join(LIB, TARGET)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert r.stdout == "burn_statement ok\n"


def test_sanitize_target_builds_the_driver():
    subprocess.run(["make", "-s", "-C", LIB, "sanitize"], check=True)
    assert os.path.exists(os.path.join(LIB, "build", "asan", "burn_statement"))


def _inputs(count, **over):
    return [dict(IDS, **synthetic.burn_inputs(i), **over) for i in range(count)]


def _bench_pack(kws):
    """bench.pack_inputs restated (bench.py is not imported: it is the benchmark, not a library): burn u64, mint
    u64, tx 32, recipient 20, secret 32, ids 3 x u32 in a 128-byte record, little-endian"""
    out = np.zeros((len(kws), 128), dtype=np.uint8)
    for i, kw in enumerate(kws):
        b = kw["burn_amount"].to_bytes(8, "little") + kw["mint_amount"].to_bytes(8, "little")
        b += kw["tx_prefix_hash"] + kw["recipient_address"].ljust(20, b"\0")[:20] + kw["secret"].ljust(32, b"\0")[:32]
        b += kw["network_id"].to_bytes(4, "little") + kw["target_chain_id"].to_bytes(4, "little")
        b += kw["commitment_version"].to_bytes(4, "little")
        out[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return out


def test_pack_records_round_trip_and_bytes():
    import xfgstark
    kws = _inputs(9)
    kws[3].update(network_id=0, target_chain_id=0xFFFFFFFF, commitment_version=7)
    kws[4].update(burn_amount=8_000_000_000, mint_amount=1 << 63)
    rec = xfgstark.pack_records(kws)
    assert rec.shape == (9, 128) and rec.dtype == np.uint8 and rec.flags.c_contiguous
    assert np.array_equal(rec, _bench_pack(kws))
    assert (rec[:, 112:] == 0).all()
    assert xfgstark.unpack_records(rec) == kws
    assert np.array_equal(xfgstark.pack_records(xfgstark.unpack_records(rec)), rec)
    # the defaults of prove_burn_mint for the three ids
    assert np.array_equal(xfgstark.pack_records([synthetic.burn_inputs(0)]), rec[:1])


def test_pack_records_matches_the_benchmarks_packing():
    """the records of the sharded path (bench.pack_inputs), byte for byte"""
    import bench
    import xfgstark
    kws = _inputs(5)
    assert bench.REC == xfgstark.RECORD_BYTES == 128
    assert np.array_equal(xfgstark.pack_records(kws), bench.pack_inputs(kws))
    assert bench.unpack_inputs(xfgstark.pack_records(kws)) == xfgstark.unpack_records(xfgstark.pack_records(kws))


def test_host_records_give_the_constants_of_the_struct_path_and_the_oracle():
    import xfgstark
    kws = _inputs(12)
    kws[5].update(burn_amount=8_000_000_000, mint_amount=8_000_000_000)
    kws[6].update(network_id=0, target_chain_id=0xFFFFFFFF, commitment_version=0xFFFFFFFF)
    kws[7].update(tx_prefix_hash=bytes(4) + b"\x01" + bytes(27))  # valid: the u64 is non-zero, pub[2] is 0
    kws[8].update(tx_prefix_hash=b"\xff" * 32, recipient_address=b"\xff" * 20, secret=b"\xff" * 32)
    got = xfgstark.air_consts_from_records(xfgstark.pack_records(kws))
    for kw, g in zip(kws, got):
        assert g == xfgstark.air_consts(**kw)
        st, air = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                                    kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])
        assert st == 0 and g == (list(air.pub), air.nullifier, air.commitment)
    assert got[7][0][2] == 0


def _kats():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))


def test_host_records_match_the_reference_package():
    import xfgstark
    r = _kats()["test_data_package"]
    kw = {k: (bytes.fromhex(v) if isinstance(v, str) else v) for k, v in r["inputs"].items()}
    (pub, nf, cm), = xfgstark.air_consts_from_records(xfgstark.pack_records([kw]))
    assert pub == r["pub_inputs"] and nf == r["nullifier"] and cm == r["commitment"]


def test_host_records_report_the_reference_validation_statuses():
    """every case of the golden validation list that a record can state (a record's recipient always has 20
    bytes: the case with 19 has no record), through the C entry, with the constants marshalled all the same"""
    import xfgstark
    C = xfgstark.C
    cases = [c for c in _kats()["validation"] if c["rlen"] == 20]
    assert {c["status"] for c in cases} == {0, 1, 2, 3}
    kws = [dict(IDS, burn_amount=c["burn"], mint_amount=c["mint"], tx_prefix_hash=bytes([0 if c["tx_zero"] else 1]) + bytes(31),
                recipient_address=b"\x12" * 20, secret=b"\x2a" * 32) for c in cases]
    rec = xfgstark.pack_records(kws)
    airs, sts = (xfgstark._abi._AirConsts * len(kws))(), (C.c_int * len(kws))()
    assert xfgstark._lib.xfg_air_consts_from_records(None, len(kws), rec.ctypes.data, 0, airs, sts) == 0
    assert list(sts) == [c["status"] for c in cases]
    for kw, a, c in zip(kws, airs, cases):
        st, air = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                                    kw["secret"])
        assert st == c["status"]
        assert a.pub_inputs[3] == list(O.air_from_inputs(8_000_000, 8_000_000, b"\x01" + bytes(31), kw["recipient_address"],
                                                         kw["secret"])[1].pub)[3]
        assert list(a.pub_inputs)[:2] == [kw["burn_amount"] & 0xFFFFFFFF, kw["mint_amount"] & 0xFFFFFFFF]
    got = xfgstark.air_consts_from_records(rec)
    assert [g.status if isinstance(g, xfgstark.XfgStarkError) else 0 for g in got] == [c["status"] for c in cases]


def test_validation_order_and_reserved_bytes():
    import xfgstark
    kw = _inputs(1)[0]
    rec = xfgstark.pack_records([kw] * 5)
    rec[0, 0] ^= 1               # burn amount ...
    rec[0, 8] ^= 2               # ... and a mint mismatch behind it: status 1
    rec[1, 8] ^= 2               # mint mismatch ...
    rec[1, 16:24] = 0            # ... and a zero tx hash: status 2
    rec[2, 16:24] = 0            # zero tx hash ...
    rec[2, 127] = 1              # ... and a reserved byte: status 3
    rec[3, 112] = 0x80           # a reserved byte alone: status 9
    got = xfgstark.air_consts_from_records(rec)
    assert [g.status if isinstance(g, xfgstark.XfgStarkError) else 0 for g in got] == [1, 2, 3, 9, 0]


def test_host_entry_refusals():
    import xfgstark
    C = xfgstark.C
    rec = xfgstark.pack_records(_inputs(2))
    airs, sts = (xfgstark._abi._AirConsts * 2)(), (C.c_int * 2)()
    f = xfgstark._lib.xfg_air_consts_from_records
    assert f(None, 0, rec.ctypes.data, 0, airs, sts) == 9          # count 0
    assert f(None, 2, None, 0, airs, sts) == 9                     # a null pointer
    assert f(None, 2, rec.ctypes.data, 0, None, sts) == 9
    assert f(None, 2, rec.ctypes.data, 2, airs, sts) == 9          # an unknown flag
    assert f(None, 2, rec.ctypes.data, xfgstark.RECORDS_ON_DEVICE, airs, sts) == 9  # the device flag needs a context
    with pytest.raises(xfgstark.XfgStarkError):
        xfgstark.air_consts_from_records(rec.reshape(-1)[:200])    # no whole number of records
    with pytest.raises(xfgstark.XfgStarkError):
        xfgstark.air_consts_from_records(rec.astype(np.uint16))
