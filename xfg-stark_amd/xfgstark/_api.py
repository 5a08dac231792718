"""The product API: the reference's prover, verifier, options and proof types over the C ABI, and the
instrumentation bench.py reads."""
import ctypes as C
import operator
import sys

from ._abi import (ACCEPT_MIN_CONJECTURED_SECURITY, ACCEPT_OPTION_SET, RECORD_BYTES, RECORDS_ON_DEVICE, STATUS,
                   TRACE_ON_DEVICE, TRACE_VALIDATE, XfgStarkError, _Acceptable, _AirConsts, _BurnInputs, _BurnRecord,
                   _lib, _Options, _ProofInfo, _TraceFault, _TraceLayout, _u8p)
from ._hooks import KernelHooks
from ._marshal import air_array, air_struct, array, bytes_ptr, new_buffer, out_slots, ptr, trace_array, zeros


class TraceFault:
    """xfg_trace_fault: what Trace::validate reports first for a trace. kind 1 = assertion `index` (0..7)
    on main_trace(column, step), expected / found the asserted value and the cell; 2 = transition
    constraint `index` (0..6) at `step`; 3 = the cell (column, step) = found is not a canonical field
    element. str() is Winterfell's message."""
    ASSERTION, TRANSITION, NONCANONICAL = 1, 2, 3

    def __init__(self, kind, index, column, step, expected, found):
        self.kind, self.index, self.column, self.step = kind, index, column, step
        self.expected, self.found = expected, found

    @classmethod
    def _from_c(cls, f):
        return cls(f.kind, f.index, f.column, f.step, f.expected, f.found) if f.kind else None

    def astuple(self):
        return (self.kind, self.index, self.column, self.step, self.expected, self.found)

    def __eq__(self, other):
        return isinstance(other, TraceFault) and other.astuple() == self.astuple()

    def __str__(self):
        if self.kind == self.ASSERTION:
            return f"trace does not satisfy assertion main_trace({self.column}, {self.step}) == {self.expected}"
        if self.kind == self.TRANSITION:
            return f"main transition constraint {self.index} did not evaluate to ZERO at step {self.step}"
        return "trace element is not a canonical field element"

    def __repr__(self):
        return "TraceFault(kind={}, index={}, column={}, step={}, expected={}, found={})".format(*self.astuple())


class FieldExtension:
    NONE = 1
    QUADRATIC = 2
    CUBIC = 3


_option_values = operator.attrgetter(*[name for name, _ in _Options._fields_])  # of an xfg_options or a ProofOptions


class ProofOptions:
    """winterfell::ProofOptions::new(num_queries, blowup_factor, grinding_factor, field_extension,
    fri_folding_factor, fri_remainder_max_degree) -- argument order of winter-air 0.8.
    blowup_factor: a power of two in [2, 128]; 32, 64 and 128 need trace_length * blowup_factor <= 2^24 and a
    last FRI layer of at least blowup_factor points (else XfgStarkError 6). fri_folding_factor: 2, 4, 8 or 16."""

    def __init__(self, num_queries, blowup_factor, grinding_factor, field_extension, fri_folding_factor,
                 fri_remainder_max_degree):
        self.num_queries = num_queries
        self.blowup_factor = blowup_factor
        self.grinding_factor = grinding_factor
        self.field_extension = field_extension
        self.fri_folding_factor = fri_folding_factor
        self.fri_remainder_max_degree = fri_remainder_max_degree

    @classmethod
    def reference(cls):
        """XfgBurnMintProver::new's ProofOptions::new(42, 8, 4, None, 8, 31) (src/burn_mint_prover.rs:28-35)."""
        o = _Options()
        _lib.xfg_default_options(C.byref(o))
        return cls._from_c(o)

    @classmethod
    def _from_c(cls, o):
        return cls(*_option_values(o))

    def _c(self):
        return _Options(*_option_values(self))

    def _c_and_bound(self, trace_length):
        """(xfg_options, xfg_proof_size_bound of a proof of `trace_length` under them)"""
        o = self._c()
        return o, _lib.xfg_proof_size_bound(trace_length, C.byref(o))

    def security_level(self, trace_length):
        """StarkProof::security_level(conjectured = true) of a proof of `trace_length` under these options, in
        bits (xfg_security_level); options outside the supported set raise XfgStarkError 9"""
        o, bits = self._c(), C.c_uint32()
        st = _lib.xfg_security_level(trace_length, C.byref(o), C.byref(bits))
        if st:
            raise XfgStarkError(st, f"no security level for trace length {trace_length} under {self!r}")
        return bits.value

    def __repr__(self):
        return ("ProofOptions(num_queries={0.num_queries}, blowup_factor={0.blowup_factor}, grinding_factor="
                "{0.grinding_factor}, field_extension={0.field_extension}, fri_folding_factor="
                "{0.fri_folding_factor}, fri_remainder_max_degree={0.fri_remainder_max_degree})").format(self)


class AcceptableOptions:
    """winterfell::AcceptableOptions, the verifier's policy: option_set([ProofOptions, ...]) takes a proof whose
    six options equal one member's (1..32 members), min_conjectured_security(bits) one whose conjectured
    security level is at least `bits`. MinProvenSecurity is not offered. The library's own limits (cubic
    extension, LDE sizes, last FRI layer) hold under either: see xfg_verify_acceptable in the header."""

    def __init__(self, kind, options=(), min_security=0):
        self.kind, self.options, self.min_security = kind, list(options), min_security

    @classmethod
    def option_set(cls, options):
        return cls(ACCEPT_OPTION_SET, options=options)

    @classmethod
    def min_conjectured_security(cls, bits):
        return cls(ACCEPT_MIN_CONJECTURED_SECURITY, min_security=bits)

    def _c(self):
        """the xfg_acceptable; the option array it points to stays alive on the struct"""
        arr = (_Options * len(self.options))(*[o._c() for o in self.options])
        a = _Acceptable(self.kind, self.min_security, arr if self.options else None, len(self.options))
        a._keep = arr
        return a

    def __repr__(self):
        if self.kind == ACCEPT_MIN_CONJECTURED_SECURITY:
            return f"AcceptableOptions.min_conjectured_security({self.min_security})"
        return f"AcceptableOptions.option_set({self.options!r})"


class StarkProof:
    """Serialized winterfell::StarkProof (to_bytes layout: DESIGN.md "Proof format").
    StarkProof.from_bytes parses and validates the structure (xfg_proof_parse); the parsed header is
    exposed as attributes (trace_length, options, num_unique_queries, pow_nonce, ...)."""

    def __init__(self, data: bytes):
        self._data = bytes(data)
        self._info = None

    @classmethod
    def from_bytes(cls, data: bytes):
        p = cls(data)
        p._parse()
        return p

    def _parse(self):
        if self._info is None:
            info, err = _ProofInfo(), C.create_string_buffer(256)
            st = _lib.xfg_proof_parse(bytes_ptr(self._data), len(self._data), C.byref(info), err, 256)
            if st:
                raise XfgStarkError(st, err.value.decode())
            self._info = info
        return self._info

    def to_bytes(self) -> bytes:
        return self._data

    @property
    def trace_length(self):
        return self._parse().trace_length

    @property
    def options(self):
        return ProofOptions._from_c(self._parse().options)

    @property
    def num_unique_queries(self):
        return self._parse().num_unique_queries

    @property
    def num_fri_layers(self):
        return self._parse().num_fri_layers

    @property
    def remainder_len(self):
        """FRI remainder coefficients (E elements)"""
        return self._parse().remainder_len

    @property
    def pow_nonce(self):
        return self._parse().pow_nonce

    @property
    def trace_root(self):
        return bytes(self._parse().trace_root)

    @property
    def constraint_root(self):
        return bytes(self._parse().constraint_root)

    @property
    def ood_frame(self):
        """([T_c(z)], [T_c(z g)], H(z))"""
        i = self._parse()
        return list(i.ood_trace[0::2]), list(i.ood_trace[1::2]), i.ood_composition

    def security_level(self):
        """StarkProof::security_level(conjectured = true): the level of the options and trace length the proof
        states (ProofOptions.security_level)"""
        return self.options.security_level(self.trace_length)

    def __len__(self):
        return len(self._data)

    def __eq__(self, other):
        return isinstance(other, StarkProof) and other._data == self._data


class XfgBurnMintVerifier:
    """Mirror of the reference XfgBurnMintVerifier (src/burn_mint_verifier.rs:78-316) over
    xfg_verify. The statement of a proof is its AIR constants `air` = (public inputs[12], nullifier,
    commitment), as returned by air_consts(); acceptable options default to the reference's
    ProofOptions::new(42, 8, 4, None, 8, 31) (:95-110). `acceptable` (an AcceptableOptions) is Winterfell's
    policy argument: with None the verifier takes the one-element set of `proof_options`, as the reference
    does (:271); with a policy every verify call goes through the xfg_*_acceptable entries and
    `proof_options` is not consulted."""

    def __init__(self, security_parameter=128, proof_options=None, acceptable=None):
        self.security_parameter = security_parameter
        self.proof_options = proof_options or ProofOptions.reference()
        self.acceptable = acceptable

    @classmethod
    def with_options(cls, security_parameter, proof_options):
        return cls(security_parameter, proof_options)

    def _entry(self, name):
        """(the C entry `name` or its _acceptable form, the options or the policy it takes)"""
        if self.acceptable is None:
            return getattr(_lib, name), self.proof_options._c()
        return getattr(_lib, name + "_acceptable"), self.acceptable._c()

    def verify_with_details(self, proof, air):
        """-> (accepted, error text or None, proof size)"""
        data = proof.to_bytes() if isinstance(proof, StarkProof) else bytes(proof)
        a, err = air_struct(air), C.create_string_buffer(256)
        fn, o = self._entry("xfg_verify")
        st = fn(bytes_ptr(data), len(data), C.byref(a), C.byref(o), err, 256)
        if st not in (0, 10):
            raise XfgStarkError(st, STATUS.get(st))
        return st == 0, (err.value.decode() or None), len(data)

    def verify_with_public_inputs(self, proof, air):
        return self.verify_with_details(proof, air)[0]

    def verify_burn_mint(self, proof, burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret,
                         network_id=1, target_chain_id=42161, commitment_version=1):
        """statement rebuilt from the prover's inputs (the full 32-byte tx hash limbs included: the
        reference's zeroed limbs at :146-150 would reject every honest proof)"""
        air = air_consts(burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id,
                         target_chain_id, commitment_version)
        return self.verify_with_public_inputs(proof, air)

    def batch_verify(self, proofs_and_airs, threads=0, gpu=None):
        """BatchBurnMintVerifier::verify_batch: list of (proof, air) -> list of bool. Host threads, or
        the GPU of `gpu` (an XfgBurnMintProver context) via xfg_verify_batch_gpu."""
        k = len(proofs_and_airs)
        if k == 0:
            return []
        keep, ptrs, lens, airs, res = self._batch_args(proofs_and_airs)
        if gpu is not None:
            fn, o = self._entry("xfg_verify_batch_gpu")
            gpu._call(fn, k, ptrs, lens, airs, C.byref(o), res)
        else:
            fn, o = self._entry("xfg_verify_batch")
            st = fn(k, ptrs, lens, airs, C.byref(o), res, threads)
            if st:
                raise XfgStarkError(st, STATUS.get(st))
        return [r == 0 for r in res]

    def _batch_args(self, proofs_and_airs):
        """the C arguments of a batch: (objects to keep alive, proofs, lens, airs, results)"""
        k = len(proofs_and_airs)
        datas = [(p.to_bytes() if isinstance(p, StarkProof) else bytes(p)) for p, _ in proofs_and_airs]
        ptrs = (_u8p * k)(*[bytes_ptr(d) for d in datas])
        lens = (C.c_size_t * k)(*[len(d) for d in datas])
        air_np, airs = air_array(a for _, a in proofs_and_airs)
        return (datas, air_np), ptrs, lens, airs, (C.c_int * k)()

    def debug_batch_verify(self, proofs_and_airs, gpu):
        """batch_verify(..., gpu=gpu) with what the device decided (xfg_debug_verify_batch_gpu): list of
        (accepted, flag word the verifier kernels set, error text or None) per item"""
        k = len(proofs_and_airs)
        if k == 0:
            return []
        keep, ptrs, lens, airs, res = self._batch_args(proofs_and_airs)
        flags = (C.c_uint64 * k)()
        stride = 256
        errs = C.create_string_buffer(k * stride)
        fn, o = self._entry("xfg_debug_verify_batch_gpu")
        gpu._call(fn, k, ptrs, lens, airs, C.byref(o), res, flags, errs, stride)
        texts = [errs.raw[i * stride:(i + 1) * stride].split(b"\0", 1)[0].decode() for i in range(k)]
        return [(res[i] == 0, int(flags[i]), texts[i] or None) for i in range(k)]

    def verify_all(self, proofs_and_airs, threads=0):
        return all(self.batch_verify(proofs_and_airs, threads))


def blake3(data: bytes) -> bytes:
    """the library's host BLAKE3 (any length)"""
    out = (C.c_uint8 * 32)()
    _lib.xfg_selftest_blake3(bytes_ptr(bytes(data)), len(data), out)
    return bytes(out)


def burn_inputs(burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id=1,
                target_chain_id=42161, commitment_version=1):
    """pack prove_burn_mint arguments; keeps the referenced byte strings alive on the struct"""
    tx = bytes(tx_prefix_hash)
    if len(tx) != 32:
        raise XfgStarkError(9, "tx_prefix_hash must be 32 bytes ([u8; 32])")
    s = _BurnInputs()
    s.burn_amount = burn_amount
    s.mint_amount = mint_amount
    s.tx_prefix_hash = (C.c_uint8 * 32)(*tx)
    rcpt, sec = bytes(recipient_address), bytes(secret)
    s._keep = (rcpt, sec)
    s.recipient_address = rcpt
    s.recipient_len = len(rcpt)
    s.secret = sec
    s.secret_len = len(sec)
    s.network_id = network_id
    s.target_chain_id = target_chain_id
    s.commitment_version = commitment_version
    return s


def _burn_array(inputs):
    """xfg_burn_inputs[len(inputs)] from dicts of prove_burn_mint kwargs -> (the array, the byte strings it
    points to: keep both until the library has marshalled them)"""
    arr, keep = (_BurnInputs * len(inputs))(), []
    for i, kw in enumerate(inputs):
        s = burn_inputs(**kw)
        keep.append(s._keep)
        arr[i] = s
    return arr, keep


def air_consts(burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id=1,
               target_chain_id=42161, commitment_version=1):
    """(public inputs[12], nullifier, commitment) exactly as the prover derives them (host-side)."""
    s = burn_inputs(burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id,
                    target_chain_id, commitment_version)
    a = _AirConsts()
    st = _lib.xfg_burn_air_consts(C.byref(s), C.byref(a))
    if st:
        raise XfgStarkError(st, STATUS[st])
    return list(a.pub_inputs), a.nullifier, a.commitment


def pack_records(inputs):
    """dicts of prove_burn_mint kwargs -> their xfg_burn_record's as a [count, 128] uint8 numpy array (the packed
    records a sharded run scatters). A record has room for exactly a 20-byte recipient and a 32-byte secret:
    shorter ones are zero-filled and longer ones cut, so statements that depend on either length being refused
    (statuses 4 and 5) cannot be expressed as records"""
    out = zeros((len(inputs), RECORD_BYTES), "uint8")
    for i, kw in enumerate(inputs):
        tx = bytes(kw["tx_prefix_hash"])
        if len(tx) != 32:
            raise XfgStarkError(9, "tx_prefix_hash must be 32 bytes ([u8; 32])")
        r = _BurnRecord.from_buffer(out[i])
        r.burn_amount, r.mint_amount = kw["burn_amount"], kw["mint_amount"]
        r.tx_prefix_hash[:] = tx
        r.recipient[:] = bytes(kw["recipient_address"]).ljust(20, b"\0")[:20]
        r.secret[:] = bytes(kw["secret"]).ljust(32, b"\0")[:32]
        r.network_id = kw.get("network_id", 1)
        r.target_chain_id = kw.get("target_chain_id", 42161)
        r.commitment_version = kw.get("commitment_version", 1)
    return out


def unpack_records(records):
    """the inverse of pack_records: [count, 128] uint8 -> dicts of prove_burn_mint kwargs (the reserved bytes are
    not part of a statement and are dropped)"""
    a = array(records, "uint8").reshape(-1, RECORD_BYTES).copy()
    res = []
    for row in a:
        r = _BurnRecord.from_buffer(row)
        res.append(dict(burn_amount=r.burn_amount, mint_amount=r.mint_amount, tx_prefix_hash=bytes(r.tx_prefix_hash),
                        recipient_address=bytes(r.recipient), secret=bytes(r.secret), network_id=r.network_id,
                        target_chain_id=r.target_chain_id, commitment_version=r.commitment_version))
    return res


def _record_view(records, device=None):
    """the C arguments of `count` records: (object to keep alive, pointer, count, flags). A C-contiguous uint8 numpy
    array of 128 * count bytes is host memory; a uint8 torch.Tensor must lie on cuda:`device` and goes to the
    library as it is (its current stream is synchronised first: the data is complete before the lanes read it)"""
    if hasattr(records, "data_ptr"):  # a torch.Tensor (torch itself is not imported here)
        t = records
        if device is None or t.device.type != "cuda" or (t.device.index or 0) != device:
            raise XfgStarkError(9, f"records tensor is on {t.device}, the prover on device {device}")
        if str(t.dtype) != "torch.uint8" or not t.is_contiguous() or t.numel() % RECORD_BYTES:
            raise XfgStarkError(9, "records tensor must be contiguous uint8, 128 bytes per record")
        if t.numel():
            import torch
            torch.cuda.current_stream(t.device).synchronize()
        return t, t.data_ptr() or None, t.numel() // RECORD_BYTES, RECORDS_ON_DEVICE
    a = records
    if not (hasattr(a, "ctypes") and str(a.dtype) == "uint8" and a.flags.c_contiguous and a.size % RECORD_BYTES == 0):
        raise XfgStarkError(9, "records: a C-contiguous uint8 numpy array of 128 bytes per record, or a tensor")
    return a, a.ctypes.data or None, a.size // RECORD_BYTES, 0


def air_consts_from_records(records, prover=None):
    """the statement of each record as the verifiers take it (xfg_air_consts_from_records): a list of
    (public inputs[12], nullifier, commitment), an XfgStarkError in the place of an invalid record. Host records
    are computed on the host; a tensor on `prover`'s device by the prover's record kernel"""
    keep, where, count, flags = _record_view(records, getattr(prover, "_device", None))
    airs, sts = (_AirConsts * max(count, 1))(), (C.c_int * max(count, 1))()
    if prover is not None:
        prover._call(_lib.xfg_air_consts_from_records, count, where, flags, airs, sts)
    else:
        st = _lib.xfg_air_consts_from_records(None, count, where, flags, airs, sts)
        if st:
            raise XfgStarkError(st, STATUS.get(st))
    return [XfgStarkError(sts[i], STATUS.get(sts[i])) if sts[i] else
            (list(airs[i].pub_inputs), airs[i].nullifier, airs[i].commitment) for i in range(count)]


def record_size(count, trace_length, options):
    """bytes of a fixed-size batch record (XfgBurnMintProver.submit_batch_record): `count` int64
    proof lengths, then `count` slots of xfg_proof_size_bound bytes, proof i at slot i"""
    return 8 * count + count * options._c_and_bound(trace_length)[1]


class PendingBatch:
    """a submitted batch (XfgBurnMintProver.submit_batch); result() -> list of StarkProof | XfgStarkError.
    A batch is consumed once: by result() (which can be called again and returns the same list),
    by packed_into(), or -- for a batch written into a caller's record -- by record_ready()."""

    def __init__(self, prover, ticket, buf, base, cap, outs, lens, sts, record=False, owner=None, faults=None):
        self._p, self._t, self._buf, self._base, self._cap = prover, ticket, buf, base, cap
        self._outs, self._lens, self._sts = outs, lens, sts
        self._record = record  # proofs live in the caller's record: no pooled buffer to release
        # the object owning the caller's record: kept alive while the workers may still write into
        # it (until the batch has been waited for, here or in __del__)
        self._owner = owner
        # a batch of caller-supplied traces (submit_traces): the xfg_trace_fault array the wait fills;
        # owner then holds the traces (array or device tensor), which the lanes read until the wait
        self._faults = faults
        self._res = None
        self._consumed = None  # name of the call that consumed the batch, if not result()

    def _release(self):
        if self._buf is not None:
            self._p._free.append(self._buf)
            self._buf = None

    def wait(self):
        """block until every proof of the batch is done (idempotent); the batch's status code"""
        if not hasattr(self, "_wst"):
            self._wst = _lib.xfg_batch_wait(self._p._ctx, self._t)
        return self._wst

    def _check_unconsumed(self, what):
        if self._consumed:
            raise XfgStarkError(9, f"{what} after {self._consumed}(): the batch was already consumed")

    def _first_failure(self):
        """the error of the first proof that failed, or None (a slice of a ctypes array is a list)"""
        st = next(filter(None, self._sts[:]), 0)
        return XfgStarkError(st, STATUS.get(st)) if st else None

    def result(self):
        if self._res is None:
            self._check_unconsumed("result")
            st = self.wait()
            if st:
                self._release()
                raise self._p._err(st)
            res = []
            for i in range(len(self._sts)):
                if self._sts[i]:
                    fault = TraceFault._from_c(self._faults[i]) if self._faults is not None else None
                    err = XfgStarkError(self._sts[i], str(fault) if fault else STATUS.get(self._sts[i]))
                    err.fault = fault  # TraceFault of an INVALID_TRACE / non-canonical proof, else None
                    res.append(err)
                else:
                    res.append(StarkProof(C.string_at(self._base + i * self._cap, self._lens[i])))
            self._release()
            self._res = res
        return self._res

    def record_ready(self):
        """wait for a batch submitted with submit_batch_record; its record (lengths + fixed slots)
        is then complete in the caller's buffer. A failed proof raises (its length is zeroed in the
        record first, so a record that travels anyway cannot be read as a proof)."""
        if not self._record:
            raise XfgStarkError(9, "record_ready: the batch was not submitted into a record")
        self._check_unconsumed("record_ready")
        if self._res is not None:
            raise XfgStarkError(9, "record_ready after result()")
        self._consumed = "record_ready"
        st = self.wait()
        # a batch-level failure leaves every status 0 and the header words at the capacity the
        # submission wrote: zero them all, so the record cannot be read as cap-byte proofs
        bad = self._first_failure()
        if st or bad:
            for i, failed in enumerate(self._sts[:]):
                if st or failed:
                    self._lens[i] = 0
            raise self._p._err(st) if st else bad
        return 8 * len(self._sts) + self._cap * len(self._sts)

    def record_views(self):
        """after record_ready(): every proof of the batch as a zero-copy memoryview into the caller's
        record (valid while the record is neither freed nor reused)"""
        if self._consumed != "record_ready" or not hasattr(self, "_wst") or self._wst or any(self._sts[:]):
            raise XfgStarkError(9, "record_views: call record_ready() first (and it must have succeeded)")
        return [memoryview((C.c_uint8 * self._cap).from_address(self._base + i * self._cap)).cast("B")[:self._lens[i]]
                for i in range(len(self._sts))]

    def packed_into(self, dst):
        """wait, then write the batch as one record into the uint8 numpy array `dst`: count int64
        lengths followed by the proof bytes back to back, straight from the workers' output buffer
        -- no per-proof bytes objects. Returns the record size. Any per-proof error raises."""
        if self._res is not None:
            raise XfgStarkError(9, "packed_into after result(): the batch's buffer was released")
        self._check_unconsumed("packed_into")
        self._consumed = "packed_into"
        st = self.wait()
        if st:
            self._release()
            raise self._p._err(st)
        k = len(self._sts)
        bad = self._first_failure()
        lens = array([self._lens[i] for i in range(k)], "int64")
        hdr = 8 * k
        need = hdr + int(lens.sum())
        if bad or need > dst.size:
            self._release()
            raise bad or XfgStarkError(8, "packed_into: destination too small")
        dst[:hdr] = lens.view("uint8")
        base, off = dst.ctypes.data, hdr
        for i in range(k):
            C.memmove(base + off, self._base + i * self._cap, int(lens[i]))
            off += int(lens[i])
        self._release()
        return need

    def __del__(self, _finalizing=sys.is_finalizing):
        # the workers write into this batch's buffers: never release them before the batch is done;
        # a batch that was waited for but never consumed returns its buffer to the pool (the
        # finalizing check is bound at definition: module globals, `sys` included, are gone late in
        # interpreter teardown)
        if not _finalizing() and getattr(self._p, "_ctx", None):
            if self._res is None and not hasattr(self, "_wst"):
                _lib.xfg_batch_wait(self._p._ctx, self._t)
            self._release()


class XfgBurnMintProver(KernelHooks):
    """reference XfgBurnMintProver (src/burn_mint_prover.rs:18-244) on one MI355X device. The kernel-level
    test hooks (debug_*) come from KernelHooks."""

    def __init__(self, security_parameter=128, device=0, proof_options=None):
        self._security_parameter = security_parameter
        self._options = proof_options or ProofOptions.reference()
        self._device = device
        self._free = []  # host output buffers of finished batches, taken again by _take_buffer
        self._ctx = _lib.xfg_ctx_create(device)
        if not self._ctx:
            raise XfgStarkError(7, f"no HIP device {device} available for libxfgstark (no CPU fallback)")

    @classmethod
    def new(cls, security_parameter=128, device=0):
        return cls(security_parameter, device)

    @classmethod
    def with_options(cls, security_parameter, proof_options, device=0):
        return cls(security_parameter, device, proof_options)

    def close(self):
        if getattr(self, "_ctx", None):
            _lib.xfg_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self, _finalizing=sys.is_finalizing):
        # at interpreter exit the module globals (`sys` and the HIP runtime included) may already be
        # gone -- hence the check bound at definition; process teardown releases the device buffers,
        # so only collect contexts dropped while running
        if not _finalizing():
            self.close()

    def _err(self, st):
        buf = C.create_string_buffer(1024)
        _lib.xfg_last_error(self._ctx, buf, 1024)
        return XfgStarkError(st, buf.value.decode() or STATUS.get(st, str(st)))

    def _call(self, fn, *args):
        """fn(context, *args) for an entry that returns a status; a status other than XFG_OK raises"""
        st = fn(self._ctx, *args)
        if st:
            raise self._err(st)

    def security_parameter(self):
        return self._security_parameter

    def proof_options(self):
        return self._options

    def get_proof_size(self, proof: StarkProof) -> int:
        return len(proof.to_bytes())

    def proof_size_bound(self, trace_length) -> int:
        """the largest proof this prover emits for `trace_length` under its options (xfg_proof_size_bound)"""
        return self._options._c_and_bound(trace_length)[1]

    def _prove_one(self, fn, trace_length, *args):
        """fn(context, *args, options, out, out_len) -> the StarkProof it wrote"""
        o, cap = self._options._c_and_bound(trace_length)
        buf = C.create_string_buffer(cap)
        ln = C.c_size_t(cap)
        self._call(fn, *args, C.byref(o), C.cast(buf, _u8p), C.byref(ln))
        return StarkProof(C.string_at(buf, ln.value))

    def prove_burn_mint(self, burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id=1,
                        target_chain_id=42161, commitment_version=1, trace_length=64) -> StarkProof:
        s = burn_inputs(burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id,
                        target_chain_id, commitment_version)
        return self._prove_one(_lib.xfg_prove_burn_mint, trace_length, C.byref(s), trace_length)

    def prove_trace(self, trace, pub_inputs, nullifier, commitment) -> StarkProof:
        """ExecutionTrace-level proving; trace = 7 columns of n canonical u64 (column-major)."""
        tr = array(trace)
        width, n = tr.shape
        a = air_struct((pub_inputs, nullifier, commitment))
        return self._prove_one(_lib.xfg_prove_trace, n, ptr(tr), width, n, C.byref(a))

    def prove_batch(self, inputs, trace_length=64):
        """list of dicts of prove_burn_mint kwargs -> list of StarkProof | XfgStarkError (per proof)."""
        return self.submit_batch(inputs, trace_length).result()

    def _submit(self, fn, head, k, cap, tail=(), buf=None, record=None, **pending):
        """submit k proofs of bound `cap` through the asynchronous entry fn(context, *head, outs, lens, statuses,
        *tail, ticket) -> PendingBatch. The proofs go into the pooled buffer `buf`, which returns to the pool if
        the library refuses the batch, or into the slots behind the k length words at address `record`"""
        base = C.addressof(buf) if record is None else record + 8 * k
        outs, lens, sts = out_slots(k, cap, base, record)
        ticket = C.c_uint64(0)
        try:
            self._call(fn, *head, outs, lens, sts, *tail, C.byref(ticket))
        except XfgStarkError:
            if buf is not None:
                self._free.append(buf)
            raise
        return PendingBatch(self, ticket.value, buf, base, cap, outs, lens, sts, record=record is not None, **pending)

    def submit_batch(self, inputs, trace_length=64):
        """asynchronous prove_batch (xfg_prove_batch_submit): inputs are validated and marshalled
        now, proving runs on the context's lane workers; PendingBatch.result() waits. Submitting
        the next batch before collecting this one overlaps their host and device work."""
        k = len(inputs)
        arr, keep = _burn_array(inputs)
        o, cap = self._options._c_and_bound(trace_length)
        return self._submit(_lib.xfg_prove_batch_submit, (k, arr, trace_length, C.byref(o)), k, cap,
                            buf=self._take_buffer(cap * k))

    def submit_batch_record(self, inputs, trace_length, addr, nbytes, owner=None):
        """submit_batch whose output is a caller-owned fixed-size record at host address `addr`
        (record_size bytes): the workers write proof i into slot i and its length into header word
        i, so the record can be handed to a collective (bench.py's exchange step) without packing.
        The record must stay untouched until PendingBatch.record_ready() returns; `owner` (the
        tensor, array or ctypes buffer holding it) is referenced by the PendingBatch so that the
        memory stays valid at least that long -- without it the caller must keep the record alive."""
        k = len(inputs)
        o, cap = self._options._c_and_bound(trace_length)
        if k == 0 or cap == 0 or nbytes < 8 * k + cap * k:
            raise XfgStarkError(9, f"submit_batch_record: record of {nbytes} B for {k} proofs of bound {cap} B")
        arr, keep = _burn_array(inputs)
        return self._submit(_lib.xfg_prove_batch_submit, (k, arr, trace_length, C.byref(o)), k, cap,
                            record=addr, owner=owner)

    def submit_records(self, records, trace_length=64):
        """asynchronous prove_records (xfg_prove_records_submit) -> PendingBatch. records: the statements as packed
        xfg_burn_record's (pack_records), a C-contiguous uint8 numpy array [count, 128] or a uint8 torch.Tensor of
        the same bytes on the prover's device. A tensor is read where it lies by the lanes' record kernel: nothing
        is copied to the host and no statement is marshalled there before the launch. It is referenced by the
        PendingBatch until the batch has been waited for and must not be written before then. As for
        prove_traces, torch and the library must share one HIP runtime"""
        keep, where, count, flags = _record_view(records, self._device)
        o, cap = self._options._c_and_bound(trace_length)
        return self._submit(_lib.xfg_prove_records_submit, (count, where, trace_length, C.byref(o), flags), count, cap,
                            buf=self._take_buffer(cap * count), owner=keep)

    def prove_records(self, records, trace_length=64):
        """prove_batch for packed records (host array or device tensor, see submit_records) -> list of
        StarkProof | XfgStarkError (per proof): the same proofs and statuses as prove_batch(unpack_records(...))"""
        return self.submit_records(records, trace_length).result()

    def air_consts_from_records(self, records):
        """air_consts_from_records(records) with a tensor on this prover's device going through the record kernel
        (refused while batches are pending)"""
        return air_consts_from_records(records, prover=self)

    def last_error(self):
        """the text of the last failing call or proof on this context (xfg_last_error), "" when there is none"""
        buf = C.create_string_buffer(1024)
        _lib.xfg_last_error(self._ctx, buf, 1024)
        return buf.value.decode()

    def _trace_view(self, traces, airs):
        """the C arguments of a batch of traces of logical shape [count][7][n]: (objects to keep alive, pointer,
        count, width, n, airs array, flags, layout). layout: None for contiguous data, which goes to the entries
        without a layout as it always has; else the (trace, column, row) strides in 8-byte words of a strided
        tensor or array, which goes to the _strided entries as it lies"""
        if hasattr(traces, "data_ptr"):  # a torch.Tensor (torch itself is not imported here)
            t = traces
            if t.device.type != "cuda" or (t.device.index or 0) != self._device:
                raise XfgStarkError(9, f"traces tensor is on {t.device}, the prover on device {self._device}")
            if str(t.dtype) not in ("torch.int64", "torch.uint64"):
                raise XfgStarkError(9, "traces tensor must have dtype int64 or uint64")
            shape, keep, flags = tuple(t.shape), t, TRACE_ON_DEVICE
            layout = None if t.is_contiguous() or len(shape) != 3 else tuple(t.stride())
            if len(shape) == 3 and t.numel():
                import torch
                torch.cuda.current_stream(t.device).synchronize()  # the data is complete before the lanes read it
            where = t.data_ptr()
        else:
            a, layout = trace_array(traces)
            shape, keep, flags, where = a.shape, a, 0, a.ctypes.data
        if len(shape) != 3:
            raise XfgStarkError(9, "traces: [count][7][n]")
        count, width, n = shape
        if layout is not None and (width != 7 or min(layout) < 0):  # a layout names seven columns
            raise XfgStarkError(9, "XfgBurnMintAir traces have 7 columns" if width != 7
                                else "traces: a view with a negative stride is not supported")
        if len(airs) != count:
            raise XfgStarkError(9, f"{count} traces, {len(airs)} AIR constants")
        air_np, air_p = air_array(airs)
        return (keep, air_np), where or None, count, width, n, air_p, flags, layout

    def _trace_args(self, traces, airs):
        """_trace_view without the layout: (objects to keep alive, pointer, count, width, n, airs array, flags)"""
        return self._trace_view(traces, airs)[:7]

    def submit_traces(self, traces, airs, validate=False):
        """asynchronous prove_traces (xfg_prove_trace_batch_submit, or _strided_submit for a strided view) ->
        PendingBatch; the traces (array or tensor) are referenced by it until it has been waited for, and must
        not be written before then"""
        keep, where, count, width, n, air_p, flags, layout = self._trace_view(traces, airs)
        o, cap = self._options._c_and_bound(n) if count else (self._options._c(), 0)
        faults = (_TraceFault * count)()
        flags |= TRACE_VALIDATE if validate else 0
        if layout is None:
            fn, head = _lib.xfg_prove_trace_batch_submit, (count, where, width, n, air_p, C.byref(o), flags)
        else:
            at = _TraceLayout(*layout)
            keep = keep + (at,)
            fn, head = _lib.xfg_prove_trace_batch_strided_submit, (count, where, n, C.byref(at), air_p, C.byref(o), flags)
        return self._submit(fn, head, count, cap, tail=(faults,), buf=self._take_buffer(cap * count), owner=keep,
                            faults=faults)

    def prove_traces(self, traces, airs, validate=False):
        """ExecutionTrace-level proving of a batch: traces = numpy uint64 array or int64 / uint64 torch.Tensor
        on the prover's device, of logical shape [count][7][n] with any non-negative strides: row-major data
        [count][n][7] is rows.permute(0, 2, 1) (numpy: rows.transpose(0, 2, 1)), rows padded to 8 words are
        rows[..., :7].permute(0, 2, 1). A strided view is read where it lies, without a copy (a host array
        whose strides are not multiples of 8 bytes is copied first). airs = count x
        (pub_inputs[12], nullifier, commitment) -> list of StarkProof | XfgStarkError (per proof).
        validate: Trace::validate on the device first; a trace that violates the AIR gives an
        XfgStarkError of status 11 (INVALID_TRACE) whose .fault is the TraceFault and whose text is
        Winterfell's message, the other proofs are unaffected.
        A tensor's data_ptr() goes to the library as it is, so torch and the library must share one HIP
        runtime: with a torch build that bundles its own, import torch before this package (the library
        then binds to the runtime torch loaded); a pointer the library's runtime does not know is refused"""
        return self.submit_traces(traces, airs, validate).result()

    def check_traces(self, traces, airs):
        """Trace::validate on the device alone (xfg_check_traces, or xfg_check_traces_strided for a strided
        view: traces as for prove_traces): -> list of TraceFault | None"""
        keep, where, count, width, n, air_p, flags, layout = self._trace_view(traces, airs)
        if width != 7:
            raise XfgStarkError(9, "XfgBurnMintAir traces have 7 columns")
        faults = (_TraceFault * max(count, 1))()
        if layout is None:
            self._call(_lib.xfg_check_traces, count, where, n, air_p, flags, faults)
        else:
            self._call(_lib.xfg_check_traces_strided, count, where, n, C.byref(_TraceLayout(*layout)), air_p, flags, faults)
        return [TraceFault._from_c(faults[i]) for i in range(count)]

    def _take_buffer(self, size):
        """a host output buffer of `size` bytes: a recycled one, else a new mapping (_marshal.new_buffer)"""
        for i, b in enumerate(self._free):
            if C.sizeof(b) >= size:
                return self._free.pop(i)
        return new_buffer(size)

    def prepare(self, count, trace_length=64, buffers=0):
        """allocate workspaces for batches of `count` proofs of this shape (setup, untimed), and
        `buffers` host output buffers for submit_batch, their pages touched now -- as many as the
        caller keeps batches in flight, so steady-state submissions allocate nothing"""
        o, cap = self._options._c_and_bound(trace_length)
        self._call(_lib.xfg_prepare, count, trace_length, C.byref(o))
        if buffers:
            size = cap * count
            have = sum(1 for b in self._free if C.sizeof(b) >= size)
            self._free += [new_buffer(size, touch=True) for _ in range(max(0, buffers - have))]

    # ---- instrumentation
    def set_timing(self, on=True):
        _lib.xfg_set_timing(self._ctx, 1 if on else 0)

    def stage_times(self):
        ms = (C.c_double * 16)()
        names = (C.c_char_p * 16)()
        k = _lib.xfg_stage_times(self._ctx, ms, names, 16)
        return {names[i].decode(): ms[i] for i in range(k)}

    def bench_lde(self, count, n, blowup, iters):
        avg = C.c_double()
        self._call(_lib.xfg_bench_lde, count, n, blowup, iters, C.byref(avg))
        return avg.value

    def lde_probe(self, enabled):
        """(total ms, launch sets, polynomials) of the trace-LDE launch sets timed in the proving
        pipeline since the last lde_probe(True) (HIP events on the launching lane's stream)"""
        ms, sets, polys = C.c_double(), C.c_uint64(), C.c_uint64()
        self._call(_lib.xfg_lde_probe, 1 if enabled else 0, C.byref(ms), C.byref(sets), C.byref(polys))
        return ms.value, sets.value, polys.value

    def grind_probe(self):
        """(GRIND_DEVICE_MIN, proofs whose nonce this context searched on the device, on the host)"""
        dmin, dev, host = C.c_uint32(), C.c_uint64(), C.c_uint64()
        self._call(_lib.xfg_grind_probe, C.byref(dmin), C.byref(dev), C.byref(host))
        return dmin.value, dev.value, host.value
