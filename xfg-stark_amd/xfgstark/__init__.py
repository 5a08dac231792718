"""xfgstark -- Python mirror of the reference prover API over the MI355X C ABI (libxfgstark.so).

Mirrors reference src/burn_mint_prover.rs (XfgBurnMintProver::new / with_options /
prove_burn_mint / get_proof_size / security_parameter / proof_options) and the Winterfell
ProofOptions / StarkProof surface it returns. All proving runs in libxfgstark.so (HIP kernels
for gfx950); there is no CPU fallback: if the library is missing this module fails to import, and
without a GPU the prover constructor raises.
"""
import ctypes as C
import mmap
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
# XFG_LIB: an alternative build of the same library (same-box A/B of kernel variants)
LIB_PATH = os.environ.get("XFG_LIB") or os.path.join(_PKG, "libxfgstark.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "xfg_stark.h")

if not os.path.exists(LIB_PATH):
    raise ImportError(f"libxfgstark.so not built at {LIB_PATH}: run `make -C xfg-stark_amd` "
                      "(or __graft_entry__.build()); the prover has no CPU fallback")

_lib = C.CDLL(LIB_PATH)

STATUS = {0: "OK", 1: "INVALID_BURN_AMOUNT", 2: "MINT_MISMATCH", 3: "ZERO_TX_HASH", 4: "BAD_RECIPIENT_LEN",
          5: "SHORT_SECRET", 6: "PROVER_ERROR", 7: "DEVICE_ERROR", 8: "BUFFER_TOO_SMALL", 9: "INVALID_ARGUMENT",
          10: "VERIFY_FAILED", 11: "INVALID_TRACE"}
TRACE_VALIDATE, TRACE_ON_DEVICE = 1, 2  # XFG_TRACE_* flags of xfg_prove_trace_batch


class _Options(C.Structure):
    _fields_ = [("num_queries", C.c_uint32), ("blowup_factor", C.c_uint32), ("grinding_factor", C.c_uint32),
                ("field_extension", C.c_uint32), ("fri_folding_factor", C.c_uint32),
                ("fri_remainder_max_degree", C.c_uint32)]


class _BurnInputs(C.Structure):
    _fields_ = [("burn_amount", C.c_uint64), ("mint_amount", C.c_uint64), ("tx_prefix_hash", C.c_uint8 * 32),
                ("recipient_address", C.c_char_p), ("recipient_len", C.c_size_t), ("secret", C.c_char_p),
                ("secret_len", C.c_size_t), ("network_id", C.c_uint32), ("target_chain_id", C.c_uint32),
                ("commitment_version", C.c_uint32)]


class _AirConsts(C.Structure):
    _fields_ = [("pub_inputs", C.c_uint64 * 12), ("nullifier", C.c_uint64), ("commitment", C.c_uint64)]


class _ProofInfo(C.Structure):
    _fields_ = [("trace_width", C.c_uint32), ("trace_length", C.c_uint64), ("options", _Options),
                ("num_unique_queries", C.c_uint32), ("num_fri_layers", C.c_uint32), ("remainder_len", C.c_uint32),
                ("pow_nonce", C.c_uint64), ("trace_root", C.c_uint8 * 32), ("constraint_root", C.c_uint8 * 32),
                ("ood_trace", C.c_uint64 * 14), ("ood_composition", C.c_uint64), ("size", C.c_size_t)]


class _TraceFault(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32), ("column", C.c_uint32), ("step", C.c_uint64),
                ("expected", C.c_uint64), ("found", C.c_uint64)]


_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)
_lib.xfg_ctx_create.restype = C.c_void_p
_lib.xfg_ctx_create.argtypes = [C.c_int]
_lib.xfg_ctx_destroy.argtypes = [C.c_void_p]
_lib.xfg_default_options.argtypes = [C.POINTER(_Options)]
_lib.xfg_last_error.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
_lib.xfg_proof_size_bound.restype = C.c_size_t
_lib.xfg_proof_size_bound.argtypes = [C.c_uint64, C.POINTER(_Options)]
_lib.xfg_prove_burn_mint.argtypes = [C.c_void_p, C.POINTER(_BurnInputs), C.c_uint64, C.POINTER(_Options), _u8p,
                                     C.POINTER(C.c_size_t)]
_lib.xfg_prove_trace.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, C.POINTER(_AirConsts),
                                 C.POINTER(_Options), _u8p, C.POINTER(C.c_size_t)]
_lib.xfg_prove_batch.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_BurnInputs), C.c_uint64, C.POINTER(_Options),
                                 C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
_lib.xfg_prove_batch_submit.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_BurnInputs), C.c_uint64,
                                         C.POINTER(_Options), C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
_lib.xfg_batch_wait.argtypes = [C.c_void_p, C.c_uint64]
_lib.xfg_proof_parse.argtypes = [_u8p, C.c_size_t, C.POINTER(_ProofInfo), C.c_char_p, C.c_size_t]
_lib.xfg_verify.argtypes = [_u8p, C.c_size_t, C.POINTER(_AirConsts), C.POINTER(_Options), C.c_char_p, C.c_size_t]
_lib.xfg_verify_batch.argtypes = [C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(_AirConsts),
                                  C.POINTER(_Options), C.POINTER(C.c_int), C.c_uint32]
_lib.xfg_verify_batch_gpu.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                      C.POINTER(_AirConsts), C.POINTER(_Options), C.POINTER(C.c_int)]
if hasattr(_lib, "xfg_debug_verify_batch_gpu"):  # absent from builds older than the verifier flag word
    _lib.xfg_debug_verify_batch_gpu.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                                C.POINTER(_AirConsts), C.POINTER(_Options), C.POINTER(C.c_int),
                                                _u64p, C.c_char_p, C.c_size_t]
_lib.xfg_selftest_blake3.argtypes = [_u8p, C.c_size_t, _u8p]
_lib.xfg_prepare.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(_Options)]
_lib.xfg_burn_air_consts.argtypes = [C.POINTER(_BurnInputs), C.POINTER(_AirConsts)]
_lib.xfg_set_timing.argtypes = [C.c_void_p, C.c_int]
_lib.xfg_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_char_p), C.c_int]
_lib.xfg_bench_lde.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
_lib.xfg_lde_probe.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64)]
_lib.xfg_debug_lde.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, C.c_uint32, _u64p]
_lib.xfg_debug_ood_deep.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]
if hasattr(_lib, "xfg_debug_ood_deep_e"):  # absent from builds older than the OOD / DEEP hook in E (XFG_LIB A/B)
    _lib.xfg_debug_ood_deep_e.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, _u64p, _u64p, _u64p, _u64p,
                                          C.POINTER(C.c_uint32), _u64p, C.c_uint64, _u64p, _u64p, _u64p,
                                          C.POINTER(C.c_uint32), _u64p, C.POINTER(C.c_int)]
_lib.xfg_debug_interpolate.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, C.c_int, _u64p]
if hasattr(_lib, "xfg_debug_const_columns"):  # absent from builds older than the constant-column skip (XFG_LIB A/B)
    _lib.xfg_debug_const_columns.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint32, C.c_uint64, _u8p]
    _lib.xfg_debug_lde_skip.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, C.c_uint32, _u8p, _u64p]
    _lib.xfg_debug_interpolate_skip.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, C.c_int, _u8p, _u64p]
if hasattr(_lib, "xfg_debug_interpolate_keep"):  # absent from builds older than the truncated inverse hook (XFG_LIB A/B)
    _lib.xfg_debug_interpolate_keep.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, _u64p]
if hasattr(_lib, "xfg_debug_constraint_eval"):  # absent from builds older than the kernel-level parity hooks
    _lib.xfg_debug_constraint_eval.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _u64p,
                                               C.POINTER(_AirConsts), _u64p, _u64p]
    _lib.xfg_debug_fri_fold.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u64p,
                                        _u64p, _u64p]
if hasattr(_lib, "xfg_debug_field"):  # absent from builds older than the primitive self test (XFG_LIB A/B)
    _lib.xfg_debug_field.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, _u64p, _u64p, _u64p]
if hasattr(_lib, "xfg_debug_coin_draws"):  # absent from builds older than the device transcript
    _lib.xfg_debug_coin_draws.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32, C.c_uint32,
                                          _u64p, _u64p, _u64p, _u64p, C.POINTER(C.c_int)]
if hasattr(_lib, "xfg_debug_merkle_lde"):  # absent from builds older than the whole-heap Merkle test
    _lib.xfg_debug_merkle_lde.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _u64p, _u64p,
                                          C.c_uint64, _u8p, _u8p]
    _lib.xfg_debug_merkle_fri.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _u64p,
                                          _u8p]
if hasattr(_lib, "xfg_debug_merkle_lde_const"):  # absent from builds that fill the constant columns' planes (XFG_LIB A/B)
    _lib.xfg_debug_merkle_lde_const.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _u64p, _u8p,
                                                _u64p, _u64p, C.c_uint64, _u8p, _u8p]
    _lib.xfg_debug_poison_lde.argtypes = [C.c_void_p, C.c_int]
if hasattr(_lib, "xfg_debug_col_classes"):  # absent from builds without shared trace columns (XFG_LIB A/B)
    _lib.xfg_debug_col_classes.argtypes = [C.c_void_p, _u64p, C.c_uint32, C.c_uint64, _u8p, _u64p]
    _lib.xfg_debug_ood_deep_const.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, _u64p, _u8p, _u64p, _u64p,
                                              _u64p, _u64p, C.POINTER(C.c_uint32), _u64p, C.c_uint64, _u64p, _u64p,
                                              _u64p, C.POINTER(C.c_uint32), _u64p, C.POINTER(C.c_int)]
class _ProbePattern(C.Structure):
    _fields_ = [("kind", C.c_uint32 * 7), ("reserved", C.c_uint32), ("row", C.c_uint64 * 7), ("proof", C.c_uint64)]


if hasattr(_lib, "xfg_debug_trace_probe"):  # absent from builds that detect in the written trace (XFG_LIB A/B)
    _lib.xfg_debug_trace_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(_AirConsts), C.c_uint32,
                                           C.POINTER(_ProbePattern), _u8p, _u64p, _u64p]
if hasattr(_lib, "xfg_debug_fri_fold_f"):  # absent from builds older than folding factors 2, 4 and 16
    _lib.xfg_debug_fri_fold_f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_uint32, _u64p, _u64p, _u64p]
    _lib.xfg_debug_merkle_fri_f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                            C.c_uint32, _u64p, _u8p]
if hasattr(_lib, "xfg_debug_grind"):  # absent from builds older than the device proof-of-work search (XFG_LIB A/B)
    _lib.xfg_debug_grind.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_uint64,
                                     C.c_uint32, C.c_uint32, _u64p]
    _lib.xfg_grind_probe.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), _u64p, _u64p]
if hasattr(_lib, "xfg_prove_trace_batch"):  # absent from builds older than the trace batches (XFG_LIB A/B)
    _lib.xfg_check_traces.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(_AirConsts),
                                      C.c_uint32, C.POINTER(_TraceFault)]
    _lib.xfg_prove_trace_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64,
                                           C.POINTER(_AirConsts), C.POINTER(_Options), C.c_uint32, C.POINTER(_u8p),
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(_TraceFault)]
    _lib.xfg_prove_trace_batch_submit.argtypes = _lib.xfg_prove_trace_batch.argtypes + [C.POINTER(C.c_uint64)]


class XfgStarkError(Exception):
    """XfgStarkError::CryptoError(String) (reference src/lib.rs:66-110); `.status` is the C-ABI code."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status
        self.kind = STATUS.get(status, str(status))


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
        return cls(o.num_queries, o.blowup_factor, o.grinding_factor, o.field_extension, o.fri_folding_factor,
                   o.fri_remainder_max_degree)

    def _c(self):
        return _Options(self.num_queries, self.blowup_factor, self.grinding_factor, self.field_extension,
                        self.fri_folding_factor, self.fri_remainder_max_degree)

    def __repr__(self):
        return ("ProofOptions(num_queries={0.num_queries}, blowup_factor={0.blowup_factor}, grinding_factor="
                "{0.grinding_factor}, field_extension={0.field_extension}, fri_folding_factor="
                "{0.fri_folding_factor}, fri_remainder_max_degree={0.fri_remainder_max_degree})").format(self)


def _bytes_ptr(b):
    return C.cast(C.c_char_p(b), _u8p)


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
            st = _lib.xfg_proof_parse(_bytes_ptr(self._data), len(self._data), C.byref(info), err, 256)
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
        o = self._parse().options
        return ProofOptions(o.num_queries, o.blowup_factor, o.grinding_factor, o.field_extension,
                            o.fri_folding_factor, o.fri_remainder_max_degree)

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

    def __len__(self):
        return len(self._data)

    def __eq__(self, other):
        return isinstance(other, StarkProof) and other._data == self._data


def _air_struct(air):
    pub, nullifier, commitment = air
    a = _AirConsts()
    a.pub_inputs = (C.c_uint64 * 12)(*pub)
    a.nullifier = nullifier
    a.commitment = commitment
    return a


class XfgBurnMintVerifier:
    """Mirror of the reference XfgBurnMintVerifier (src/burn_mint_verifier.rs:78-316) over
    xfg_verify. The statement of a proof is its AIR constants `air` = (public inputs[12], nullifier,
    commitment), as returned by air_consts(); acceptable options default to the reference's
    ProofOptions::new(42, 8, 4, None, 8, 31) (:95-110)."""

    def __init__(self, security_parameter=128, proof_options=None):
        self.security_parameter = security_parameter
        self.proof_options = proof_options or ProofOptions.reference()

    @classmethod
    def with_options(cls, security_parameter, proof_options):
        return cls(security_parameter, proof_options)

    def verify_with_details(self, proof, air):
        """-> (accepted, error text or None, proof size)"""
        data = proof.to_bytes() if isinstance(proof, StarkProof) else bytes(proof)
        a, o, err = _air_struct(air), self.proof_options._c(), C.create_string_buffer(256)
        st = _lib.xfg_verify(_bytes_ptr(data), len(data), C.byref(a), C.byref(o), err, 256)
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
        keep, ptrs, lens, airs, res, o = self._batch_args(proofs_and_airs)
        if gpu is not None:
            st = _lib.xfg_verify_batch_gpu(gpu._ctx, k, ptrs, lens, airs, C.byref(o), res)
            if st:
                raise gpu._err(st)
            return [r == 0 for r in res]
        st = _lib.xfg_verify_batch(k, ptrs, lens, airs, C.byref(o), res, threads)
        if st:
            raise XfgStarkError(st, STATUS.get(st))
        return [r == 0 for r in res]

    def _batch_args(self, proofs_and_airs):
        """the C arguments of a batch: (objects to keep alive, proofs, lens, airs, results, options)"""
        import numpy as np
        k = len(proofs_and_airs)
        datas = [(p.to_bytes() if isinstance(p, StarkProof) else bytes(p)) for p, _ in proofs_and_airs]
        # statements as one numpy array (per-item ctypes structs dominated large batches)
        ptrs = (_u8p * k)(*[_bytes_ptr(d) for d in datas])
        lens = (C.c_size_t * k)(*[len(d) for d in datas])
        air_np = np.array([list(a[0]) + [a[1], a[2]] for _, a in proofs_and_airs], dtype=np.uint64)
        airs = air_np.ctypes.data_as(C.POINTER(_AirConsts))
        return (datas, air_np), ptrs, lens, airs, (C.c_int * k)(), self.proof_options._c()

    def debug_batch_verify(self, proofs_and_airs, gpu):
        """batch_verify(..., gpu=gpu) with what the device decided (xfg_debug_verify_batch_gpu): list of
        (accepted, flag word the verifier kernels set, error text or None) per item"""
        k = len(proofs_and_airs)
        if k == 0:
            return []
        keep, ptrs, lens, airs, res, o = self._batch_args(proofs_and_airs)
        flags = (C.c_uint64 * k)()
        stride = 256
        errs = C.create_string_buffer(k * stride)
        st = _lib.xfg_debug_verify_batch_gpu(gpu._ctx, k, ptrs, lens, airs, C.byref(o), res, flags, errs, stride)
        if st:
            raise gpu._err(st)
        texts = [errs.raw[i * stride:(i + 1) * stride].split(b"\0", 1)[0].decode() for i in range(k)]
        return [(res[i] == 0, int(flags[i]), texts[i] or None) for i in range(k)]

    def verify_all(self, proofs_and_airs, threads=0):
        return all(self.batch_verify(proofs_and_airs, threads))


def blake3(data: bytes) -> bytes:
    """the library's host BLAKE3 (any length)"""
    out = (C.c_uint8 * 32)()
    _lib.xfg_selftest_blake3(_bytes_ptr(bytes(data)), len(data), out)
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


def exported_symbols():
    return [name for name in dir(_lib)]


def _anon_map(size):
    """private anonymous mapping (the default mmap.mmap(-1, n) is MAP_SHARED: shmem pages, slower
    to fault and to write than the private pages malloc hands out)"""
    return mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)


def record_size(count, trace_length, options):
    """bytes of a fixed-size batch record (XfgBurnMintProver.submit_batch_record): `count` int64
    proof lengths, then `count` slots of xfg_proof_size_bound bytes, proof i at slot i"""
    o = options._c()
    return 8 * count + count * _lib.xfg_proof_size_bound(trace_length, C.byref(o))


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
        bad = [i for i in range(len(self._sts)) if self._sts[i]]
        # a batch-level failure leaves every status 0 and the header words at the capacity the
        # submission wrote: zero them all, so the record cannot be read as cap-byte proofs
        for i in (range(len(self._sts)) if st else bad):
            self._lens[i] = 0
        if st:
            raise self._p._err(st)
        if bad:
            raise XfgStarkError(self._sts[bad[0]], STATUS.get(self._sts[bad[0]]))
        return 8 * len(self._sts) + self._cap * len(self._sts)

    def record_views(self):
        """after record_ready(): every proof of the batch as a zero-copy memoryview into the caller's
        record (valid while the record is neither freed nor reused)"""
        if (self._consumed != "record_ready" or not hasattr(self, "_wst") or self._wst
                or any(self._sts[i] for i in range(len(self._sts)))):
            raise XfgStarkError(9, "record_views: call record_ready() first (and it must have succeeded)")
        return [memoryview((C.c_uint8 * self._cap).from_address(self._base + i * self._cap)).cast("B")[:self._lens[i]]
                for i in range(len(self._sts))]

    def packed_into(self, dst):
        """wait, then write the batch as one record into the uint8 numpy array `dst`: count int64
        lengths followed by the proof bytes back to back, straight from the workers' output buffer
        -- no per-proof bytes objects. Returns the record size. Any per-proof error raises."""
        import numpy as np
        if self._res is not None:
            raise XfgStarkError(9, "packed_into after result(): the batch's buffer was released")
        self._check_unconsumed("packed_into")
        self._consumed = "packed_into"
        st = self.wait()
        if st:
            self._release()
            raise self._p._err(st)
        k = len(self._sts)
        bad = [i for i in range(k) if self._sts[i]]
        lens = np.array([self._lens[i] for i in range(k)], dtype=np.int64)
        hdr = 8 * k
        need = hdr + int(lens.sum())
        if bad or need > dst.size:
            self._release()
            if bad:
                raise XfgStarkError(self._sts[bad[0]], STATUS.get(self._sts[bad[0]]))
            raise XfgStarkError(8, "packed_into: destination too small")
        dst[:hdr] = lens.view(np.uint8)
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


class XfgBurnMintProver:
    """reference XfgBurnMintProver (src/burn_mint_prover.rs:18-244) on one MI355X device."""

    def __init__(self, security_parameter=128, device=0, proof_options=None):
        self._security_parameter = security_parameter
        self._options = proof_options or ProofOptions.reference()
        self._device = device
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

    def security_parameter(self):
        return self._security_parameter

    def proof_options(self):
        return self._options

    def get_proof_size(self, proof: StarkProof) -> int:
        return len(proof.to_bytes())

    def proof_size_bound(self, trace_length) -> int:
        """the largest proof this prover emits for `trace_length` under its options (xfg_proof_size_bound)"""
        o = self._options._c()
        return _lib.xfg_proof_size_bound(trace_length, C.byref(o))

    def prove_burn_mint(self, burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id=1,
                        target_chain_id=42161, commitment_version=1, trace_length=64) -> StarkProof:
        s = burn_inputs(burn_amount, mint_amount, tx_prefix_hash, recipient_address, secret, network_id,
                        target_chain_id, commitment_version)
        o = self._options._c()
        cap = _lib.xfg_proof_size_bound(trace_length, C.byref(o))
        buf = C.create_string_buffer(cap)
        ln = C.c_size_t(cap)
        st = _lib.xfg_prove_burn_mint(self._ctx, C.byref(s), trace_length, C.byref(o), C.cast(buf, _u8p), C.byref(ln))
        if st:
            raise self._err(st)
        return StarkProof(C.string_at(buf, ln.value))

    def prove_trace(self, trace, pub_inputs, nullifier, commitment) -> StarkProof:
        """ExecutionTrace-level proving; trace = 7 columns of n canonical u64 (column-major)."""
        import numpy as np
        tr = np.ascontiguousarray(np.asarray(trace, dtype=np.uint64))
        width, n = tr.shape
        a = _AirConsts()
        a.pub_inputs = (C.c_uint64 * 12)(*pub_inputs)
        a.nullifier = nullifier
        a.commitment = commitment
        o = self._options._c()
        cap = _lib.xfg_proof_size_bound(n, C.byref(o))
        buf = C.create_string_buffer(cap)
        ln = C.c_size_t(cap)
        st = _lib.xfg_prove_trace(self._ctx, tr.ctypes.data_as(_u64p), width, n, C.byref(a), C.byref(o),
                                  C.cast(buf, _u8p), C.byref(ln))
        if st:
            raise self._err(st)
        return StarkProof(C.string_at(buf, ln.value))

    def prove_batch(self, inputs, trace_length=64):
        """list of dicts of prove_burn_mint kwargs -> list of StarkProof | XfgStarkError (per proof)."""
        return self.submit_batch(inputs, trace_length).result()

    def submit_batch(self, inputs, trace_length=64):
        """asynchronous prove_batch (xfg_prove_batch_submit): inputs are validated and marshalled
        now, proving runs on the context's lane workers; PendingBatch.result() waits. Submitting
        the next batch before collecting this one overlaps their host and device work."""
        k = len(inputs)
        arr = (_BurnInputs * k)()
        keep = []
        for i, kw in enumerate(inputs):
            s = burn_inputs(**kw)
            keep.append(s._keep)
            arr[i] = s
        o = self._options._c()
        cap = _lib.xfg_proof_size_bound(trace_length, C.byref(o))
        buf = self._take_buffer(cap * k)
        base = C.addressof(buf)
        outs = (_u8p * k)(*[C.cast(base + i * cap, _u8p) for i in range(k)])
        lens = (C.c_size_t * k)(*([cap] * k))
        sts = (C.c_int * k)()
        ticket = C.c_uint64(0)
        st = _lib.xfg_prove_batch_submit(self._ctx, k, arr, trace_length, C.byref(o), outs, lens, sts,
                                         C.byref(ticket))
        if st:
            self._free.append(buf)
            raise self._err(st)
        return PendingBatch(self, ticket.value, buf, base, cap, outs, lens, sts)

    def submit_batch_record(self, inputs, trace_length, addr, nbytes, owner=None):
        """submit_batch whose output is a caller-owned fixed-size record at host address `addr`
        (record_size bytes): the workers write proof i into slot i and its length into header word
        i, so the record can be handed to a collective (bench.py's exchange step) without packing.
        The record must stay untouched until PendingBatch.record_ready() returns; `owner` (the
        tensor, array or ctypes buffer holding it) is referenced by the PendingBatch so that the
        memory stays valid at least that long -- without it the caller must keep the record alive."""
        k = len(inputs)
        o = self._options._c()
        cap = _lib.xfg_proof_size_bound(trace_length, C.byref(o))
        if k == 0 or cap == 0 or nbytes < 8 * k + cap * k:
            raise XfgStarkError(9, f"submit_batch_record: record of {nbytes} B for {k} proofs of bound {cap} B")
        arr = (_BurnInputs * k)()
        keep = []
        for i, kw in enumerate(inputs):
            s = burn_inputs(**kw)
            keep.append(s._keep)
            arr[i] = s
        base = addr + 8 * k
        outs = (_u8p * k)(*[C.cast(base + i * cap, _u8p) for i in range(k)])
        lens = (C.c_size_t * k).from_address(addr)  # the record's header: capacity in, length out
        for i in range(k):
            lens[i] = cap
        sts = (C.c_int * k)()
        ticket = C.c_uint64(0)
        st = _lib.xfg_prove_batch_submit(self._ctx, k, arr, trace_length, C.byref(o), outs, lens, sts,
                                         C.byref(ticket))
        if st:
            raise self._err(st)
        return PendingBatch(self, ticket.value, None, base, cap, outs, lens, sts, record=True, owner=owner)

    def _trace_args(self, traces, airs):
        """the C arguments of a batch of traces: (object to keep alive, pointer, count, n, airs array, flags)"""
        import numpy as np
        if hasattr(traces, "data_ptr"):  # a torch.Tensor (torch itself is not imported here)
            t = traces
            if t.device.type != "cuda" or (t.device.index or 0) != self._device:
                raise XfgStarkError(9, f"traces tensor is on {t.device}, the prover on device {self._device}")
            if str(t.dtype) not in ("torch.int64", "torch.uint64") or not t.is_contiguous():
                raise XfgStarkError(9, "traces tensor must be contiguous with dtype int64 or uint64")
            shape, keep, flags = tuple(t.shape), t, TRACE_ON_DEVICE
            if len(shape) == 3 and t.numel():
                import torch
                torch.cuda.current_stream(t.device).synchronize()  # the data is complete before the lanes copy it
            ptr = t.data_ptr()
        else:
            a = np.ascontiguousarray(np.asarray(traces, dtype=np.uint64))
            shape, keep, flags, ptr = a.shape, a, 0, a.ctypes.data
        if len(shape) != 3:
            raise XfgStarkError(9, "traces: [count][7][n]")
        count, width, n = shape
        if len(airs) != count:
            raise XfgStarkError(9, f"{count} traces, {len(airs)} AIR constants")
        air_np = np.array([list(a[0]) + [a[1], a[2]] for a in airs], dtype=np.uint64).reshape(count, 14)
        return (keep, air_np), ptr or None, count, width, n, air_np.ctypes.data_as(C.POINTER(_AirConsts)), flags

    def submit_traces(self, traces, airs, validate=False):
        """asynchronous prove_traces (xfg_prove_trace_batch_submit) -> PendingBatch; the traces (array or
        tensor) are referenced by it until it has been waited for, and must not be written before then"""
        keep, ptr, count, width, n, air_p, flags = self._trace_args(traces, airs)
        o = self._options._c()
        cap = _lib.xfg_proof_size_bound(n, C.byref(o)) if count else 0
        buf = self._take_buffer(cap * count)
        base = C.addressof(buf)
        outs = (_u8p * count)(*[C.cast(base + i * cap, _u8p) for i in range(count)])
        lens = (C.c_size_t * count)(*([cap] * count))
        sts = (C.c_int * count)()
        faults = (_TraceFault * count)()
        ticket = C.c_uint64(0)
        st = _lib.xfg_prove_trace_batch_submit(self._ctx, count, ptr, width, n, air_p, C.byref(o),
                                               flags | (TRACE_VALIDATE if validate else 0), outs, lens, sts, faults,
                                               C.byref(ticket))
        if st:
            self._free.append(buf)
            raise self._err(st)
        return PendingBatch(self, ticket.value, buf, base, cap, outs, lens, sts, owner=keep, faults=faults)

    def prove_traces(self, traces, airs, validate=False):
        """ExecutionTrace-level proving of a batch: traces = numpy uint64 array [count][7][n] or a
        contiguous int64 / uint64 torch.Tensor of that shape on the prover's device, airs = count x
        (pub_inputs[12], nullifier, commitment) -> list of StarkProof | XfgStarkError (per proof).
        validate: Trace::validate on the device first; a trace that violates the AIR gives an
        XfgStarkError of status 11 (INVALID_TRACE) whose .fault is the TraceFault and whose text is
        Winterfell's message, the other proofs are unaffected.
        A tensor's data_ptr() goes to the library as it is, so torch and the library must share one HIP
        runtime: with a torch build that bundles its own, import torch before this package (the library
        then binds to the runtime torch loaded); a pointer the library's runtime does not know is refused"""
        return self.submit_traces(traces, airs, validate).result()

    def check_traces(self, traces, airs):
        """Trace::validate on the device alone (xfg_check_traces): -> list of TraceFault | None"""
        keep, ptr, count, width, n, air_p, flags = self._trace_args(traces, airs)
        if width != 7:
            raise XfgStarkError(9, "XfgBurnMintAir traces have 7 columns")
        faults = (_TraceFault * max(count, 1))()
        st = _lib.xfg_check_traces(self._ctx, count, ptr, n, air_p, flags, faults)
        if st:
            raise self._err(st)
        return [TraceFault._from_c(faults[i]) for i in range(count)]

    def _take_buffer(self, size):
        # output buffers are recycled. A new one is an anonymous mapping, not create_string_buffer:
        # that zero-fills the whole bound (64 x 0.7 MB at n = 2^16) on the calling thread -- 11 ms
        # of page faults per batch, during which the next batch could not be submitted. The
        # mapping's pages are faulted in by the workers' proof copies instead, once.
        free = self.__dict__.setdefault("_free", [])
        for i, b in enumerate(free):
            if C.sizeof(b) >= size:
                return free.pop(i)
        # at least one byte: an anonymous mapping of length 0 raises ValueError before the C library
        # could report the invalid request (empty batch, trace length with no size bound)
        size = max(size, 1)
        return (C.c_char * size).from_buffer(_anon_map(size))

    def prepare(self, count, trace_length=64, buffers=0):
        """allocate workspaces for batches of `count` proofs of this shape (setup, untimed), and
        `buffers` host output buffers for submit_batch, their pages touched now -- as many as the
        caller keeps batches in flight, so steady-state submissions allocate nothing"""
        o = self._options._c()
        st = _lib.xfg_prepare(self._ctx, count, trace_length, C.byref(o))
        if st:
            raise self._err(st)
        if buffers:
            size = _lib.xfg_proof_size_bound(trace_length, C.byref(o)) * count
            free = self.__dict__.setdefault("_free", [])
            have = sum(1 for b in free if C.sizeof(b) >= size)
            for _ in range(max(0, buffers - have)):
                b = (C.c_char * size).from_buffer(_anon_map(size))
                C.memset(b, 0, size)  # fault the pages in at setup
                free.append(b)

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
        st = _lib.xfg_bench_lde(self._ctx, count, n, blowup, iters, C.byref(avg))
        if st:
            raise self._err(st)
        return avg.value

    def lde_probe(self, enabled):
        """(total ms, launch sets, polynomials) of the trace-LDE launch sets timed in the proving
        pipeline since the last lde_probe(True) (HIP events on the launching lane's stream)"""
        ms, sets, polys = C.c_double(), C.c_uint64(), C.c_uint64()
        st = _lib.xfg_lde_probe(self._ctx, 1 if enabled else 0, C.byref(ms), C.byref(sets), C.byref(polys))
        if st:
            raise self._err(st)
        return ms.value, sets.value, polys.value

    def debug_lde(self, coef, n, blowup):
        import numpy as np
        c = np.ascontiguousarray(np.asarray(coef, dtype=np.uint64)).reshape(-1, n)
        out = np.zeros((c.shape[0], n * blowup), dtype=np.uint64)
        st = _lib.xfg_debug_lde(self._ctx, c.ctypes.data_as(_u64p), c.shape[0], n, blowup, out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out

    def debug_lde_skip(self, coef, n, blowup, skip):
        """debug_lde with a flag per polynomial: flagged ones (vouched constant by the caller) take no
        transform and are filled in, as the prover does for the constant columns it detects"""
        import numpy as np
        c = np.ascontiguousarray(np.asarray(coef, dtype=np.uint64)).reshape(-1, n)
        f = np.ascontiguousarray(np.asarray(skip, dtype=np.uint8))
        if f.shape != (c.shape[0],):
            raise XfgStarkError(9, "debug_lde_skip: one flag per polynomial")
        out = np.zeros((c.shape[0], n * blowup), dtype=np.uint64)
        st = _lib.xfg_debug_lde_skip(self._ctx, c.ctypes.data_as(_u64p), c.shape[0], n, blowup, f.ctypes.data_as(_u8p),
                                     out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out

    def debug_const_columns(self, trace):
        """the prover's constant-column detection: trace [B,width,n] -> flags [B,width] (1 = one value in every row)"""
        import numpy as np
        tr = np.ascontiguousarray(trace, dtype=np.uint64)
        B, width, n = tr.shape
        out = np.zeros((B, width), dtype=np.uint8)
        st = _lib.xfg_debug_const_columns(self._ctx, tr.ctypes.data_as(_u64p), B, width, n, out.ctypes.data_as(_u8p))
        if st:
            raise self._err(st)
        return out

    def debug_col_classes(self, trace, values=False):
        """the unit's column detection as the prover runs it (xfg_debug_col_classes): trace [B,7,n] -> classes
        [B,7], 0 live, 1 constant, 2 the same as trace 0's column; values=True: also element 0 of every column"""
        import numpy as np
        tr = np.ascontiguousarray(trace, dtype=np.uint64)
        B, width, n = tr.shape
        if width != 7:
            raise XfgStarkError(9, "debug_col_classes: trace [B,7,n]")
        out = np.zeros((B, 7), dtype=np.uint8)
        vals = np.zeros((B, 7), dtype=np.uint64)
        st = _lib.xfg_debug_col_classes(self._ctx, tr.ctypes.data_as(_u64p), B, n, out.ctypes.data_as(_u8p),
                                        vals.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return (out, vals) if values else out

    def debug_trace_probe(self, airs, n, generator=0, pattern=None):
        """the front end of a unit of generated traces (xfg_debug_trace_probe): airs = B air_consts() tuples;
        generator 0 the burn AIR's rows, 1 the synthetic rows of pattern = (kind[7], row[7], proof) ->
        (classes [B,7], values [B,7], trace buffer [B,7,n] as left: unwritten planes are 0xFF bytes)"""
        import numpy as np
        B = len(airs)
        arr = (_AirConsts * B)(*[_air_struct(a) for a in airs])
        pat = _ProbePattern()
        if pattern is not None:
            kind, row, proof = pattern
            pat.kind = (C.c_uint32 * 7)(*kind)
            pat.row = (C.c_uint64 * 7)(*row)
            pat.proof = proof
        cls = np.zeros((B, 7), dtype=np.uint8)
        vals = np.zeros((B, 7), dtype=np.uint64)
        tr = np.zeros((B, 7, n), dtype=np.uint64)
        st = _lib.xfg_debug_trace_probe(self._ctx, B, n, arr, generator, C.byref(pat) if pattern is not None else None,
                                        cls.ctypes.data_as(_u8p), vals.ctypes.data_as(_u64p), tr.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return cls, vals, tr

    def debug_ood_deep_const(self, coef, flags, vals, hcoef, zpts, coeffs):
        """debug_ood_deep_e without coins on coefficients behind a column descriptor (xfg_debug_ood_deep_const):
        flags [B,7] 1 = constant with value vals [B,7], 2 = the coefficients of instance 0's column; the
        flagged planes of coef are replaced by 0xFF bytes on the device -> (ood [B,15,ext], deep [B,ext,n])"""
        import numpy as np
        c = np.ascontiguousarray(coef, dtype=np.uint64)
        hc = np.ascontiguousarray(hcoef, dtype=np.uint64)
        zp = np.ascontiguousarray(zpts, dtype=np.uint64)
        co = np.ascontiguousarray(coeffs, dtype=np.uint64)
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        B, _, n = c.shape
        ext = hc.shape[1]
        if (c.shape[1] != 7 or hc.shape != (B, ext, n) or zp.shape != (B, 2, ext) or co.shape != (B, 8, ext)
                or f.shape != (B, 7) or v.shape != (B, 7)):
            raise XfgStarkError(9, "debug_ood_deep_const: coef [B,7,n], flags and vals [B,7], hcoef [B,ext,n], "
                                   "zpts [B,2,ext], coeffs [B,8,ext]")
        ood = np.zeros((B, 15, ext), dtype=np.uint64)
        deep = np.zeros((B, ext, n), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(_u64p)
        st = _lib.xfg_debug_ood_deep_const(self._ctx, B, n, ext, p(c), f.ctypes.data_as(_u8p), p(v), p(hc), p(zp), p(co),
                                           None, None, 0, p(ood), p(deep), None, None, None, None)
        if st:
            raise self._err(st)
        return ood, deep

    def debug_ood_deep(self, coef, hcoef, zpts, coeffs):
        """OOD + DEEP kernels: coef [B,7,n], hcoef [B,n], zpts [B,2], coeffs [B,8] -> (ood [B,15], deep [B,n])"""
        import numpy as np
        c = np.ascontiguousarray(coef, dtype=np.uint64)
        B, _, n = c.shape
        hc = np.ascontiguousarray(hcoef, dtype=np.uint64)
        zp = np.ascontiguousarray(zpts, dtype=np.uint64)
        co = np.ascontiguousarray(coeffs, dtype=np.uint64)
        ood = np.zeros((B, 15), dtype=np.uint64)
        deep = np.zeros((B, n), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(_u64p)
        st = _lib.xfg_debug_ood_deep(self._ctx, B, n, p(c), p(hc), p(zp), p(co), p(ood), p(deep))
        if st:
            raise self._err(st)
        return ood, deep

    def debug_ood_deep_e(self, coef, hcoef, zpts, coeffs=None, coins=None, ginv=0):
        """OOD + DEEP kernels in the field of degree ext (xfg_debug_ood_deep_e): coef [B,7,n], hcoef [B,ext,n],
        zpts [B,2,ext]. Without `coins`: coeffs [B,8,ext] -> (ood [B,15,ext], deep [B,ext,n]). With coins = B x
        (32-byte seed, counter) and ginv = 1 / g, the prover's launches with the DEEP transcript step ->
        (ood, deep, dp [B,14,2] = a_0..a_6, gamma, z, zg, 1/z, 1/zg, c1, c2, coins afterwards, fail [B]).
        Shapes are passed on as they are: the library refuses what it does not support"""
        import numpy as np
        c = np.ascontiguousarray(coef, dtype=np.uint64)
        hc = np.ascontiguousarray(hcoef, dtype=np.uint64)
        zp = np.ascontiguousarray(zpts, dtype=np.uint64)
        B, _, n = c.shape
        ext = hc.shape[1]
        if c.shape[1] != 7 or hc.shape != (B, ext, n) or zp.shape != (B, 2, ext):
            raise XfgStarkError(9, "debug_ood_deep_e: coef [B,7,n], hcoef [B,ext,n], zpts [B,2,ext]")
        ood = np.zeros((B, 15, ext), dtype=np.uint64)
        deep = np.zeros((B, ext, n), dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(_u64p)
        if coins is None:
            co = np.ascontiguousarray(coeffs, dtype=np.uint64)
            if co.shape != (B, 8, ext):
                raise XfgStarkError(9, "debug_ood_deep_e: coeffs [B,8,ext]")
            st = _lib.xfg_debug_ood_deep_e(self._ctx, B, n, ext, p(c), p(hc), p(zp), p(co), None, None, 0, p(ood),
                                           p(deep), None, None, None, None)
            if st:
                raise self._err(st)
            return ood, deep
        if len(coins) != B or any(len(bytes(sd)) != 32 for sd, _ in coins):
            raise XfgStarkError(9, "debug_ood_deep_e: coins are B x (32-byte seed, counter)")
        u32p = C.POINTER(C.c_uint32)
        seeds = np.frombuffer(b"".join(bytes(sd) for sd, _ in coins), dtype="<u4").copy()
        ctrs = np.array([ctr for _, ctr in coins], dtype=np.uint64)
        dp = np.zeros((B, 14, 2), dtype=np.uint64)
        seeds_out = np.zeros(B * 8, dtype="<u4")
        ctrs_out = np.zeros(B, dtype=np.uint64)
        fail = (C.c_int * max(B, 1))()
        st = _lib.xfg_debug_ood_deep_e(self._ctx, B, n, ext, p(c), p(hc), p(zp), None, seeds.ctypes.data_as(u32p),
                                       p(ctrs), ginv, p(ood), p(deep), p(dp), seeds_out.ctypes.data_as(u32p),
                                       p(ctrs_out), fail)
        if st:
            raise self._err(st)
        after = [(seeds_out[8 * b:8 * b + 8].tobytes(), int(ctrs_out[b])) for b in range(B)]
        return ood, deep, dp, after, [fail[b] for b in range(B)]

    def debug_constraint_eval(self, trace, airs, coeffs, blowup):
        """constraint evaluation kernel behind interpolation + LDE + the divisor table, as the prover
        runs them: trace [B,7,n], airs = B x (pub[12], nullifier, commitment), coeffs [B,15,ext]
        -> ce [B,ext,2n] in natural CE-domain order"""
        import numpy as np
        tr = np.ascontiguousarray(trace, dtype=np.uint64)
        co = np.ascontiguousarray(coeffs, dtype=np.uint64)
        B, width, n = tr.shape
        if width != 7 or co.ndim != 3 or co.shape[:2] != (B, 15) or len(airs) != B:
            raise XfgStarkError(9, "debug_constraint_eval: trace [B,7,n], airs [B], coeffs [B,15,ext]")
        ext = co.shape[2]
        arr = (_AirConsts * B)(*[_air_struct(a) for a in airs])
        ce = np.zeros((B, ext, 2 * n), dtype=np.uint64)
        st = _lib.xfg_debug_constraint_eval(self._ctx, B, n, blowup, ext, tr.ctypes.data_as(_u64p), arr,
                                            co.ctypes.data_as(_u64p), ce.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return ce

    def debug_fri_fold(self, vals, alpha, logn, logbeta, coset_major, fold=8):
        """FRI fold kernel (folding factor `fold` = 2, 4, 8 or 16): vals [B,ext,D] with D = 2^(logn + logbeta)
        >= 2 fold, natural order or coset-major (natural index K at (K mod beta) n + K // beta), alpha [B,ext]
        -> [B,ext,D/fold] (xfg_debug_fri_fold_f, which refuses any other fold or a smaller D)"""
        import numpy as np
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        al = np.ascontiguousarray(alpha, dtype=np.uint64)
        B, ext, D = v.shape
        if D != 1 << (logn + logbeta) or al.shape != (B, ext):
            raise XfgStarkError(9, "debug_fri_fold: vals [B,ext,2^(logn+logbeta)], alpha [B,ext]")
        if not 0 < fold < 1 << 32:
            raise XfgStarkError(9, "debug_fri_fold: fold is 2, 4, 8 or 16")
        out = np.zeros((B, ext, D // fold), dtype=np.uint64)
        st = _lib.xfg_debug_fri_fold_f(self._ctx, B, ext, logn, logbeta, 1 if coset_major else 0, fold,
                                       v.ctypes.data_as(_u64p), al.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out

    # ops from mul2_pair on read a, b as pairs (a[2i], a[2i+1]) and write both words of the result
    FIELD_OPS = {"mul": 0, "add": 1, "sub": 2, "canon": 3, "pow2": 4, "fold": 5, "sub_weak": 6, "add_w": 7, "mul2": 8,
                 "mul2_pair": 9, "e2_mul": 10, "e2_mulb": 11, "e2_inv": 12}

    def debug_field(self, op, a, b):
        """device Goldilocks primitive `op` (FIELD_OPS) applied elementwise to u64 arrays a, b"""
        import numpy as np
        x = np.ascontiguousarray(a, dtype=np.uint64)
        y = np.ascontiguousarray(b, dtype=np.uint64)
        out = np.zeros_like(x)
        st = _lib.xfg_debug_field(self._ctx, self.FIELD_OPS[op], x.size, x.ctypes.data_as(_u64p),
                                  y.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out

    def debug_coin_draws(self, seed, counter, k, ext=1, reject=(0, 0, 0, 0)):
        """device transcript draws (xfg_debug_coin_draws): seed = 32 bytes, k <= 64 draws of E by one
        wave and one at a time, with counters 1..256 force-rejected where `reject` (4 x u64 bits) is
        set. Returns (wave [k][2], sequential [k][2], counters (wave, seq), ok (wave, seq))"""
        import numpy as np
        w = (C.c_uint32 * 8)(*np.frombuffer(bytes(seed), dtype="<u4").tolist())
        rej = np.array(reject, dtype=np.uint64)
        ow = np.zeros((k, 2), dtype=np.uint64)
        osq = np.zeros((k, 2), dtype=np.uint64)
        ctr = np.zeros(2, dtype=np.uint64)
        ok = (C.c_int * 2)()
        st = _lib.xfg_debug_coin_draws(self._ctx, w, counter, k, ext, rej.ctypes.data_as(_u64p),
                                       ow.ctypes.data_as(_u64p), osq.ctypes.data_as(_u64p),
                                       ctr.ctypes.data_as(_u64p), ok)
        if st:
            raise self._err(st)
        return ow, osq, (int(ctr[0]), int(ctr[1])), (ok[0], ok[1])

    def debug_grind(self, seeds, grind, first_nonce=1, max_nonce=0, chunk_log=0, blocks=0):
        """the prover's proof-of-work search alone (xfg_debug_grind): seeds = 32-byte strings; for each the
        smallest nonce in [first_nonce, max_nonce] whose BLAKE3(seed || nonce_le8) has >= grind trailing
        zero bits in its first 8 LE bytes, 0 where there is none. max_nonce 0: the prover's bound
        2^(grind + 8); chunk_log / blocks 0: the planner's geometry, else forced (6..16, 1..4096)"""
        import numpy as np
        k = len(seeds)
        if any(len(bytes(sd)) != 32 for sd in seeds):
            raise XfgStarkError(9, "debug_grind: seeds are 32 bytes each")
        w = np.frombuffer(b"".join(bytes(sd) for sd in seeds), dtype="<u4").copy()
        out = np.zeros(k, dtype=np.uint64)
        st = _lib.xfg_debug_grind(self._ctx, k, w.ctypes.data_as(C.POINTER(C.c_uint32)), grind, first_nonce, max_nonce,
                                  chunk_log, blocks, out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return [int(v) for v in out]

    def grind_probe(self):
        """(GRIND_DEVICE_MIN, proofs whose nonce this context searched on the device, on the host)"""
        dmin, dev, host = C.c_uint32(), C.c_uint64(), C.c_uint64()
        st = _lib.xfg_grind_probe(self._ctx, C.byref(dmin), C.byref(dev), C.byref(host))
        if st:
            raise self._err(st)
        return dmin.value, dev.value, host.value

    def debug_merkle_lde(self, lde, entries=()):
        """Merkle commitment of LDEs as the prover runs it (xfg_debug_merkle_lde): lde [B,nc,blowup,n]
        coset-major, entries = proof << log2(n) | row. Returns (heaps [B,2n,8] u32 words -- slots
        [1, n) defined, the rest 0xFFFFFFFF -- and the opening kernel's local heaps [len(entries),2 blowup,8])"""
        import numpy as np
        v = np.ascontiguousarray(lde, dtype=np.uint64)
        ent = np.ascontiguousarray(entries, dtype=np.uint64)
        B, nc, blowup, n = v.shape
        nodes = np.zeros((B, 2 * n, 8), dtype="<u4")
        local = np.zeros((ent.size, 2 * blowup, 8), dtype="<u4")
        st = _lib.xfg_debug_merkle_lde(self._ctx, B, nc, n, blowup, v.ctypes.data_as(_u64p), ent.ctypes.data_as(_u64p),
                                       ent.size, nodes.ctypes.data_as(_u8p), local.ctypes.data_as(_u8p))
        if st:
            raise self._err(st)
        return nodes, local

    def debug_merkle_lde_const(self, lde, flags=None, vals=None, entries=()):
        """debug_merkle_lde for an LDE [B,7,blowup,n] with constant columns (xfg_debug_merkle_lde_const):
        flags [B,7] and vals [B,7] go to the kernels, and the flagged planes are set to 0xFF bytes on the
        device before the launches. flags = vals = None: the dense kernels, blowup up to 128"""
        import numpy as np
        v = np.ascontiguousarray(lde, dtype=np.uint64)
        ent = np.ascontiguousarray(entries, dtype=np.uint64)
        B, nc, blowup, n = v.shape
        if (flags is None) != (vals is None):
            raise XfgStarkError(9, "debug_merkle_lde_const: flags and vals go together")
        fp = vp = None
        if flags is not None:
            f = np.ascontiguousarray(flags, dtype=np.uint8)
            cv = np.ascontiguousarray(vals, dtype=np.uint64)
            if f.shape != (B, nc) or cv.shape != (B, nc):
                raise XfgStarkError(9, "debug_merkle_lde_const: flags [B,nc], vals [B,nc]")
            fp, vp = f.ctypes.data_as(_u8p), cv.ctypes.data_as(_u64p)
        nodes = np.zeros((B, 2 * n, 8), dtype="<u4")
        local = np.zeros((ent.size, 2 * blowup, 8), dtype="<u4")
        st = _lib.xfg_debug_merkle_lde_const(self._ctx, B, nc, n, blowup, v.ctypes.data_as(_u64p), fp, vp,
                                             ent.ctypes.data_as(_u64p), ent.size, nodes.ctypes.data_as(_u8p),
                                             local.ctypes.data_as(_u8p))
        if st:
            raise self._err(st)
        return nodes, local

    def debug_poison_lde(self, on):
        """while on, every unit sets its trace LDE buffer to 0xFF bytes before the transforms (xfg_debug_poison_lde)"""
        st = _lib.xfg_debug_poison_lde(self._ctx, 1 if on else 0)
        if st:
            raise self._err(st)

    def debug_merkle_fri(self, vals, logn, logbeta, coset_major, fold=8):
        """Merkle commitment of FRI layers (xfg_debug_merkle_fri_f): vals and fold as for debug_fri_fold. Returns the heaps [B,2 rows,8] u32 words, rows = 2^(logn + logbeta) / fold
        (slot 0: 0xFFFFFFFF)"""
        import numpy as np
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        B, ext, D = v.shape
        if D != 1 << (logn + logbeta):
            raise XfgStarkError(9, "debug_merkle_fri: vals [B,ext,2^(logn+logbeta)]")
        if not 0 < fold < 1 << 32:
            raise XfgStarkError(9, "debug_merkle_fri: fold is 2, 4, 8 or 16")
        nodes = np.zeros((B, 2 * (D // fold), 8), dtype="<u4")
        st = _lib.xfg_debug_merkle_fri_f(self._ctx, B, ext, logn, logbeta, 1 if coset_major else 0, fold,
                                         v.ctypes.data_as(_u64p), nodes.ctypes.data_as(_u8p))
        if st:
            raise self._err(st)
        return nodes

    def debug_interpolate(self, evals, n, offset7=False):
        import numpy as np
        e = np.ascontiguousarray(np.asarray(evals, dtype=np.uint64)).reshape(-1, n)
        out = np.zeros_like(e)
        st = _lib.xfg_debug_interpolate(self._ctx, e.ctypes.data_as(_u64p), e.shape[0], n, 1 if offset7 else 0,
                                        out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out

    def debug_interpolate_keep(self, evals, n, keep, offset7=False):
        """the truncated inverse transform of the composition polynomial and the FRI remainder: the first
        `keep` coefficients of every polynomial, `keep` words apart. -> (coefficients [npoly][keep], the 8
        guard words behind them, which a correct run leaves at 0xFF..FF)"""
        import numpy as np
        e = np.ascontiguousarray(np.asarray(evals, dtype=np.uint64)).reshape(-1, n)
        keep = int(keep)
        if not 0 <= keep < 1 << 64:
            raise XfgStarkError(9, "debug_interpolate_keep: keep is 1..n")
        out = np.zeros(e.shape[0] * min(keep, n) + 8, dtype=np.uint64)
        st = _lib.xfg_debug_interpolate_keep(self._ctx, e.ctypes.data_as(_u64p), e.shape[0], n, keep,
                                             1 if offset7 else 0, out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out[:-8].reshape(e.shape[0], keep), out[-8:]

    def debug_interpolate_skip(self, evals, n, skip, offset7=False):
        """debug_interpolate with a flag per polynomial (see debug_lde_skip)"""
        import numpy as np
        e = np.ascontiguousarray(np.asarray(evals, dtype=np.uint64)).reshape(-1, n)
        f = np.ascontiguousarray(np.asarray(skip, dtype=np.uint8))
        if f.shape != (e.shape[0],):
            raise XfgStarkError(9, "debug_interpolate_skip: one flag per polynomial")
        out = np.zeros_like(e)
        st = _lib.xfg_debug_interpolate_skip(self._ctx, e.ctypes.data_as(_u64p), e.shape[0], n, 1 if offset7 else 0,
                                             f.ctypes.data_as(_u8p), out.ctypes.data_as(_u64p))
        if st:
            raise self._err(st)
        return out
