"""The C ABI of libxfgstark.so as ctypes sees it: the library, the structs of include/xfg_stark.h and
one table of prototypes, a row per C function. tests/test_abi.py holds the table against the header, so a
new C entry is one prototype there and one row here."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
RECORDS_ON_DEVICE = 1  # XFG_RECORDS_ON_DEVICE of xfg_prove_records
RECORD_BYTES = 128  # sizeof(xfg_burn_record)


class XfgStarkError(Exception):
    """XfgStarkError::CryptoError(String) (reference src/lib.rs:66-110); `.status` is the C-ABI code."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status
        self.kind = STATUS.get(status, str(status))


class _Options(C.Structure):
    _fields_ = [("num_queries", C.c_uint32), ("blowup_factor", C.c_uint32), ("grinding_factor", C.c_uint32),
                ("field_extension", C.c_uint32), ("fri_folding_factor", C.c_uint32),
                ("fri_remainder_max_degree", C.c_uint32)]


ACCEPT_OPTION_SET, ACCEPT_MIN_CONJECTURED_SECURITY = 0, 1  # XFG_ACCEPT_* kinds of xfg_acceptable


class _Acceptable(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("min_security", C.c_uint32), ("options", C.POINTER(_Options)),
                ("num_options", C.c_uint32)]


class _BurnInputs(C.Structure):
    _fields_ = [("burn_amount", C.c_uint64), ("mint_amount", C.c_uint64), ("tx_prefix_hash", C.c_uint8 * 32),
                ("recipient_address", C.c_char_p), ("recipient_len", C.c_size_t), ("secret", C.c_char_p),
                ("secret_len", C.c_size_t), ("network_id", C.c_uint32), ("target_chain_id", C.c_uint32),
                ("commitment_version", C.c_uint32)]


class _BurnRecord(C.Structure):
    _fields_ = [("burn_amount", C.c_uint64), ("mint_amount", C.c_uint64), ("tx_prefix_hash", C.c_uint8 * 32),
                ("recipient", C.c_uint8 * 20), ("secret", C.c_uint8 * 32), ("network_id", C.c_uint32),
                ("target_chain_id", C.c_uint32), ("commitment_version", C.c_uint32), ("reserved", C.c_uint8 * 16)]


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


class _TraceLayout(C.Structure):
    _fields_ = [("trace_stride", C.c_uint64), ("col_stride", C.c_uint64), ("row_stride", C.c_uint64)]


class _ProbePattern(C.Structure):
    _fields_ = [("kind", C.c_uint32 * 7), ("reserved", C.c_uint32), ("row", C.c_uint64 * 7), ("proof", C.c_uint64)]


_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)

# shorthands of the table below: scalars, then pointers
_ctx, _int, _u32, _u64, _sz, _str = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_char_p
_intp, _szp, _f64p, _bufs = C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_double), C.POINTER(_u8p)
_opts, _burn, _airs, _faults = C.POINTER(_Options), C.POINTER(_BurnInputs), C.POINTER(_AirConsts), C.POINTER(_TraceFault)
# the submit entries take their synchronous form's arguments and a ticket
_PROVE_BATCH = [_ctx, _u32, _burn, _u64, _opts, _bufs, _szp, _intp]
_TRACE_BATCH = [_ctx, _u32, C.c_void_p, _u32, _u64, _airs, _opts, _u32, _bufs, _szp, _intp, _faults]
_layout = C.POINTER(_TraceLayout)
_accept = C.POINTER(_Acceptable)
_TRACE_BATCH_STRIDED = [_ctx, _u32, C.c_void_p, _u64, _layout, _airs, _opts, _u32, _bufs, _szp, _intp, _faults]
_RECORDS = [_ctx, _u32, C.c_void_p, _u64, _opts, _u32, _bufs, _szp, _intp]  # records: host or device memory
_FRI = [_ctx, _u32, _u32, _u32, _u32, _int]  # count, ext, logn, logbeta, coset_major
_OOD_TAIL = [_u64p, _u64p, _u64p, _u32p, _u64p, _u64, _u64p, _u64p, _u64p, _u32p, _u64p, _intp]  # from hcoef on

# (name, restype, argtypes) of every function the header declares, in the header's order
TABLE = [
    ("xfg_ctx_create", C.c_void_p, [_int]),
    ("xfg_ctx_destroy", None, [_ctx]),
    ("xfg_default_options", _int, [_opts]),
    ("xfg_last_error", _int, [_ctx, _str, _sz]),
    ("xfg_proof_size_bound", _sz, [_u64, _opts]),
    ("xfg_prove_burn_mint", _int, [_ctx, _burn, _u64, _opts, _u8p, _szp]),
    ("xfg_prove_trace", _int, [_ctx, _u64p, _u32, _u64, _airs, _opts, _u8p, _szp]),
    ("xfg_prove_batch", _int, _PROVE_BATCH),
    ("xfg_prove_batch_submit", _int, _PROVE_BATCH + [_u64p]),
    ("xfg_batch_wait", _int, [_ctx, _u64]),
    ("xfg_check_traces", _int, [_ctx, _u32, C.c_void_p, _u64, _airs, _u32, _faults]),
    ("xfg_prove_trace_batch", _int, _TRACE_BATCH),
    ("xfg_prove_trace_batch_submit", _int, _TRACE_BATCH + [_u64p]),
    ("xfg_check_traces_strided", _int, [_ctx, _u32, C.c_void_p, _u64, _layout, _airs, _u32, _faults]),
    ("xfg_prove_trace_batch_strided", _int, _TRACE_BATCH_STRIDED),
    ("xfg_prove_trace_batch_strided_submit", _int, _TRACE_BATCH_STRIDED + [_u64p]),
    ("xfg_prove_records", _int, _RECORDS),
    ("xfg_prove_records_submit", _int, _RECORDS + [_u64p]),
    ("xfg_air_consts_from_records", _int, [_ctx, _u32, C.c_void_p, _u32, _airs, _intp]),
    ("xfg_prepare", _int, [_ctx, _u32, _u64, _opts]),
    ("xfg_burn_air_consts", _int, [_burn, _airs]),
    ("xfg_proof_parse", _int, [_u8p, _sz, C.POINTER(_ProofInfo), _str, _sz]),
    ("xfg_verify", _int, [_u8p, _sz, _airs, _opts, _str, _sz]),
    ("xfg_verify_batch", _int, [_u32, _bufs, _szp, _airs, _opts, _intp, _u32]),
    ("xfg_verify_batch_gpu", _int, [_ctx, _u32, _bufs, _szp, _airs, _opts, _intp]),
    ("xfg_security_level", _int, [_u64, _opts, _u32p]),
    ("xfg_verify_acceptable", _int, [_u8p, _sz, _airs, _accept, _str, _sz]),
    ("xfg_verify_batch_acceptable", _int, [_u32, _bufs, _szp, _airs, _accept, _intp, _u32]),
    ("xfg_verify_batch_gpu_acceptable", _int, [_ctx, _u32, _bufs, _szp, _airs, _accept, _intp]),
    ("xfg_selftest_blake3", _int, [_u8p, _sz, _u8p]),
    ("xfg_selftest_field", _int, [_u64, _u64, _u64p]),
    ("xfg_set_timing", _int, [_ctx, _int]),
    ("xfg_stage_times", _int, [_ctx, _f64p, C.POINTER(C.c_char_p), _int]),
    ("xfg_bench_lde", _int, [_ctx, _u32, _u64, _u32, _u32, _f64p]),
    ("xfg_lde_probe", _int, [_ctx, _int, _f64p, _u64p, _u64p]),
    ("xfg_debug_lde", _int, [_ctx, _u64p, _u32, _u64, _u32, _u64p]),
    ("xfg_debug_interpolate", _int, [_ctx, _u64p, _u32, _u64, _int, _u64p]),
    ("xfg_debug_const_columns", _int, [_ctx, _u64p, _u32, _u32, _u64, _u8p]),
    ("xfg_debug_col_classes", _int, [_ctx, _u64p, _u32, _u64, _u8p, _u64p]),
    ("xfg_debug_trace_probe", _int, [_ctx, _u32, _u64, _airs, _u32, C.POINTER(_ProbePattern), _u8p, _u64p, _u64p]),
    ("xfg_debug_trace_ingest", _int, [_ctx, _u32, _u64, _u64p, _u64, _layout, _airs, _int, _u8p, _u64p, _faults, _u64p]),
    ("xfg_debug_lde_skip", _int, [_ctx, _u64p, _u32, _u64, _u32, _u8p, _u64p]),
    ("xfg_debug_interpolate_skip", _int, [_ctx, _u64p, _u32, _u64, _int, _u8p, _u64p]),
    ("xfg_debug_interpolate_keep", _int, [_ctx, _u64p, _u32, _u64, _u64, _int, _u64p]),
    ("xfg_debug_field", _int, [_ctx, _u32, _u64, _u64p, _u64p, _u64p]),
    ("xfg_debug_ood_deep", _int, [_ctx, _u32, _u64, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]),
    ("xfg_debug_ood_deep_e", _int, [_ctx, _u32, _u64, _u32, _u64p] + _OOD_TAIL),
    ("xfg_debug_ood_deep_const", _int, [_ctx, _u32, _u64, _u32, _u64p, _u8p, _u64p] + _OOD_TAIL),
    ("xfg_debug_constraint_eval", _int, [_ctx, _u32, _u64, _u32, _u32, _u64p, _airs, _u64p, _u64p]),
    ("xfg_debug_fri_fold", _int, _FRI + [_u64p, _u64p, _u64p]),
    ("xfg_debug_fri_fold_f", _int, _FRI + [_u32, _u64p, _u64p, _u64p]),
    ("xfg_debug_coin_draws", _int, [_ctx, _u32p, _u64, _u32, _u32, _u64p, _u64p, _u64p, _u64p, _intp]),
    ("xfg_debug_merkle_lde", _int, [_ctx, _u32, _u32, _u64, _u32, _u64p, _u64p, _u64, _u8p, _u8p]),
    ("xfg_debug_merkle_lde_const", _int, [_ctx, _u32, _u32, _u64, _u32, _u64p, _u8p, _u64p, _u64p, _u64, _u8p, _u8p]),
    ("xfg_debug_poison_lde", _int, [_ctx, _int]),
    ("xfg_debug_merkle_fri", _int, _FRI + [_u64p, _u8p]),
    ("xfg_debug_merkle_fri_f", _int, _FRI + [_u32, _u64p, _u8p]),
    ("xfg_debug_grind", _int, [_ctx, _u32, _u32p, _u32, _u64, _u64, _u32, _u32, _u64p]),
    ("xfg_grind_probe", _int, [_ctx, _u32p, _u64p, _u64p]),
    ("xfg_debug_keccak256", _int, [_ctx, _u32, _u8p, _u32p, _u8p]),
    ("xfg_debug_verify_batch_gpu", _int, [_ctx, _u32, _bufs, _szp, _airs, _opts, _intp, _u64p, _str, _sz]),
    ("xfg_debug_verify_batch_gpu_acceptable", _int, [_ctx, _u32, _bufs, _szp, _airs, _accept, _intp, _u64p, _str, _sz]),
]


def bind(lib, table=TABLE):
    """set restype and argtypes of every row's function on `lib`; -> the names it does not export. An older
    build loaded through XFG_LIB lacks the newer hooks: it still imports, and calling one of them raises
    AttributeError from ctypes"""
    missing = []
    for name, restype, argtypes in table:
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)
        else:
            fn.restype, fn.argtypes = restype, argtypes
    return missing


MISSING = bind(_lib)


def exported_symbols():
    return dir(_lib)
