"""xfgstark -- Python mirror of the reference prover API over the MI355X C ABI (libxfgstark.so).

Mirrors reference src/burn_mint_prover.rs (XfgBurnMintProver::new / with_options /
prove_burn_mint / get_proof_size / security_parameter / proof_options) and the Winterfell
ProofOptions / StarkProof surface it returns. All proving runs in libxfgstark.so (HIP kernels
for gfx950); there is no CPU fallback: if the library is missing this module fails to import, and
without a GPU the prover constructor raises.

_abi: the library, its structs and the one table of prototypes; _marshal: arguments on their way in;
_api: the product API; _hooks: the kernel-level test hooks (XfgBurnMintProver.debug_*); package: data packages.
"""
import ctypes as C  # noqa: F401  (tests and scripts build their own arguments with xfgstark.C)

from ._abi import (HEADER_PATH, LIB_PATH, RECORD_BYTES, RECORDS_ON_DEVICE, STATUS, TRACE_ON_DEVICE,  # noqa: F401
                   TRACE_VALIDATE, XfgStarkError, _Acceptable, _BurnRecord, _lib, _Options, _TraceFault, _TraceLayout,
                   _u8p, _u64p, exported_symbols)
from ._api import (AcceptableOptions, FieldExtension, PendingBatch, ProofOptions, StarkProof, TraceFault,  # noqa: F401
                   XfgBurnMintProver, XfgBurnMintVerifier, air_consts, air_consts_from_records, blake3, burn_inputs,
                   pack_records, record_size, unpack_records)
