"""What the wrappers do to their arguments on the way into the library, each written once."""
import ctypes as C
import mmap

from ._abi import XfgStarkError, _AirConsts, _u8p, _u64p


def np():
    """numpy, imported when the first array is marshalled: importing the package imports neither it nor torch"""
    import numpy
    return numpy


def array(x, dtype="uint64", shape=None, what=None):
    """x as a C-contiguous array of `dtype`; given `shape`, any other shape raises XfgStarkError(9, what)"""
    a = np().ascontiguousarray(x, dtype=dtype)
    if shape is not None and a.shape != tuple(shape):
        raise XfgStarkError(9, what)
    return a


def trace_array(x):
    """a batch of host traces [count][7][n] -> (array, layout). A uint64 ndarray that is not C-contiguous and
    whose strides are non-negative multiples of 8 bytes goes to the library as it lies, without a copy: layout =
    its (trace, column, row) strides in 8-byte words. Anything else is copied into a C-contiguous array, layout
    None. A negative stride raises XfgStarkError(9): the library's strides are unsigned"""
    n_ = np()
    if isinstance(x, n_.ndarray) and x.dtype == n_.uint64 and x.ndim == 3:
        if any(s < 0 for s in x.strides):
            raise XfgStarkError(9, "traces: a view with a negative stride is not supported")
        if not x.flags.c_contiguous and x.flags.aligned and all(s % 8 == 0 for s in x.strides):
            return x, tuple(s // 8 for s in x.strides)
    return array(x), None


def zeros(shape, dtype="uint64"):
    return np().zeros(shape, dtype=dtype)


def words(data):
    """bytes -> their little-endian u32 words, as the library takes BLAKE3 seeds"""
    return np().frombuffer(data, dtype="<u4").copy()


def ptr(a, kind=_u64p):
    """the data pointer of an array (u64 words unless `kind` says otherwise)"""
    return a.ctypes.data_as(kind)


def bytes_ptr(b):
    return C.cast(C.c_char_p(b), _u8p)


def air_struct(air):
    """one xfg_air_consts from (pub_inputs[12], nullifier, commitment)"""
    pub, nullifier, commitment = air
    return _AirConsts((C.c_uint64 * 12)(*pub), nullifier, commitment)


def air_array(airs):
    """xfg_air_consts[] from an iterable of (pub_inputs[12], nullifier, commitment) tuples, as one numpy array
    (per-item ctypes structs dominated large batches) -> (the array, which owns the memory; its pointer)"""
    rows = [list(a[0]) + [a[1], a[2]] for a in airs]
    words14 = array(rows).reshape(len(rows), 14)
    return words14, ptr(words14, C.POINTER(_AirConsts))


def out_slots(k, cap, base, header=None):
    """the output arguments of a batch of k proofs: slot i is the `cap` bytes at base + i cap; the lengths
    (capacity in, length out), at address `header` where a caller's record keeps them; the statuses"""
    outs = (_u8p * k)(*[C.cast(base + i * cap, _u8p) for i in range(k)])
    lens = (C.c_size_t * k).from_address(header) if header is not None else (C.c_size_t * k)()
    lens[:] = [cap] * k
    return outs, lens, (C.c_int * k)()


def new_buffer(size, touch=False):
    """a host output buffer of at least one byte (a mapping of length 0 raises ValueError before the C library
    could report the invalid request: empty batch, trace length with no size bound). It is a private
    anonymous mapping: mmap.mmap(-1, n) is MAP_SHARED by default, shmem pages that are slower to fault and
    to write than the private pages malloc hands out; and create_string_buffer zero-fills the whole bound
    (64 x 0.7 MB at n = 2^16) on the calling thread, 11 ms of page faults per batch during which the next
    batch could not be submitted. The pages are faulted in by the workers' proof copies instead, once, or
    here with `touch` (setup)"""
    size = max(size, 1)
    b = (C.c_char * size).from_buffer(mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS))
    if touch:
        C.memset(b, 0, size)
    return b
