"""The named layouts of caller-supplied traces that the CPU and the GPU tests of the strided entries share, and
the batches they run on.

TEST INFRASTRUCTURE ONLY. A layout says where cell (trace i, column c, step s) lies in one flat buffer of
8-byte words: offset + i * trace_stride + c * col_stride + s * row_stride (xfg_trace_layout).

    dense        {7n, n, 1}              the hook; the entries copy it as they do without a layout (one raw test)
    rows7        {7n, 1, 7}              row-major; the tile form of the ingest kernels, pitch 7
    rows8        {8n, 1, 8}              rows padded to 8 words; the 8th word of every row is 2^64 - 1
    rows12+3     {12n, 1, 12}, offset 3  seven columns of a wider table; the base is only 8-byte aligned
    rows24       {24n, 1, 24}            a pitch past the tile form: the generic form
    cols_padded  {7(n+8), n+8, 1}        padded columns: the generic form, coalesced
    batch_inner  {1, n count, count}     the traces interleaved, the trace index innermost
    broadcast    {0, n, 1}               every trace is trace 0

Every word of a buffer that is no cell holds 2^64 - 1, which is no field element: a pad word that surfaces
anywhere shows. The buffers of rows7 and rows8 end exactly at the extent: no pad follows the last row.
"""
import functools

import numpy as np
from numpy.lib.stride_tricks import as_strided

import plain_ref as R
import trace_check_ref as T

P = R.P
FILL = np.uint64((1 << 64) - 1)
NAMES = ["dense", "rows7", "rows8", "rows12+3", "rows24", "cols_padded", "batch_inner", "broadcast"]
TILED = ("rows7", "rows8", "rows12+3")  # the layouts the ingest kernels take in their tile form


def strides_of(name, count, n):
    """(trace, column, row) strides in words, and the words in front of cell (0, 0, 0)"""
    return {"dense": ((7 * n, n, 1), 0), "rows7": ((7 * n, 1, 7), 0), "rows8": ((8 * n, 1, 8), 0),
            "rows12+3": ((12 * n, 1, 12), 3), "rows24": ((24 * n, 1, 24), 0),
            "cols_padded": ((7 * (n + 8), n + 8, 1), 0), "batch_inner": ((1, n * count, count), 0),
            "broadcast": ((0, n, 1), 0)}[name]


def extent(layout, count, n):
    return (count - 1) * layout[0] + 6 * layout[1] + (n - 1) * layout[2] + 1


class Layout:
    """`dense` [count][7][n] uint64 laid out as `name` says: flat (the buffer, offset + extent words), layout,
    offset, view (the strided [count][7][n] view of flat). With broadcast every trace is dense[0]"""

    def __init__(self, name, dense):
        dense = np.ascontiguousarray(dense, dtype=np.uint64)
        self.name = name
        self.count, _, self.n = dense.shape
        self.layout, self.offset = strides_of(name, self.count, self.n)
        self.flat = np.full(self.offset + extent(self.layout, self.count, self.n), FILL, dtype=np.uint64)
        self.view = as_strided(self.flat[self.offset:], shape=dense.shape, strides=tuple(8 * s for s in self.layout))
        if name == "broadcast":
            self.view[0] = dense[0]
        else:
            self.view[...] = dense

    def materialise(self):
        """the dense array the layout names"""
        return np.ascontiguousarray(self.view)

    def tensor(self, device="cuda:0"):
        """the same view of a device copy of the buffer, as an int64 tensor (the bits are kept)"""
        import torch
        flat = torch.from_numpy(self.flat.view(np.int64)).to(device)
        return torch.as_strided(flat, (self.count, 7, self.n), self.layout, self.offset)


def canonical(traces):
    t = np.asarray(traces, dtype=np.uint64)
    return np.where(t >= np.uint64(P), t - np.uint64(P), t)


def classify(traces):
    """the numpy rule for the column classes of a unit [count][7][n] (on canonical cells): 1 constant = all rows
    equal; 2 shared = equal to trace 0's column, not constant, not trace 0; else 0 live -> (classes, element 0)"""
    t = canonical(traces)
    const = (t == t[:, :, :1]).all(axis=2)
    same = (t == t[:1]).all(axis=2)
    same[0] = False
    return np.where(const, 1, np.where(same, 2, 0)).astype(np.uint8), t[:, :, 0].copy()


@functools.lru_cache(maxsize=None)
def class_batch(n):
    """the batch the class tests run on, (traces [5][7][n], airs): trace 0 a valid burn trace; 1 the same with
    column 4 replaced by random cells; 2 trace 0 itself; 3 a random trace; 4 wide_consts"""
    t0, air0 = T.valid_trace(n, 11)
    rng = np.random.default_rng(1000 + n)
    t1 = t0.copy()
    t1[4] = rng.integers(0, P, size=n, dtype=np.uint64)
    t3, air3 = R.make_trace("random", n, 77 + n)
    t4, air4 = R.make_trace("wide_consts", n, 78 + n)
    traces = np.stack([t0, t1, t0.copy(), np.array(t3, dtype=np.uint64), np.array(t4, dtype=np.uint64)])
    return traces, [air0, air0, air0, air3, air4]


@functools.lru_cache(maxsize=None)
def check_batch(n):
    """every planted case of trace_check_ref at n and three random traces: (traces, airs, names, expected faults)"""
    planted = T.planted_cases(n)
    cases = [(tr, air) for _, tr, air, _ in planted] + T.random_cases(n, [n + 1, n + 2, n + 3])
    names = [c[0] for c in planted] + ["random"] * 3
    return (np.stack([tr for tr, _ in cases]), [air for _, air in cases], names,
            [T.first_fault(tr, air) for tr, air in cases])
