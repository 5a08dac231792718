"""Kernel-level test hooks (the xfg_debug_* entries): host arrays in, one launch set of the prover's own
kernels, host arrays out. The layouts, and the 0xFF bytes the entries put where nothing may be read or
left, are described in include/xfg_stark.h."""
import ctypes as C

from ._abi import XfgStarkError, _lib, _ProbePattern, _TraceFault, _TraceLayout, _u8p, _u32p
from ._marshal import air_array, array, ptr, words, zeros


class KernelHooks:
    """the debug_* methods of XfgBurnMintProver, which supplies _call (the context goes first, a status raises)"""

    def debug_lde(self, coef, n, blowup):
        c = array(coef).reshape(-1, n)
        out = zeros((c.shape[0], n * blowup))
        self._call(_lib.xfg_debug_lde, ptr(c), c.shape[0], n, blowup, ptr(out))
        return out

    def debug_lde_skip(self, coef, n, blowup, skip):
        """debug_lde with a flag per polynomial: flagged ones (vouched constant by the caller) take no
        transform and are filled in, as the prover does for the constant columns it detects"""
        c = array(coef).reshape(-1, n)
        f = array(skip, "uint8", (c.shape[0],), "debug_lde_skip: one flag per polynomial")
        out = zeros((c.shape[0], n * blowup))
        self._call(_lib.xfg_debug_lde_skip, ptr(c), c.shape[0], n, blowup, ptr(f, _u8p), ptr(out))
        return out

    def debug_keccak256(self, messages):
        """Keccak-256 of single-block messages (each at most 135 bytes) by the record kernel's permutation
        (xfg_debug_keccak256) -> list of 32-byte digests"""
        k = len(messages)
        msgs, lens = zeros((max(k, 1), 136), "uint8"), zeros((max(k, 1),), "uint32")
        for i, m in enumerate(messages):
            if len(m) > 135:
                raise XfgStarkError(9, "debug_keccak256: a message is one block, at most 135 bytes")
            msgs[i, :len(m)] = list(m)
            msgs[i, len(m):] = 0xA5  # never read
            lens[i] = len(m)
        out = zeros((max(k, 1), 32), "uint8")
        self._call(_lib.xfg_debug_keccak256, k, ptr(msgs, _u8p), ptr(lens, _u32p), ptr(out, _u8p))
        return [out[i].tobytes() for i in range(k)]

    def debug_const_columns(self, trace):
        """the prover's constant-column detection: trace [B,width,n] -> flags [B,width] (1 = one value in every row)"""
        tr = array(trace)
        B, width, n = tr.shape
        out = zeros((B, width), "uint8")
        self._call(_lib.xfg_debug_const_columns, ptr(tr), B, width, n, ptr(out, _u8p))
        return out

    def debug_col_classes(self, trace, values=False):
        """the unit's column detection as the prover runs it (xfg_debug_col_classes): trace [B,7,n] -> classes
        [B,7], 0 live, 1 constant, 2 the same as trace 0's column; values=True: also element 0 of every column"""
        tr = array(trace)
        B, width, n = tr.shape
        if width != 7:
            raise XfgStarkError(9, "debug_col_classes: trace [B,7,n]")
        out, vals = zeros((B, 7), "uint8"), zeros((B, 7))
        self._call(_lib.xfg_debug_col_classes, ptr(tr), B, n, ptr(out, _u8p), ptr(vals))
        return (out, vals) if values else out

    def debug_trace_probe(self, airs, n, generator=0, pattern=None):
        """the front end of a unit of generated traces (xfg_debug_trace_probe): airs = B air_consts() tuples;
        generator 0 the burn AIR's rows, 1 the synthetic rows of pattern = (kind[7], row[7], proof) ->
        (classes [B,7], values [B,7], trace buffer [B,7,n] as left: unwritten planes are 0xFF bytes)"""
        B = len(airs)
        keep, air_p = air_array(airs)
        pat = None
        if pattern is not None:
            kind, row, proof = pattern
            pat = C.byref(_ProbePattern((C.c_uint32 * 7)(*kind), 0, (C.c_uint64 * 7)(*row), proof))
        cls, vals, tr = zeros((B, 7), "uint8"), zeros((B, 7)), zeros((B, 7, n))
        self._call(_lib.xfg_debug_trace_probe, B, n, air_p, generator, pat, ptr(cls, _u8p), ptr(vals), ptr(tr))
        return cls, vals, tr

    def debug_trace_ingest(self, buf, layout, count, n, airs, validate=False):
        """the front end of a unit of device traces in a strided layout (xfg_debug_trace_ingest): buf = a flat
        uint64 array, uploaded as it is; layout = (trace, column, row) strides in words, None for dense; airs =
        count air_consts() tuples -> (classes [count,7], values [count,7], faults: list of the xfg_trace_fault
        fields (kind, index, column, step, expected, found) or None, trace buffer [count,7,n] as left: unwritten
        planes are 0xFF bytes)"""
        b = array(buf).reshape(-1)
        keep, air_p = air_array(airs)
        at = None if layout is None else C.byref(_TraceLayout(*layout))
        cls, vals, tr = zeros((count, 7), "uint8"), zeros((count, 7)), zeros((count, 7, n))
        faults = (_TraceFault * max(count, 1))()
        self._call(_lib.xfg_debug_trace_ingest, count, n, ptr(b), b.size, at, air_p, 1 if validate else 0,
                   ptr(cls, _u8p), ptr(vals), faults, ptr(tr))
        fields = [name for name, _ in _TraceFault._fields_]
        return cls, vals, [tuple(getattr(f, k) for k in fields) if f.kind else None for f in faults[:count]], tr

    def debug_ood_deep_const(self, coef, flags, vals, hcoef, zpts, coeffs):
        """debug_ood_deep_e without coins on coefficients behind a column descriptor (xfg_debug_ood_deep_const):
        flags [B,7] 1 = constant with value vals [B,7], 2 = the coefficients of instance 0's column; the
        flagged planes of coef are replaced by 0xFF bytes on the device -> (ood [B,15,ext], deep [B,ext,n])"""
        c, hc, zp, co, v = array(coef), array(hcoef), array(zpts), array(coeffs), array(vals)
        f = array(flags, "uint8")
        B, _, n = c.shape
        ext = hc.shape[1]
        if (c.shape[1] != 7 or hc.shape != (B, ext, n) or zp.shape != (B, 2, ext) or co.shape != (B, 8, ext)
                or f.shape != (B, 7) or v.shape != (B, 7)):
            raise XfgStarkError(9, "debug_ood_deep_const: coef [B,7,n], flags and vals [B,7], hcoef [B,ext,n], "
                                   "zpts [B,2,ext], coeffs [B,8,ext]")
        ood, deep = zeros((B, 15, ext)), zeros((B, ext, n))
        self._call(_lib.xfg_debug_ood_deep_const, B, n, ext, ptr(c), ptr(f, _u8p), ptr(v), ptr(hc), ptr(zp), ptr(co),
                   None, None, 0, ptr(ood), ptr(deep), None, None, None, None)
        return ood, deep

    def debug_ood_deep(self, coef, hcoef, zpts, coeffs):
        """OOD + DEEP kernels: coef [B,7,n], hcoef [B,n], zpts [B,2], coeffs [B,8] -> (ood [B,15], deep [B,n])"""
        c, hc, zp, co = array(coef), array(hcoef), array(zpts), array(coeffs)
        B, _, n = c.shape
        ood, deep = zeros((B, 15)), zeros((B, n))
        self._call(_lib.xfg_debug_ood_deep, B, n, ptr(c), ptr(hc), ptr(zp), ptr(co), ptr(ood), ptr(deep))
        return ood, deep

    def debug_ood_deep_e(self, coef, hcoef, zpts, coeffs=None, coins=None, ginv=0):
        """OOD + DEEP kernels in the field of degree ext (xfg_debug_ood_deep_e): coef [B,7,n], hcoef [B,ext,n],
        zpts [B,2,ext]. Without `coins`: coeffs [B,8,ext] -> (ood [B,15,ext], deep [B,ext,n]). With coins = B x
        (32-byte seed, counter) and ginv = 1 / g, the prover's launches with the DEEP transcript step ->
        (ood, deep, dp [B,14,2] = a_0..a_6, gamma, z, zg, 1/z, 1/zg, c1, c2, coins afterwards, fail [B]).
        Shapes are passed on as they are: the library refuses what it does not support"""
        c, hc, zp = array(coef), array(hcoef), array(zpts)
        B, _, n = c.shape
        ext = hc.shape[1]
        if c.shape[1] != 7 or hc.shape != (B, ext, n) or zp.shape != (B, 2, ext):
            raise XfgStarkError(9, "debug_ood_deep_e: coef [B,7,n], hcoef [B,ext,n], zpts [B,2,ext]")
        ood, deep = zeros((B, 15, ext)), zeros((B, ext, n))
        if coins is None:
            co = array(coeffs, shape=(B, 8, ext), what="debug_ood_deep_e: coeffs [B,8,ext]")
            self._call(_lib.xfg_debug_ood_deep_e, B, n, ext, ptr(c), ptr(hc), ptr(zp), ptr(co), None, None, 0,
                       ptr(ood), ptr(deep), None, None, None, None)
            return ood, deep
        if len(coins) != B or any(len(bytes(sd)) != 32 for sd, _ in coins):
            raise XfgStarkError(9, "debug_ood_deep_e: coins are B x (32-byte seed, counter)")
        seeds, ctrs = words(b"".join(bytes(sd) for sd, _ in coins)), array([ctr for _, ctr in coins])
        dp, seeds_out, ctrs_out = zeros((B, 14, 2)), zeros(B * 8, "<u4"), zeros(B)
        fail = (C.c_int * max(B, 1))()
        self._call(_lib.xfg_debug_ood_deep_e, B, n, ext, ptr(c), ptr(hc), ptr(zp), None, ptr(seeds, _u32p), ptr(ctrs),
                   ginv, ptr(ood), ptr(deep), ptr(dp), ptr(seeds_out, _u32p), ptr(ctrs_out), fail)
        after = [(seeds_out[8 * b:8 * b + 8].tobytes(), int(ctrs_out[b])) for b in range(B)]
        return ood, deep, dp, after, [fail[b] for b in range(B)]

    def debug_constraint_eval(self, trace, airs, coeffs, blowup):
        """constraint evaluation kernel behind interpolation + LDE + the divisor table, as the prover
        runs them: trace [B,7,n], airs = B x (pub[12], nullifier, commitment), coeffs [B,15,ext]
        -> ce [B,ext,2n] in natural CE-domain order"""
        tr, co = array(trace), array(coeffs)
        B, width, n = tr.shape
        if width != 7 or co.ndim != 3 or co.shape[:2] != (B, 15) or len(airs) != B:
            raise XfgStarkError(9, "debug_constraint_eval: trace [B,7,n], airs [B], coeffs [B,15,ext]")
        ext = co.shape[2]
        keep, air_p = air_array(airs)
        ce = zeros((B, ext, 2 * n))
        self._call(_lib.xfg_debug_constraint_eval, B, n, blowup, ext, ptr(tr), air_p, ptr(co), ptr(ce))
        return ce

    def debug_fri_fold(self, vals, alpha, logn, logbeta, coset_major, fold=8):
        """FRI fold kernel (folding factor `fold` = 2, 4, 8 or 16): vals [B,ext,D] with D = 2^(logn + logbeta)
        >= 2 fold, natural order or coset-major (natural index K at (K mod beta) n + K // beta), alpha [B,ext]
        -> [B,ext,D/fold] (xfg_debug_fri_fold_f, which refuses any other fold or a smaller D)"""
        v, al = array(vals), array(alpha)
        B, ext, D = v.shape
        if D != 1 << (logn + logbeta) or al.shape != (B, ext):
            raise XfgStarkError(9, "debug_fri_fold: vals [B,ext,2^(logn+logbeta)], alpha [B,ext]")
        if not 0 < fold < 1 << 32:
            raise XfgStarkError(9, "debug_fri_fold: fold is 2, 4, 8 or 16")
        out = zeros((B, ext, D // fold))
        self._call(_lib.xfg_debug_fri_fold_f, B, ext, logn, logbeta, 1 if coset_major else 0, fold, ptr(v), ptr(al),
                   ptr(out))
        return out

    # ops from mul2_pair on read a, b as pairs (a[2i], a[2i+1]) and write both words of the result
    FIELD_OPS = {"mul": 0, "add": 1, "sub": 2, "canon": 3, "pow2": 4, "fold": 5, "sub_weak": 6, "add_w": 7, "mul2": 8,
                 "mul2_pair": 9, "e2_mul": 10, "e2_mulb": 11, "e2_inv": 12}

    def debug_field(self, op, a, b):
        """device Goldilocks primitive `op` (FIELD_OPS) applied elementwise to u64 arrays a, b"""
        x, y = array(a), array(b)
        out = zeros(x.shape)
        self._call(_lib.xfg_debug_field, self.FIELD_OPS[op], x.size, ptr(x), ptr(y), ptr(out))
        return out

    def debug_coin_draws(self, seed, counter, k, ext=1, reject=(0, 0, 0, 0)):
        """device transcript draws (xfg_debug_coin_draws): seed = 32 bytes, k <= 64 draws of E by one
        wave and one at a time, with counters 1..256 force-rejected where `reject` (4 x u64 bits) is
        set. Returns (wave [k][2], sequential [k][2], counters (wave, seq), ok (wave, seq))"""
        w = (C.c_uint32 * 8)(*words(bytes(seed)).tolist())
        rej = array(reject)
        ow, osq, ctr = zeros((k, 2)), zeros((k, 2)), zeros(2)
        ok = (C.c_int * 2)()
        self._call(_lib.xfg_debug_coin_draws, w, counter, k, ext, ptr(rej), ptr(ow), ptr(osq), ptr(ctr), ok)
        return ow, osq, (int(ctr[0]), int(ctr[1])), (ok[0], ok[1])

    def debug_grind(self, seeds, grind, first_nonce=1, max_nonce=0, chunk_log=0, blocks=0):
        """the prover's proof-of-work search alone (xfg_debug_grind): seeds = 32-byte strings; for each the
        smallest nonce in [first_nonce, max_nonce] whose BLAKE3(seed || nonce_le8) has >= grind trailing
        zero bits in its first 8 LE bytes, 0 where there is none. max_nonce 0: the prover's bound
        2^(grind + 8); chunk_log / blocks 0: the planner's geometry, else forced (6..16, 1..4096)"""
        if any(len(bytes(sd)) != 32 for sd in seeds):
            raise XfgStarkError(9, "debug_grind: seeds are 32 bytes each")
        w = words(b"".join(bytes(sd) for sd in seeds))
        out = zeros(len(seeds))
        self._call(_lib.xfg_debug_grind, len(seeds), ptr(w, _u32p), grind, first_nonce, max_nonce, chunk_log, blocks,
                   ptr(out))
        return [int(v) for v in out]

    def debug_merkle_lde(self, lde, entries=()):
        """Merkle commitment of LDEs as the prover runs it (xfg_debug_merkle_lde): lde [B,nc,blowup,n]
        coset-major, entries = proof << log2(n) | row. Returns (heaps [B,2n,8] u32 words -- slots
        [1, n) defined, the rest 0xFFFFFFFF -- and the opening kernel's local heaps [len(entries),2 blowup,8])"""
        v, ent = array(lde), array(entries)
        B, nc, blowup, n = v.shape
        nodes, local = zeros((B, 2 * n, 8), "<u4"), zeros((ent.size, 2 * blowup, 8), "<u4")
        self._call(_lib.xfg_debug_merkle_lde, B, nc, n, blowup, ptr(v), ptr(ent), ent.size, ptr(nodes, _u8p),
                   ptr(local, _u8p))
        return nodes, local

    def debug_merkle_lde_const(self, lde, flags=None, vals=None, entries=()):
        """debug_merkle_lde for an LDE [B,7,blowup,n] with constant columns (xfg_debug_merkle_lde_const):
        flags [B,7] and vals [B,7] go to the kernels, and the flagged planes are set to 0xFF bytes on the
        device before the launches. flags = vals = None: the dense kernels, blowup up to 128"""
        v, ent = array(lde), array(entries)
        B, nc, blowup, n = v.shape
        if (flags is None) != (vals is None):
            raise XfgStarkError(9, "debug_merkle_lde_const: flags and vals go together")
        fp = vp = None
        if flags is not None:
            f, cv = array(flags, "uint8"), array(vals)
            if f.shape != (B, nc) or cv.shape != (B, nc):
                raise XfgStarkError(9, "debug_merkle_lde_const: flags [B,nc], vals [B,nc]")
            fp, vp = ptr(f, _u8p), ptr(cv)
        nodes, local = zeros((B, 2 * n, 8), "<u4"), zeros((ent.size, 2 * blowup, 8), "<u4")
        self._call(_lib.xfg_debug_merkle_lde_const, B, nc, n, blowup, ptr(v), fp, vp, ptr(ent), ent.size,
                   ptr(nodes, _u8p), ptr(local, _u8p))
        return nodes, local

    def debug_poison_lde(self, on):
        """while on, every unit sets its trace LDE buffer to 0xFF bytes before the transforms (xfg_debug_poison_lde)"""
        self._call(_lib.xfg_debug_poison_lde, 1 if on else 0)

    def debug_merkle_fri(self, vals, logn, logbeta, coset_major, fold=8):
        """Merkle commitment of FRI layers (xfg_debug_merkle_fri_f): vals and fold as for debug_fri_fold. Returns
        the heaps [B,2 rows,8] u32 words, rows = 2^(logn + logbeta) / fold (slot 0: 0xFFFFFFFF)"""
        v = array(vals)
        B, ext, D = v.shape
        if D != 1 << (logn + logbeta):
            raise XfgStarkError(9, "debug_merkle_fri: vals [B,ext,2^(logn+logbeta)]")
        if not 0 < fold < 1 << 32:
            raise XfgStarkError(9, "debug_merkle_fri: fold is 2, 4, 8 or 16")
        nodes = zeros((B, 2 * (D // fold), 8), "<u4")
        self._call(_lib.xfg_debug_merkle_fri_f, B, ext, logn, logbeta, 1 if coset_major else 0, fold, ptr(v),
                   ptr(nodes, _u8p))
        return nodes

    def debug_interpolate(self, evals, n, offset7=False):
        e = array(evals).reshape(-1, n)
        out = zeros(e.shape)
        self._call(_lib.xfg_debug_interpolate, ptr(e), e.shape[0], n, 1 if offset7 else 0, ptr(out))
        return out

    def debug_interpolate_keep(self, evals, n, keep, offset7=False):
        """the truncated inverse transform of the composition polynomial and the FRI remainder: the first
        `keep` coefficients of every polynomial, `keep` words apart. -> (coefficients [npoly][keep], the 8
        guard words behind them, which a correct run leaves at 0xFF..FF)"""
        e = array(evals).reshape(-1, n)
        keep = int(keep)
        if not 0 <= keep < 1 << 64:
            raise XfgStarkError(9, "debug_interpolate_keep: keep is 1..n")
        out = zeros(e.shape[0] * min(keep, n) + 8)
        self._call(_lib.xfg_debug_interpolate_keep, ptr(e), e.shape[0], n, keep, 1 if offset7 else 0, ptr(out))
        return out[:-8].reshape(e.shape[0], keep), out[-8:]

    def debug_interpolate_skip(self, evals, n, skip, offset7=False):
        """debug_interpolate with a flag per polynomial (see debug_lde_skip)"""
        e = array(evals).reshape(-1, n)
        f = array(skip, "uint8", (e.shape[0],), "debug_interpolate_skip: one flag per polynomial")
        out = zeros(e.shape)
        self._call(_lib.xfg_debug_interpolate_skip, ptr(e), e.shape[0], n, 1 if offset7 else 0, ptr(f, _u8p), ptr(out))
        return out
