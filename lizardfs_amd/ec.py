"""Batched Reed-Solomon encode/decode on MI355X — the GPU mirror of the
reference's ReedSolomon<32,32> (reed_solomon.h:41-373) plugin surface.

Parts are torch uint8 tensors resident on the GPU; PyTorch provides memory
and streams, liblizec.so provides the compute.  Semantics mirror the
reference exactly: parts indexed 0..k+m-1 (data then parity,
slice_traits.h:183-197), None input = implicit zero part
(reed_solomon.h:79), exactly m erased parts per recover call
(reed_solomon.h:95), per-(erasure-pattern) table cache
(reed_solomon.h:194-198).
"""
import ctypes
import hashlib

import numpy as np
import torch

from . import lib as L
from . import slice_traits


_BLOCK = slice_traits.BLOCK_SIZE   # 64 KiB


def _tables_cache_key(k, m, present, nonnull, needed):
    return (k, m, present, nonnull, needed)


# Plan-cache keys.  A cached plan holds device pointer arrays built from the
# addresses, row strides and geometry of one call, so every number those
# arrays (or the tables) are computed from must be part of the key.  Pure
# functions of ints and tuples: no tensors, no engine.

def enc_plan_key(data_addr, parity_addr, S, plen):
    """encode_batch(data, parity=...): both tensors are contiguous, so the
    two base addresses, S and plen fix every part address."""
    return ("enc", int(data_addr), int(parity_addr), int(S), int(plen))


def rec_plan_key(present, nonnull, needed, src_addrs, src_strides, out_addrs,
                 S, plen):
    """recover_batch(..., out=...): fragment j's row s lies at
    src_addrs[j] + s*src_strides[j]; the outputs are contiguous."""
    return ("rec", int(present), int(nonnull), int(needed),
            tuple(int(a) for a in src_addrs),
            tuple(int(x) for x in src_strides),
            tuple(int(a) for a in out_addrs), int(S), int(plen))


def mix_plan_key(digest, bases, strides, out_addr, S, plen):
    """recover_batch_mixed(..., out=...): `digest` covers the per-stripe
    patterns (table index, output slots, erased masks)."""
    return ("mix", bytes(digest), tuple(int(b) for b in bases),
            tuple(int(x) for x in strides), int(out_addr), int(S), int(plen))


_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _pattern_masks(sets, nparts, what):
    """Per-stripe index sets -> (uint64 bitmask [S], set size [S]).  An
    integer ndarray [S, n] (one row per stripe) takes a vectorised path."""
    if isinstance(sets, np.ndarray) and sets.ndim == 2 and \
            sets.dtype.kind in "iu":
        if sets.size and (sets.min() < 0 or sets.max() >= nparts):
            raise ValueError(f"{what}: part index out of [0,{nparts})")
        bits = np.uint64(1) << sets.astype(np.uint64)
        masks = np.bitwise_or.reduce(bits, axis=1) if sets.shape[1] else \
            np.zeros(sets.shape[0], np.uint64)
        masks = masks.astype(np.uint64)
    else:
        masks = np.empty(len(sets), np.uint64)
        for s, idx in enumerate(sets):
            v = 0
            for i in idx:
                i = int(i)
                if not 0 <= i < nparts:
                    raise ValueError(
                        f"{what}[{s}]: part index {i} out of [0,{nparts})")
                v |= 1 << i
            masks[s] = v
    masks = np.ascontiguousarray(masks)
    sizes = _POPCOUNT8[masks.view(np.uint8).reshape(-1, 8)].sum(axis=1)
    return masks, sizes


# (k, m, erased mask, want mask) -> (ISA-L table bytes, rebuilt parts): the
# matrix inversion behind a pattern is done once per process, like the
# reference's per-pattern matrix cache (reed_solomon.h:194-198).
_pattern_cache = {}
_PATTERN_CACHE_MAX = 16384


def _pattern_table(k, m, em, wm):
    key = (k, m, em, wm)
    t = _pattern_cache.get(key)
    if t is None:
        nparts = k + m
        present = ((1 << nparts) - 1) & ~em
        tbl = np.zeros(32 * 32 * 32, np.uint8)
        ic = ctypes.c_int()
        oc = ctypes.c_int()
        L.check(L.lib().lizec_rs_tables(
            k, m, present, present, wm,
            tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            ctypes.byref(ic), ctypes.byref(oc)), "lizec_rs_tables")
        assert ic.value == k
        parts = [i for i in range(nparts) if (wm >> i) & 1]
        assert oc.value == len(parts)
        t = (tbl[:32 * k * oc.value].copy(), parts)
        if len(_pattern_cache) >= _PATTERN_CACHE_MAX:
            _pattern_cache.clear()
        _pattern_cache[key] = t
    return t


def build_pattern_tables(k, m, erased, want=None):
    """Recover tables for a batch whose stripes carry their own erasure
    patterns (host-side only; needs no GPU).

    erased: length-S sequence of index sets, exactly m indices each
      (reed_solomon.h:95), or an integer ndarray [S, m].
    want: length-S sequence of non-empty subsets of the matching erased
      set (default: the erased sets).
    Returns (tables, index, slots):
      tables uint8 [P, 32*k*oc] — one ISA-L-layout table per distinct
        (erased, want) pair, oc = the largest want size; a pattern wanting
        fewer parts has zero rows for its unused outputs;
      index  uint32 [S] — stripe -> row of `tables`;
      slots  int64 [S, oc] — part rebuilt in each output slot, ascending,
        -1 for an unused slot.
    """
    tables, index, pslots, _ = _pattern_tables(k, m, erased, want)
    return tables, index, pslots[index]


def _pattern_tables(k, m, erased, want):
    """build_pattern_tables, per pattern: (tables [P, .], index [S],
    slots [P, oc], erased masks [P])."""
    nparts = k + m
    emask, esize = _pattern_masks(erased, nparts, "erased")
    S = emask.shape[0]
    if S == 0:
        raise ValueError("no stripes")
    if np.any(esize != m):
        s = int(np.argmax(esize != m))
        raise ValueError(f"erased[{s}]: exactly m={m} erased parts required "
                         f"(got {int(esize[s])})")
    if want is None or want is erased:
        wmask, wsize = emask, esize
    else:
        wmask, wsize = _pattern_masks(want, nparts, "want")
        if wmask.shape[0] != S:
            raise ValueError(f"want has {wmask.shape[0]} entries, erased {S}")
        if np.any(wsize == 0):
            raise ValueError(f"want[{int(np.argmax(wsize == 0))}] is empty")
        bad = (wmask & ~emask) != 0
        if np.any(bad):
            raise ValueError(f"want[{int(np.argmax(bad))}] must be a subset "
                             f"of erased")
    oc = int(wsize.max())
    if 2 * nparts <= 64:
        # both masks fit one word: a 1-D unique is much faster at large S
        sh = np.uint64(nparts)
        keys, index = np.unique((emask << sh) | wmask, return_inverse=True)
        pairs = np.stack([keys >> sh,
                          keys & np.uint64((1 << nparts) - 1)], axis=1)
    else:
        pairs, index = np.unique(np.stack([emask, wmask], axis=1), axis=0,
                                 return_inverse=True)
    index = np.ascontiguousarray(index.reshape(-1).astype(np.uint32))
    P = pairs.shape[0]
    tables = np.zeros((P, 32 * k * oc), np.uint8)
    pslots = np.full((P, oc), -1, np.int64)
    for p in range(P):
        tbl, parts = _pattern_table(k, m, int(pairs[p, 0]), int(pairs[p, 1]))
        tables[p, :tbl.size] = tbl
        pslots[p, :len(parts)] = parts
    return tables, index, pslots, np.ascontiguousarray(pairs[:, 0])


class ReedSolomon:
    """Reed-Solomon ec(k,m) over batches of stripes on one GPU."""

    def __init__(self, k, m, device=0):
        if not (slice_traits.MIN_DATA <= k <= slice_traits.MAX_DATA):
            raise ValueError(f"k={k} out of [2,32]")
        if not (slice_traits.MIN_PARITY <= m <= slice_traits.MAX_PARITY):
            raise ValueError(f"m={m} out of [1,32]")
        self.k = k
        self.m = m
        self.device = device
        self.slice_type = slice_traits.ec_slice_type(k, m)
        self._tables = {}
        self._plans = {}
        self._engine = L.engine(device)
        self._lib = L.lib()

    def __del__(self):
        try:
            for p in getattr(self, "_plans", {}).values():
                self._lib.lizec_ec_plan_destroy(p)
        except Exception:
            pass

    # ---------------- tables (host-side matrix algebra) ---

    def _get_tables(self, present, nonnull, needed):
        key = _tables_cache_key(self.k, self.m, present, nonnull, needed)
        t = self._tables.get(key)
        if t is None:
            tbl = np.zeros(32 * 32 * 32, np.uint8)
            ic = ctypes.c_int()
            oc = ctypes.c_int()
            L.check(self._lib.lizec_rs_tables(
                self.k, self.m, present, nonnull, needed,
                tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                ctypes.byref(ic), ctypes.byref(oc)), "lizec_rs_tables")
            t = (np.ascontiguousarray(tbl[:32 * ic.value * oc.value]),
                 ic.value, oc.value)
            self._tables[key] = t
        return t

    # ---------------- batch ops ----------------

    def _run(self, part_len, tbl, ic, oc, src_ptrs, dst_ptrs, nstripes,
             plan_key=None):
        """Launch a batch.  When plan_key is given (stable buffers), the
        device-side tables+pointer arrays are built once and reused
        (lizec_ec_plan_*), so steady-state steps do zero host->device
        traffic — mirroring the reference's matrix cache."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if plan_key is not None:
            plan = self._plans.get(plan_key)
            if plan is None:
                while len(self._plans) >= 64:   # bound device-side state
                    oldest = next(iter(self._plans))
                    self._lib.lizec_ec_plan_destroy(self._plans.pop(oldest))
                plan = ctypes.c_void_p()
                L.check(self._lib.lizec_ec_plan_create(
                    self._engine, part_len, ic, oc,
                    tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                    src_ptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                    dst_ptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                    nstripes, ctypes.byref(plan)), "lizec_ec_plan_create")
                self._plans[plan_key] = plan
            L.check(self._lib.lizec_ec_plan_run(plan, ctypes.c_void_p(stream)),
                    "lizec_ec_plan_run")
            return
        L.check(self._lib.lizec_ec_encode_batch(
            self._engine, part_len, ic, oc,
            tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            src_ptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            dst_ptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            nstripes, ctypes.c_void_p(stream)), "lizec_ec_encode_batch")

    @staticmethod
    def _check_part(t, what):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous CUDA uint8 tensor")

    @staticmethod
    def _check_aligned(t, what, row_stride=0):
        """The kernels move parts in 16-byte vectors (lizec.h): every part
        row of `t` must start on a 16-byte boundary."""
        if t.data_ptr() % 16 or row_stride % 16:
            raise ValueError(f"{what}: part rows must be 16-byte aligned "
                             f"(address {t.data_ptr():#x}, row stride "
                             f"{row_stride})")

    @staticmethod
    def _frag_geom(t, what):
        """[S, L] fragment, possibly a strided view (e.g. data[:, i, :]):
        rows must be contiguous; returns (S, L, row_stride_bytes)."""
        if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 2 or \
                t.stride(1) != 1:
            raise ValueError(f"{what} must be a CUDA uint8 [S, L] tensor "
                             f"with contiguous rows")
        return t.shape[0], t.shape[1], t.stride(0)

    def encode_batch(self, data, parity=None):
        """Compute parity for a batch of stripes.

        data: uint8 CUDA tensor [S, k, L] (contiguous), L % 16 == 0.
        Returns parity [S, m, L] (allocated if not given).
        Mirrors ReedSolomon::encode (reed_solomon.h:134-155) /
        ChunkWriter::computeParityBlock (chunk_writer.cc:365-402), batched.
        """
        self._check_part(data, "data")
        S, k, plen = data.shape
        if k != self.k:
            raise ValueError(f"data has {k} parts, expected {self.k}")
        if plen % 16:
            raise ValueError("part length must be a multiple of 16")
        self._check_aligned(data, "data")
        caller_parity = parity is not None
        if parity is None:
            parity = torch.empty((S, self.m, plen), dtype=torch.uint8,
                                 device=data.device)
        else:
            self._check_part(parity, "parity")
            if tuple(parity.shape) != (S, self.m, plen):
                raise ValueError(f"parity must be [S={S}, m={self.m}, "
                                 f"L={plen}], got {tuple(parity.shape)}")
            self._check_aligned(parity, "parity")

        dmask = (1 << self.k) - 1
        pmask = ((1 << self.m) - 1) << self.k
        tbl, ic, oc = self._get_tables(dmask, dmask, pmask)
        assert (ic, oc) == (self.k, self.m)

        src = (data.data_ptr() +
               np.arange(S * k, dtype=np.uint64) * np.uint64(plen))
        dst = (parity.data_ptr() +
               np.arange(S * self.m, dtype=np.uint64) * np.uint64(plen))
        # plans are cached only for caller-owned (stable) output buffers
        plan_key = (enc_plan_key(data.data_ptr(), parity.data_ptr(), S, plen)
                    if caller_parity else None)
        self._run(plen, tbl, ic, oc, src, dst, S, plan_key=plan_key)
        return parity

    def recover_batch(self, fragments, erased, want=None, out=None):
        """Recover missing parts for a batch of stripes.

        fragments: list of k+m entries; entry i is a uint8 CUDA tensor [S, L]
          for an available part, or None (erased part, or available-but-zero
          part if i not in `erased` — reed_solomon.h:79).
        erased: iterable of part indices (exactly m of them,
          reed_solomon.h:95; pad with available parts you don't need, as
          ec_read_plan.h:126-133 does).
        want: indices to reconstruct (default: all erased).
        Returns dict part_index -> uint8 tensor [S, L].
        """
        nparts = self.k + self.m
        if len(fragments) != nparts:
            raise ValueError(f"need {nparts} fragment slots")
        erased = frozenset(erased)
        if len(erased) != self.m:
            raise ValueError(f"exactly m={self.m} erased parts required "
                             f"(got {len(erased)}); pad like ec_read_plan.h:126")
        want = frozenset(want) if want is not None else erased
        if not want.issubset(erased):
            raise ValueError("want must be a subset of erased")

        present = 0
        nonnull = 0
        needed = 0
        S = plen = dev = None
        for i in range(nparts):
            if i in erased:
                continue
            present |= 1 << i
            if fragments[i] is not None:
                s, l, rs = self._frag_geom(fragments[i], f"fragment {i}")
                if S is not None and (s, l) != (S, plen):
                    raise ValueError(
                        f"fragment {i} is [{s}, {l}], expected [{S}, {plen}]")
                self._check_aligned(fragments[i], f"fragment {i}",
                                    rs if s > 1 else 0)
                nonnull |= 1 << i
                S, plen = s, l
                dev = fragments[i].device
        for i in want:
            needed |= 1 << i
        if S is None:
            raise ValueError("all surviving parts are None")
        if plen % 16:
            raise ValueError("part length must be a multiple of 16")

        tbl, ic, oc = self._get_tables(present, nonnull, needed)

        srcs = [fragments[i] for i in range(nparts)
                if (nonnull >> i) & 1]
        if out is not None:
            outs = out   # caller-provided stable buffers -> plan is cached
            for i in want:
                self._check_part(outs[i], f"out[{i}]")
                if tuple(outs[i].shape) != (S, plen):
                    raise ValueError(f"out[{i}] must be [S={S}, L={plen}], "
                                     f"got {tuple(outs[i].shape)}")
                self._check_aligned(outs[i], f"out[{i}]")
        else:
            outs = {i: torch.empty((S, plen), dtype=torch.uint8, device=dev)
                    for i in sorted(want)}
        rows = np.arange(S, dtype=np.uint64)
        src = np.empty((S, ic), np.uint64)
        rstrides = [self._frag_geom(t, "fragment")[2] for t in srcs]
        for j, t in enumerate(srcs):
            src[:, j] = t.data_ptr() + rows * np.uint64(rstrides[j])
        dst = np.empty((S, oc), np.uint64)
        for j, i in enumerate(sorted(want)):
            dst[:, j] = outs[i].data_ptr() + rows * np.uint64(plen)
        plan_key = None
        if out is not None:
            plan_key = rec_plan_key(
                present, nonnull, needed, [t.data_ptr() for t in srcs],
                rstrides, [outs[i].data_ptr() for i in sorted(want)], S, plen)
        self._run(plen, tbl, ic, oc, np.ascontiguousarray(src.ravel()),
                  np.ascontiguousarray(dst.ravel()), S, plan_key=plan_key)
        return outs

    def recover_batch_blocks(self, fragments, erased, want=None, out=None, *,
                             nblocks, src_stride=_BLOCK, dst_stride=_BLOCK):
        """recover_batch over parts stored as 64 KiB blocks at a fixed
        stride, at addresses that need only be 4-byte aligned
        (lizec_ec_encode_batch_strided) — survivors read straight from
        INTERLEAVED-format images, parts rebuilt straight into them.

        fragments, erased, want: as for recover_batch, except that a
          fragment is a [S, span] row view starting at block 0's DATA (for
          an INTERLEAVED image batch, img[:, 4:]); block b of row s lies at
          byte b*src_stride of the row, span >= (nblocks-1)*src_stride +
          65536.  Encode is the case erased = want = the parity parts.
        out: dict part -> [S, span] row view laid out the same way with
          dst_stride; required unless dst_stride is 65536, where plain
          [S, nblocks*65536] tensors are allocated.  Only the blocks are
          written: bytes between them (the CRC slots) keep their value.
        Rows and strides must be multiples of 4 bytes.
        Returns dict part_index -> tensor.
        """
        nparts = self.k + self.m
        if len(fragments) != nparts:
            raise ValueError(f"need {nparts} fragment slots")
        erased = frozenset(erased)
        if len(erased) != self.m:
            raise ValueError(f"exactly m={self.m} erased parts required "
                             f"(got {len(erased)}); pad like ec_read_plan.h:126")
        want = frozenset(want) if want is not None else erased
        if not want.issubset(erased):
            raise ValueError("want must be a subset of erased")
        nblocks = int(nblocks)
        if nblocks < 1 or nblocks * _BLOCK > 1 << 31:
            raise ValueError(f"nblocks={nblocks} out of [1, 32768]")
        for name, stride in (("src_stride", src_stride),
                             ("dst_stride", dst_stride)):
            if stride < _BLOCK or stride % 4:
                raise ValueError(f"{name}={stride} must be a multiple of 4 "
                                 f"and at least {_BLOCK}")
        if out is None and dst_stride != _BLOCK:
            raise ValueError("out is required when dst_stride != 65536")

        def rows_of(t, what, stride):
            """[S, span] view -> (S, row addresses), layout checked."""
            s, span, rstride = self._frag_geom(t, what)
            need = (nblocks - 1) * stride + _BLOCK
            if span < need:
                raise ValueError(f"{what}: rows of {span} bytes cannot hold "
                                 f"{nblocks} blocks at stride {stride} "
                                 f"({need} bytes)")
            if t.data_ptr() % 4 or (s > 1 and rstride % 4):
                raise ValueError(f"{what}: block data must be 4-byte aligned "
                                 f"(address {t.data_ptr():#x}, row stride "
                                 f"{rstride})")
            return s, (t.data_ptr() +
                       np.arange(s, dtype=np.uint64) * np.uint64(rstride))

        present = nonnull = needed = 0
        S = dev = None
        src_cols = []
        for i in range(nparts):
            if i in erased:
                continue
            present |= 1 << i
            if fragments[i] is not None:
                s, rows = rows_of(fragments[i], f"fragment {i}", src_stride)
                if S is not None and s != S:
                    raise ValueError(f"fragment {i} has {s} rows, "
                                     f"expected {S}")
                nonnull |= 1 << i
                S, dev = s, fragments[i].device
                src_cols.append(rows)
        for i in want:
            needed |= 1 << i
        if S is None:
            raise ValueError("all surviving parts are None")

        tbl, ic, oc = self._get_tables(present, nonnull, needed)
        if out is not None:
            outs = out
        else:
            outs = {i: torch.empty((S, nblocks * _BLOCK), dtype=torch.uint8,
                                   device=dev) for i in sorted(want)}
        dst_cols = []
        for i in sorted(want):
            s, rows = rows_of(outs[i], f"out[{i}]", dst_stride)
            if s != S:
                raise ValueError(f"out[{i}] has {s} rows, expected {S}")
            dst_cols.append(rows)
        src = np.ascontiguousarray(np.stack(src_cols, axis=1).ravel())
        dst = np.ascontiguousarray(np.stack(dst_cols, axis=1).ravel())
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(self._lib.lizec_ec_encode_batch_strided(
            self._engine, nblocks, ic, oc,
            tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            src.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            dst.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            S, src_stride, dst_stride, ctypes.c_void_p(stream)),
            "lizec_ec_encode_batch_strided")
        return outs

    def recover_batch_mixed(self, fragments, erased, want=None, out=None):
        """Recover missing parts for a batch whose stripes each carry their
        own erasure pattern, in one call (lizec_ec_encode_batch_multi).

        fragments: list of k+m uint8 CUDA tensors [S, L] (strided row views
          allowed, as in recover_batch).  None is not allowed: every stripe
          reads exactly k sources.  Rows of a part erased in a stripe are
          ignored; a stripe's sources are its k surviving parts, ascending.
        erased / want: per-stripe index sets, see build_pattern_tables.
        out: optional uint8 CUDA tensor [S, oc, L] (contiguous); supplying
          it makes the buffers stable, so the plan is cached.
        Returns (out [S, oc, L], slots [S, oc]): out[s, j] holds part
        slots[s, j]; slots of -1 are passed as address 0 and never written.
        """
        nparts = self.k + self.m
        if len(fragments) != nparts:
            raise ValueError(f"need {nparts} fragments")
        S = plen = dev = None
        bases = np.empty(nparts, np.uint64)
        strides = np.empty(nparts, np.uint64)
        for i, t in enumerate(fragments):
            if t is None:
                raise ValueError(f"fragment {i} is None: recover_batch_mixed "
                                 f"needs all k+m tensors")
            s, l, rstride = self._frag_geom(t, f"fragment {i}")
            if S is not None and (s, l) != (S, plen):
                raise ValueError(
                    f"fragment {i} is [{s}, {l}], expected [{S}, {plen}]")
            self._check_aligned(t, f"fragment {i}", rstride if s > 1 else 0)
            S, plen, dev = s, l, t.device
            bases[i] = t.data_ptr()
            strides[i] = rstride
        if plen % 16:
            raise ValueError("part length must be a multiple of 16")

        tables, index, pslots, pemask = _pattern_tables(self.k, self.m,
                                                        erased, want)
        slots = pslots[index]
        if index.shape[0] != S:
            raise ValueError(f"{index.shape[0]} patterns for {S} stripes")
        oc = slots.shape[1]
        if out is not None:
            self._check_part(out, "out")
            if tuple(out.shape) != (S, oc, plen):
                raise ValueError(f"out must be [S={S}, oc={oc}, L={plen}], "
                                 f"got {tuple(out.shape)}")
            self._check_aligned(out, "out")
            outs = out
        else:
            outs = torch.empty((S, oc, plen), dtype=torch.uint8, device=dev)

        def call(fn, last, what):
            # sources: each pattern's k surviving parts in ascending order
            palive = np.array(
                [[i for i in range(nparts) if not (int(e) >> i) & 1]
                 for e in pemask], np.intp)
            alive = palive[index]                              # [S, k]
            rows = np.arange(S, dtype=np.uint64)[:, None]
            src = np.ascontiguousarray(bases[alive] + rows * strides[alive])
            dst = (np.uint64(outs.data_ptr()) +
                   np.arange(S * oc, dtype=np.uint64).reshape(S, oc) *
                   np.uint64(plen))
            dst = np.ascontiguousarray(np.where(slots >= 0, dst,
                                                np.uint64(0)))
            u8p = ctypes.POINTER(ctypes.c_uint8)
            u32p = ctypes.POINTER(ctypes.c_uint32)
            u64p = ctypes.POINTER(ctypes.c_uint64)
            L.check(fn(self._engine, plen, self.k, oc,
                       tables.ctypes.data_as(u8p), tables.shape[0],
                       index.ctypes.data_as(u32p), src.ctypes.data_as(u64p),
                       dst.ctypes.data_as(u64p), S, last), what)

        stream = torch.cuda.current_stream(self.device).cuda_stream
        if out is None:
            call(self._lib.lizec_ec_encode_batch_multi,
                 ctypes.c_void_p(stream), "lizec_ec_encode_batch_multi")
            return outs, slots
        # stable buffers: the pointer arrays are only built on a plan miss
        h = hashlib.blake2b(digest_size=16)
        h.update(index.tobytes())
        h.update(pslots.tobytes())
        h.update(pemask.tobytes())
        plan_key = mix_plan_key(h.digest(), bases, strides, outs.data_ptr(),
                                S, plen)
        plan = self._plans.get(plan_key)
        if plan is None:
            while len(self._plans) >= 64:   # bound device-side state
                oldest = next(iter(self._plans))
                self._lib.lizec_ec_plan_destroy(self._plans.pop(oldest))
            plan = ctypes.c_void_p()
            call(self._lib.lizec_ec_plan_create_multi, ctypes.byref(plan),
                 "lizec_ec_plan_create_multi")
            self._plans[plan_key] = plan
        L.check(self._lib.lizec_ec_plan_run(plan, ctypes.c_void_p(stream)),
                "lizec_ec_plan_run")
        return outs, slots

    def _per_stripe_sets(self, sets, S, what):
        """One index set for all stripes, or one per stripe -> per stripe."""
        if isinstance(sets, np.ndarray):
            if sets.ndim == 2:
                per = sets
            elif sets.ndim == 1:
                per = np.broadcast_to(sets, (S, sets.shape[0]))
                per = np.ascontiguousarray(per)
            else:
                raise ValueError(f"{what}: expected 1 or 2 dimensions")
        else:
            sets = list(sets)
            if sets and all(isinstance(i, (int, np.integer)) for i in sets):
                per = [sets] * S
            else:
                per = sets
        if len(per) != S:
            raise ValueError(f"{what} has {len(per)} entries for {S} stripes")
        return per

    def _ragged_prepare(self, fragments, erased, want, part_blocks,
                        src_stride, allow_empty=False):
        """Argument checks and the source side of a ragged call:
        (S, device, tables, index, slots, src addresses [S, k], src counts
        [S, k], dst counts [S, oc])."""
        nparts = self.k + self.m
        if len(fragments) != nparts:
            raise ValueError(f"need {nparts} fragment slots")
        pb = np.asarray(part_blocks)
        if pb.ndim != 2 or pb.shape[1] != nparts or pb.shape[0] < 1 or \
                pb.dtype.kind not in "iu":
            raise ValueError(f"part_blocks must be an int array "
                             f"[S, {nparts}]")
        if pb.min() < 0 or pb.max() > 32768:
            raise ValueError("part_blocks out of [0, 32768]")
        pb = pb.astype(np.int64)
        S = pb.shape[0]
        if src_stride < _BLOCK or src_stride % 4:
            raise ValueError(f"src_stride={src_stride} must be a multiple "
                             f"of 4 and at least {_BLOCK}")
        erased = self._per_stripe_sets(erased, S, "erased")
        if want is not None:
            want = self._per_stripe_sets(want, S, "want")
        tables, index, pslots, pemask = _pattern_tables(self.k, self.m,
                                                        erased, want)
        slots = pslots[index]
        # sources: each pattern's k surviving parts in ascending order
        palive = np.array(
            [[i for i in range(nparts) if not (int(e) >> i) & 1]
             for e in pemask], np.intp)
        alive = palive[index]                                  # [S, k]
        read = np.zeros(nparts, bool)
        read[np.unique(alive)] = True
        bases = np.zeros(nparts, np.uint64)
        strides = np.zeros(nparts, np.uint64)
        dev = None
        for i, t in enumerate(fragments):
            if t is None:
                if read[i]:
                    raise ValueError(f"fragment {i} is None but survives in "
                                     f"some stripe")
                continue
            s, span, rstride = self._frag_geom(t, f"fragment {i}")
            if s != S:
                raise ValueError(f"fragment {i} has {s} rows, expected {S}")
            top = int(pb[:, i].max())
            need = (top - 1) * src_stride + _BLOCK if top else 0
            if span < need:
                raise ValueError(f"fragment {i}: rows of {span} bytes cannot "
                                 f"hold {top} blocks at stride {src_stride} "
                                 f"({need} bytes)")
            if t.data_ptr() % 4 or (s > 1 and rstride % 4):
                raise ValueError(f"fragment {i}: block data must be 4-byte "
                                 f"aligned (address {t.data_ptr():#x}, row "
                                 f"stride {rstride})")
            dev = t.device
            bases[i] = t.data_ptr()
            strides[i] = rstride
        if dev is None:
            raise ValueError("all fragments are None")
        rows = np.arange(S, dtype=np.uint64)[:, None]
        src = np.ascontiguousarray(bases[alive] + rows * strides[alive])
        src_nb = np.ascontiguousarray(
            np.take_along_axis(pb, alive, axis=1).astype(np.uint32))
        dst_nb = np.take_along_axis(pb, np.maximum(slots, 0), axis=1)
        dst_nb = np.ascontiguousarray(
            np.where(slots >= 0, dst_nb, 0).astype(np.uint32))
        if not allow_empty and not dst_nb.any():
            raise ValueError("no wanted part has any block")
        return S, dev, tables, index, slots, src, src_nb, dst_nb

    def _ragged_call(self, tables, index, src, src_nb, dst, dst_nb,
                     src_stride, dst_stride):
        """lizec_ec_encode_batch_ragged over prepared host arrays."""
        S, oc = dst_nb.shape
        u8p = ctypes.POINTER(ctypes.c_uint8)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        dst = np.ascontiguousarray(dst, np.uint64)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(self._lib.lizec_ec_encode_batch_ragged(
            self._engine, self.k, oc, tables.ctypes.data_as(u8p),
            tables.shape[0], index.ctypes.data_as(u32p),
            src.ctypes.data_as(u64p), src_nb.ctypes.data_as(u32p),
            dst.ctypes.data_as(u64p), dst_nb.ctypes.data_as(u32p), S,
            src_stride, dst_stride, ctypes.c_void_p(stream)),
            "lizec_ec_encode_batch_ragged")

    def recover_batch_ragged(self, fragments, erased, want=None, out=None, *,
                             part_blocks, src_stride=_BLOCK,
                             dst_stride=_BLOCK):
        """Recover missing parts for a batch whose chunks differ in length
        (and, if wanted, in erasure pattern) in one call
        (lizec_ec_encode_batch_ragged): the ragged sibling of
        recover_batch_mixed and recover_batch_blocks.

        part_blocks: int array [S, k+m], 64 KiB blocks of every part of
          every stripe (slice_traits.number_of_blocks of the chunk's block
          count); a part ends where the zeros past the end of its chunk
          begin.
        erased / want: one index set for all stripes, or per-stripe sets as
          in build_pattern_tables.
        fragments: list of k+m [S, span] row views as in
          recover_batch_blocks; span must cover the largest count of that
          part.  Blocks at or beyond part_blocks[s, i] are never read and
          count as zeros.  None is allowed only for a part that is erased
          in every stripe.
        out: optional [S, oc, span_out] uint8 CUDA tensor with contiguous
          rows (a view is fine), blocks at dst_stride; required unless
          dst_stride is 65536.
        Returns (out [S, oc, span_out], slots [S, oc]) as
        recover_batch_mixed does; of out[s, j] only the blocks below
        part_blocks[s, slots[s, j]] are written.  Encode is the case
        erased = want = the parity parts.
        """
        if dst_stride < _BLOCK or dst_stride % 4:
            raise ValueError(f"dst_stride={dst_stride} must be a multiple "
                             f"of 4 and at least {_BLOCK}")
        if out is None and dst_stride != _BLOCK:
            raise ValueError("out is required when dst_stride != 65536")
        S, dev, tables, index, slots, src, src_nb, dst_nb = \
            self._ragged_prepare(fragments, erased, want, part_blocks,
                                 src_stride)
        oc = slots.shape[1]
        need = (int(dst_nb.max()) - 1) * dst_stride + _BLOCK
        if out is None:
            out = torch.empty((S, oc, need), dtype=torch.uint8, device=dev)
        else:
            if out.dtype != torch.uint8 or not out.is_cuda or \
                    out.dim() != 3 or out.stride(2) != 1 or \
                    tuple(out.shape[:2]) != (S, oc):
                raise ValueError(f"out must be a CUDA uint8 [S={S}, oc={oc}, "
                                 f"span] tensor with contiguous rows")
            if out.shape[2] < need:
                raise ValueError(f"out: rows of {out.shape[2]} bytes cannot "
                                 f"hold {int(dst_nb.max())} blocks at stride "
                                 f"{dst_stride} ({need} bytes)")
            if out.data_ptr() % 4 or out.stride(0) % 4 or out.stride(1) % 4:
                raise ValueError("out: block data must be 4-byte aligned")
        dst = (np.uint64(out.data_ptr()) +
               np.arange(S, dtype=np.uint64)[:, None] *
               np.uint64(out.stride(0)) +
               np.arange(oc, dtype=np.uint64)[None, :] *
               np.uint64(out.stride(1)))
        self._ragged_call(tables, index, src, src_nb, dst, dst_nb,
                          src_stride, dst_stride)
        return out, slots

    def sync(self):
        L.check(self._lib.lizec_engine_sync(self._engine))
