"""Shared by test_chunk_write_host.py and test_gpu_chunk_write.py: writes
into chunks cut into the parts of a slice, the arguments of one
lizec_chunk_write call, and the bytes it has to produce.

The expected bytes need no oracle entry point of their own.  The columns of
every touched row are put together with numpy by the rule of lizec.h (new
data, else the part's block as it is, else zeros), the parity comes from
oracle.rs_encode (ec) or XOR (xor) over `size` bytes, and the CRCs from
oracle.crc32.  The encode table is the oracle's: rs.recover with every parity
erased, all ones for a xor slice.
"""
import numpy as np

import oracle
from chunk_read_cases import BLOCK, FILL, GUARD, PartStore, Slice  # noqa: F401

WRITE_DTYPE = np.dtype([("data", "<u8"), ("crcs", "<u8"),
                        ("data_stride", "<u4"), ("par_stride", "<u4"),
                        ("first_block", "<u4"), ("block_count", "<u4"),
                        ("from", "<u4"), ("to", "<u4")])


class FirstRows(Slice):
    """The first `rows` parities of ec(k, m): a call with rows < m, for the
    pass sizes that no small slice reaches.  The table is the head of
    ec(k, m)'s, the expected parities the head of its parities."""

    def __init__(self, k, m, rows):
        Slice.__init__(self, "ec", k, m)
        self.full_m, self.m = m, rows
        self.name += f"-rows{rows}"


def encode_table(sl):
    """[m][ks][32], from the oracle."""
    if sl.kind[0] == "xor":
        return oracle.init_tables(np.ones(sl.ks, np.uint8))
    m = getattr(sl, "full_m", sl.m)
    data = (1 << sl.ks) - 1
    tbl, ic, oc = oracle.rs_make_tables(sl.ks, m, data, data,
                                        ((1 << m) - 1) << sl.ks)
    assert (ic, oc) == (sl.ks, m)
    return np.ascontiguousarray(tbl[:32 * sl.ks * sl.m])


def parity_of(sl, cols, size):
    """cols: ks arrays of `size` bytes (None = zeros) -> m parity arrays."""
    cols = [None if c is None else np.ascontiguousarray(c) for c in cols]
    if sl.kind[0] == "xor":
        out = np.zeros(size, np.uint8)
        for c in cols:
            if c is not None:
                out ^= c
        return [out]
    return oracle.rs_encode(sl.ks, getattr(sl, "full_m", sl.m), cols,
                            size)[:sl.m]


class Chunk:
    """A chunk of n blocks of a slice: its data parts as they are now, with
    their offsets in a PartStore (None for a part without a block)."""

    def __init__(self, sl, n, store, seed):
        self.sl, self.n = sl, n
        rng = np.random.default_rng(seed)
        self.blocks = rng.integers(0, 256, (n, BLOCK), np.uint8)
        self.parts = [self.blocks[c::sl.ks] for c in range(sl.ks)]
        self.nb = [p.shape[0] for p in self.parts]
        self.offs = [store.put(p) if p.shape[0] else None
                     for p in self.parts]
        self.memo = {}   # expected values of rows and blocks seen before


class Writes:
    """The writes of one call, with their layout: where the data, the parity
    outputs and the CRC arrays lie, and what the arena has to hold after
    the call.

    par_phase(write index, parity, r0, from) -> the output's address mod 16;
    par_stride(size) -> stride between the touched rows of one parity."""

    def __init__(self, sl):
        self.sl = sl
        self.w = []

    def add(self, chunk, first, count, frm, to, data, data_off, data_stride,
            want=None, crcs=True, fill=True):
        """data: the buffer the new bytes lie in, block i at data_off +
        i * data_stride.  want: the wanted parities (None = all).  fill =
        False passes every fill count as 0 (a write of whole rows)."""
        sl = self.sl
        size = to - frm
        r0, r1 = first // sl.ks, (first + count - 1) // sl.ks
        want = list(range(sl.m)) if want is None else list(want)
        par, crc = {}, []
        # many writes of a call share blocks and whole rows (the host test
        # points every write into one pool of new bytes): each is computed
        # once per chunk
        memo = chunk.memo

        def once(key, fn):
            if key not in memo:
                memo[key] = fn()
            return memo[key]

        for i in range(count):
            at = data_off + i * data_stride
            crc.append(once((id(data), at, size),
                            lambda: oracle.crc32(data[at:at + size])))
        for b in range(r0, r1 + 1):
            cols, key = [], [id(data), b, frm, to]
            for c in range(sl.ks):
                cb = b * sl.ks + c
                if first <= cb < first + count:
                    at = data_off + (cb - first) * data_stride
                    cols.append(data[at:at + size])
                    key.append(at)
                elif b < chunk.nb[c]:
                    assert fill
                    cols.append(chunk.parts[c][b, frm:to])
                    key.append("fill")
                else:
                    cols.append(None)
                    key.append(None)
            p = once(tuple(key), lambda: parity_of(sl, cols, size))
            for r in range(sl.m):
                par[b - r0, r] = p[r]
        self.w.append(dict(chunk=chunk, first=first, count=count, frm=frm,
                           to=to, size=size, data_off=data_off,
                           data_stride=data_stride, want=want, crcs=crcs,
                           fill=fill, touched=r1 - r0 + 1, r0=r0, par=par,
                           crc=crc))

    def __len__(self):
        return len(self.w)

    def layout(self, par_phase, par_stride):
        """Places every parity output and CRC array in an arena of FILL, each
        between GUARD bytes; returns (arena size, expected arena)."""
        at = 0
        for i, w in enumerate(self.w):
            w["pstride"] = par_stride(w["size"])
            span = (w["touched"] - 1) * w["pstride"] + w["size"]
            w["par_off"] = {}
            for r in w["want"]:
                ph = par_phase(i, r, w["r0"], w["frm"]) % 16
                w["par_off"][r] = at + GUARD + ph
                at += (GUARD + 16 + span + GUARD + 15) // 16 * 16
            w["crc_off"] = None
            if w["crcs"]:
                w["crc_off"] = at + GUARD
                at += GUARD + 4 * (w["count"] + w["touched"] * self.sl.m) + \
                    GUARD
                at = (at + 15) // 16 * 16
        want = np.full(at, FILL, np.uint8)
        for w in self.w:
            for r, off in w["par_off"].items():
                for i in range(w["touched"]):
                    o = off + i * w["pstride"]
                    want[o:o + w["size"]] = w["par"][i, r]
            if w["crc_off"] is None:
                continue
            slots = {i: c for i, c in enumerate(w["crc"])}
            for i in range(w["touched"]):
                for r in w["want"]:
                    memo, arr = w["chunk"].memo, w["par"][i, r]
                    if ("crc", id(arr)) not in memo:   # arr lives in memo
                        memo["crc", id(arr)] = oracle.crc32(arr)
                    slots[w["count"] + i * self.sl.m + r] = \
                        memo["crc", id(arr)]
            for k, c in slots.items():
                o = w["crc_off"] + 4 * k
                want[o:o + 4] = np.frombuffer(
                    np.uint32(c).tobytes(), np.uint8)
        return at, want

    def arrays(self, store_base, data_base, arena_base):
        """(writes, fill_ptrs, fill_nb, par_ptrs) for the three buffers at
        these addresses; layout() must have run."""
        sl = self.sl
        W = len(self.w)
        wr = np.zeros(W, WRITE_DTYPE)
        fp = np.zeros((W, sl.ks), np.uint64)
        fn = np.zeros((W, sl.ks), np.uint32)
        pp = np.zeros((W, sl.m), np.uint64)
        for i, w in enumerate(self.w):
            wr[i] = (data_base + w["data_off"],
                     0 if w["crc_off"] is None else arena_base + w["crc_off"],
                     w["data_stride"], w["pstride"], w["first"], w["count"],
                     w["frm"], w["to"])
            if w["fill"]:
                for c in range(sl.ks):
                    if w["chunk"].nb[c]:
                        fp[i, c] = store_base + w["chunk"].offs[c]
                        fn[i, c] = w["chunk"].nb[c]
            for r, off in w["par_off"].items():
                pp[i, r] = arena_base + off
        return wr, fp, fn, pp


def block_ranges(limit):
    """Every (first, count) inside [0, limit)."""
    return [(f, c) for f in range(limit) for c in range(1, limit - f + 1)]
