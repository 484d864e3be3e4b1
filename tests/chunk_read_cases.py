"""Shared by test_chunk_read_host.py and test_gpu_chunk_read.py: chunks cut
into the parts of a slice, and the arguments of one lizec_chunk_read call.

A chunk read returns the chunk, so the expected bytes need no oracle entry
point of their own: a random chunk of n blocks is cut round-robin into data
parts with numpy, the parities come from oracle.rs_encode (ec) or XOR (xor)
over rows zero-padded past n, and whatever a read rebuilds must equal the
chunk blocks it was cut from.
"""
import itertools

import numpy as np

import oracle

BLOCK = 65536
GUARD = 256
FILL = 0xA5
LOST = 0x80
UNMAPPED = 0xFF


class Slice:
    """kind: ("std",), ("xor", N) or ("ec", k, m).  cols[c] is the slice part
    behind view column c; a xor slice keeps its parity at part 0."""

    def __init__(self, *kind):
        self.kind = kind
        if kind[0] == "std":
            self.ks, self.m, self.cols = 1, 0, [0]
        elif kind[0] == "xor":
            self.ks, self.m = kind[1], 1
            self.cols = list(range(1, kind[1] + 1))
        else:
            self.ks, self.m = kind[1], kind[2]
            self.cols = list(range(kind[1]))
        self.nparts = self.ks + self.m
        self.parity = [p for p in range(self.nparts) if p not in self.cols]
        self.srcs = self.ks   # ec: k survivors; xorN: the N others; std: 1
        self.name = kind[0] + "".join(str(i) for i in kind[1:])

    def count(self, part, n):
        """Blocks of a part of a chunk of n blocks (slice_traits.h:311-316);
        a parity part is as long as data part 0."""
        d = self.cols.index(part) if part in self.cols else 0
        return (n + self.ks - d - 1) // self.ks

    def cut(self, chunk):
        """chunk [n, BLOCK] -> the parts, part p as [count(p, n), BLOCK]."""
        n, ks = chunk.shape[0], self.ks
        rows = -(-n // ks)
        grid = np.zeros((rows * ks, BLOCK), np.uint8)
        grid[:n] = chunk
        grid = grid.reshape(rows, ks, BLOCK)
        parts = [None] * self.nparts
        for c, p in enumerate(self.cols):
            parts[p] = chunk[c::ks].copy()
        if self.kind[0] == "xor":
            parts[0] = np.bitwise_xor.reduce(grid, axis=1)
        elif self.kind[0] == "ec":
            par = oracle.rs_encode(
                ks, self.m,
                [np.ascontiguousarray(grid[:, c]).reshape(-1)
                 for c in range(ks)], rows * BLOCK)
            for i, p in enumerate(self.parity):
                parts[p] = par[i].reshape(rows, BLOCK)
        for p in range(self.nparts):
            assert parts[p].shape[0] == self.count(p, n)
        return parts

    def bearable(self, lost):
        return len(lost) <= self.m

    def losses(self):
        """No loss, every single loss and, for m = 2, every double loss."""
        out = [()] + [(p,) for p in range(self.nparts)]
        if self.m == 2:
            out += list(itertools.combinations(range(self.nparts), 2))
        return out if self.m else [()]

    def plan(self, lost):
        """(source parts, col_map, table or None) of a read of a chunk whose
        parts `lost` are gone, every lost data column given a table row in
        ascending order.  With all data parts there: the data parts, copied.
        Otherwise an ec slice reads its first k surviving parts
        (ec_read_plan.h:126-133), a xor slice all the others."""
        lost = sorted(lost)
        lost_cols = [c for c, p in enumerate(self.cols) if p in lost]
        if not lost_cols:
            return list(self.cols), list(range(self.ks)), None
        assert self.bearable(lost)
        srcs = [p for p in range(self.nparts) if p not in lost][:self.ks]
        assert len(srcs) == self.ks
        col_map = [srcs.index(p) if p in srcs else LOST + lost_cols.index(c)
                   for c, p in enumerate(self.cols)]
        if self.kind[0] == "xor":
            tbl = oracle.init_tables(np.ones(self.ks, np.uint8))
        else:
            present = sum(1 << p for p in srcs)
            needed = sum(1 << self.cols[c] for c in lost_cols)
            tbl, ic, oc = oracle.rs_make_tables(self.ks, self.m, present,
                                                present, needed)
            assert (ic, oc) == (self.ks, len(lost_cols))
        return srcs, col_map, np.ascontiguousarray(tbl)


class PartStore:
    """The parts of some chunks in one buffer of random bytes: every part has
    room for `room` blocks at `stride`, of which only its own are the
    part's, so a read past a count returns random bytes.  phase(i) shifts
    the i-th part placed off its 16-byte boundary."""

    def __init__(self, nslots, room, stride=BLOCK, phase=None, seed=0):
        self.stride = stride
        self.slot = (GUARD + 16 + (room - 1) * stride + BLOCK + 15) // 16 * 16
        self.host = np.random.default_rng(seed).integers(
            0, 256, nslots * self.slot, np.uint8)
        self.phase = phase or (lambda i: 0)
        self.used = 0

    def put(self, part):
        """part [count, BLOCK] -> its offset in the buffer."""
        off = self.used * self.slot + GUARD + self.phase(self.used)
        self.used += 1
        for b in range(part.shape[0]):
            at = off + b * self.stride
            self.host[at:at + BLOCK] = part[b]
        assert off + part.shape[0] * self.stride <= self.used * self.slot
        return off


class Reads:
    """The arrays of one call, read by read."""

    def __init__(self, slice_, rows):
        self.sl, self.rows = slice_, rows
        self.src, self.nb, self.cmap = [], [], []
        self.first, self.count, self.index, self.expect = [], [], [], []

    def add(self, src_offs, src_nb, col_map, first, count, expect, index=0):
        """src_offs: offset in the part store per slot, None = address 0;
        expect [count, BLOCK]."""
        assert len(src_offs) == len(src_nb) == self.sl.srcs
        assert len(col_map) == self.sl.ks and expect.shape == (count, BLOCK)
        self.src.append(src_offs)
        self.nb.append(src_nb)
        self.cmap.append(col_map)
        self.first.append(first)
        self.count.append(count)
        self.index.append(index)
        self.expect.append(expect)

    def __len__(self):
        return len(self.first)

    def out_layout(self, stride=BLOCK, phase=None):
        """Offsets of the outputs in an arena of FILL, each between GUARD
        bytes: (offsets, arena size)."""
        offs, at = [], 0
        for i, c in enumerate(self.count):
            offs.append(at + GUARD + (phase(i) if phase else 0))
            at += (GUARD + 16 + (c - 1) * stride + BLOCK + GUARD + 15) \
                // 16 * 16
        return offs, at

    def expected_arena(self, offs, size, stride=BLOCK):
        want = np.full(size, FILL, np.uint8)
        for off, exp in zip(offs, self.expect):
            for i in range(exp.shape[0]):
                want[off + i * stride:off + i * stride + BLOCK] = exp[i]
        return want

    def arrays(self, src_base, dst_base, out_offs):
        """(src_ptrs, src_nb, col_map, first, count, dst_ptrs, index)."""
        sp = np.array([[0 if o is None else src_base + o for o in row]
                       for row in self.src], np.uint64)
        dp = np.array([dst_base + o for o in out_offs], np.uint64)
        return (sp, np.array(self.nb, np.uint32),
                np.array(self.cmap, np.uint8),
                np.array(self.first, np.uint32),
                np.array(self.count, np.uint32), dp,
                np.array(self.index, np.uint32))


def chunk_blocks(chunk, first, count):
    """Blocks [first, first + count) of a chunk, zeros from its end on."""
    out = np.zeros((count, BLOCK), np.uint8)
    have = max(0, min(chunk.shape[0], first + count) - first)
    out[:have] = chunk[first:first + have]
    return out
