"""Shared by test_chunk_write_degraded_host.py and
test_gpu_chunk_write_degraded.py: writes into chunks of a slice with lost
parts, the arguments of one lizec_chunk_write_degraded call, and the bytes it
has to produce.

The expected bytes take the reference's route (ChunkWriter::fillStripe over
readBlocks, chunk_writer.cc:440-466, :557-615) through the oracle: the old
parity parts come from oracle.rs_encode (XOR for a xor slice) over the old
chunk, [from, to) of every LOST column of a row comes from oracle.rs_recover
(XOR) over the old bytes of the first k available parts, the row's parity
from chunk_write_cases.parity_of over new, fill and rebuilt columns, and the
CRCs from oracle.crc32.

Parts are numbered as lizec_degraded_write_table numbers them: data parts
0..ks-1 in column order, then the parity parts.  A call has one old-source
slot per part of the slice, slot j = part j.  The slot of a LOST part points
at a decoy of random bytes, with the part's block count: a call that read it
would produce other bytes.
"""
import ctypes

import numpy as np

import chunk_write_cases as C
import oracle
from chunk_read_cases import BLOCK, FILL, GUARD, PartStore

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

LIZEC_OK = 0
LIZEC_EINVAL = -2

SLICES = {s.name: s for s in
          [C.Slice("xor", 3), C.Slice("ec", 2, 1), C.Slice("ec", 3, 2),
           C.Slice("ec", 5, 2), C.Slice("ec", 2, 9)] +
          [C.FirstRows(8, 7, r) for r in range(3, 8)]}

PATTERNS = ("healthy", "fill-first", "fill-last", "new-only", "m-data",
            "data+parity")
assert sorted(SLICES) == sorted(["xor3", "ec21", "ec32", "ec52", "ec29"] +
                                [f"ec87-rows{r}" for r in range(3, 8)])
assert [s.m for s in SLICES.values()] == [1, 1, 2, 2, 9, 3, 4, 5, 6, 7]


class Layout:
    """The layouts of test_gpu_chunk_write.py."""

    def __init__(self, name, stride, phase, data_phase, packed, in_place,
                 par_phases=(0, 0, 0)):
        self.name, self.stride, self.phase = name, stride, phase
        self.data_phase, self.packed = data_phase, packed
        self.in_place, self.par_phases = in_place, par_phases

    def data_stride(self, size):
        return size if self.packed else (size + 15) // 16 * 16

    def par_phase(self, i, r, r0, frm):
        if self.in_place:
            return self.phase + r0 * self.stride + frm
        return self.par_phases[(i + r) % 3]

    def par_stride(self, size):
        return self.stride if self.in_place else size


LAYOUTS = {l.name: l for l in (
    Layout("fast", 65536, 0, (0, 0, 0), False, True),
    Layout("il", 65540, 4, (0, 0, 0), True, True),
    Layout("data4", 65536, 0, (4, 8, 12), True, False),
    Layout("odd", 65536, 0, (1, 7, 13), True, False, (13, 1, 7)))}


def the_writes(ks, aligned):
    """(chunk blocks, first, count, from, to) of the seven writes of
    test_gpu_chunk_write.py, and an eighth: a whole row and the first block
    of the next, whose other columns are FILL in the last row only (none of
    the seven has such a column)."""
    n = 2 * ks + 1
    if aligned:
        r3, r4, r5, r6 = (16, 65536), (4096, 4096 + 8240), (65520, 65536), \
            (4096, 4096 + 20528)
    else:
        r3, r4, r5, r6 = (13, 65536), (4093, 4093 + 8195), (65535, 65536), \
            (13, 13 + 20485)
    return [(n, ks + 1, 1, 0, 65536),
            (n, 1, 2 * ks, 0, 65536),
            (n, 0, 2 * ks, 0, 65536),
            (2 * ks - 1, ks, 1) + r3,
            (ks + 1, 2 * ks - 1, 2) + r4,
            (n, 1, 1) + r5,
            (n, ks - 1, ks + 1) + r6,
            (n, 0, ks + 1) + r4]


def is_xor(sl):
    return sl.kind[0] == "xor"


def full_m(sl):
    return getattr(sl, "full_m", sl.m)


def build_table(sl, new_mask, have_mask, avail_mask, slot_part):
    """lizec_degraded_write_table -> (rc, table [m * (ks + srcs) * 32] cut
    to the call's rows, use mask)."""
    from lizardfs_amd import lib as L
    slot_part = np.asarray(slot_part, np.uint8)
    srcs = len(slot_part)
    tbl = np.zeros(32 * (sl.ks + srcs) * full_m(sl), np.uint8)
    mask = ctypes.c_uint32(0xFFFFFFFF)
    rc = L.lib().lizec_degraded_write_table(
        sl.ks, full_m(sl), int(is_xor(sl)), new_mask, have_mask, avail_mask,
        slot_part.ctypes.data_as(u8p), srcs, tbl.ctypes.data_as(u8p),
        ctypes.byref(mask))
    return rc, tbl[:32 * (sl.ks + srcs) * sl.m], mask.value


def survivors(sl, avail):
    """The first k available parts, ascending (ec_read_plan.h:126-133); for
    a xor slice all the others."""
    return sorted(avail)[:sl.ks]


def rebuild(sl, avail, lost_col, old, size):
    """[size] bytes of data column lost_col out of old[p], the same bytes of
    every part p (None = zeros), through the oracle."""
    srcs = survivors(sl, avail)
    assert len(srcs) == sl.ks
    zeros = np.zeros(size, np.uint8)
    got = [zeros if old[p] is None else np.ascontiguousarray(old[p])
           for p in srcs]
    if is_xor(sl):
        return np.bitwise_xor.reduce(got, axis=0)
    m = full_m(sl)
    frags = [None] * (sl.ks + m)
    for p, a in zip(srcs, got):
        frags[p] = a
    erased = sum(1 << p for p in range(sl.ks + m) if p not in srcs)
    return oracle.rs_recover(sl.ks, m, frags, erased, {lost_col},
                             size)[lost_col]


class Chunk:
    """A chunk of n blocks of a slice with ALL its parts as they are now,
    data and parity, each in a PartStore; chunk_write_cases.Chunk's fields,
    so that chunk_write_cases.Writes takes it."""

    def __init__(self, sl, n, store, seed):
        self.sl, self.n = sl, n
        rng = np.random.default_rng(seed)
        self.blocks = rng.integers(0, 256, (n, BLOCK), np.uint8)
        ks = sl.ks
        rows = -(-n // ks)
        grid = np.zeros((rows * ks, BLOCK), np.uint8)
        grid[:n] = self.blocks
        grid = grid.reshape(rows, ks, BLOCK)
        self.parts = [self.blocks[c::ks] for c in range(ks)]
        par = C.parity_of(sl, [np.ascontiguousarray(grid[:, c]).reshape(-1)
                               for c in range(ks)], rows * BLOCK)
        self.old = self.parts + [p.reshape(rows, BLOCK) for p in par]
        self.nb = [p.shape[0] for p in self.parts]
        self.old_nb = [p.shape[0] for p in self.old]
        self.old_offs = [store.put(p) if p.shape[0] else None
                         for p in self.old]
        self.offs = self.old_offs[:ks]
        # what a slot of a lost part points at: random bytes of the store
        self.decoy = store.put(np.zeros((0, BLOCK), np.uint8))
        self.memo = {}


def row_kinds(sl, chunk_nb, first, count, b):
    out = []
    for c in range(sl.ks):
        if first <= b * sl.ks + c < first + count:
            out.append("new")
        elif b < chunk_nb[c]:
            out.append("fill")
        else:
            out.append("absent")
    return out


def lost_parts(sl, pattern, chunk_nb, first, count):
    """The lost parts of a pattern for one write, or None where the write
    has no column of the kind the pattern asks for (or the slice too few
    parities).  Parity r is part ks + r."""
    ks = sl.ks
    r0, r1 = first // ks, (first + count - 1) // ks
    rows = [row_kinds(sl, chunk_nb, first, count, b)
            for b in range(r0, r1 + 1)]
    fill_first = [c for c in range(ks) if rows[0][c] == "fill"]
    fill_last = [c for c in range(ks) if rows[-1][c] == "fill" and
                 c not in fill_first] if r1 > r0 else []
    new_only = [c for c in range(ks)
                if all(r[c] != "fill" for r in rows) and
                any(r[c] == "new" for r in rows)]
    if pattern == "healthy":
        return []
    if pattern == "fill-first":
        return fill_first[:1] or None
    if pattern == "fill-last":
        return fill_last[:1] or None
    if pattern == "new-only":
        if not new_only:
            return None
        # with a second parity, one is lost as well: m - 1 wanted
        return new_only[:1] + ([ks] if sl.m >= 2 else [])
    if sl.m < 2:
        return None
    if pattern == "m-data":
        order = fill_first + fill_last + \
            [c for c in range(ks) if c not in fill_first + fill_last]
        return sorted(order[:min(sl.m, ks)])
    assert pattern == "data+parity"
    return (fill_first + fill_last + [0])[:1] + [ks]


class Case:
    """Some writes of a slice in a layout, each into a chunk of its own:
    the part store, the data buffer, and per availability pattern the
    tables, the arena and what it has to hold.  Host memory only."""

    def __init__(self, sl, lay, specs, seed=1):
        self.sl, self.lay, self.specs = sl, lay, specs
        self.nparts = sl.ks + sl.m
        self.store = PartStore((self.nparts + 1) * len(specs), 4, lay.stride,
                               lambda i: lay.phase, seed=seed)
        rng = np.random.default_rng(seed + 1)
        at, where = 0, []
        for i, (n, first, count, frm, to) in enumerate(specs):
            ds = lay.data_stride(to - frm)
            where.append((at + GUARD + lay.data_phase[i % 3], ds))
            at += (GUARD + 16 + count * ds + 15) // 16 * 16
        self.data = rng.integers(0, 256, at + GUARD, np.uint8)
        self.writes = C.Writes(sl)
        for i, (n, first, count, frm, to) in enumerate(specs):
            chunk = Chunk(sl, n, self.store, seed + 10 + i)
            self.writes.add(chunk, first, count, frm, to, self.data,
                            where[i][0], where[i][1])

    def set_lost(self, lost, crcs=True, want=None):
        """lost: per write, the lost parts.  Sets the wanted parities to the
        available ones (or `want` of them), computes the rows with LOST
        columns by the reference's route, lays the arena out; returns False
        if a write cannot be made."""
        sl = self.sl
        self.avail = []
        for w, gone in zip(self.writes.w, lost):
            avail = [p for p in range(self.nparts) if p not in gone]
            self.avail.append(avail)
            w["want"] = [r for r in range(sl.m) if sl.ks + r in avail and
                         (want is None or r in want)]
            w["crcs"] = crcs
            chunk, frm, to = w["chunk"], w["frm"], w["to"]
            for i in range(w["touched"]):
                b = w["r0"] + i
                kinds = row_kinds(sl, chunk.nb, w["first"], w["count"], b)
                gone_cols = [c for c in range(sl.ks)
                             if kinds[c] == "fill" and c in gone]
                if not gone_cols:
                    continue
                if len(avail) < sl.ks:
                    return False
                old = [chunk.old[p][b, frm:to] if b < chunk.old_nb[p]
                       else None for p in range(self.nparts)]
                cols = []
                for c in range(sl.ks):
                    if kinds[c] == "new":
                        at = w["data_off"] + (b * sl.ks + c - w["first"]) * \
                            w["data_stride"]
                        cols.append(self.data[at:at + w["size"]])
                    elif c in gone_cols:
                        cols.append(rebuild(sl, avail, c, old, w["size"]))
                    elif kinds[c] == "fill":
                        cols.append(old[c])
                    else:
                        cols.append(None)
                p = C.parity_of(sl, cols, w["size"])
                # the reference's route has to give the arrays that
                # chunk_write_cases.Writes computed from the part itself;
                # those stay (their CRCs are memoised by identity)
                for r in range(sl.m):
                    assert np.array_equal(p[r], w["par"][i, r])
        self.size, self.want = self.writes.layout(self.lay.par_phase,
                                                  self.lay.par_stride)
        self._tables()
        return True

    def set_pattern(self, pattern):
        """Every write takes the pattern where it has the columns for it and
        stays healthy otherwise; returns how many took it.  Of the eight
        writes of the_writes at least one takes every pattern the slice has
        parities for."""
        lost, took = [], 0
        for w in self.writes.w:
            gone = lost_parts(self.sl, pattern, w["chunk"].nb, w["first"],
                              w["count"])
            took += gone is not None
            lost.append(gone or [])
        assert self.set_lost(lost)
        if len(self.specs) == 8:
            assert took >= 1 or (self.sl.m < 2 and
                                 pattern in ("m-data", "data+parity"))
        return took

    def _tables(self):
        sl = self.sl
        keys, self.tables, masks = {}, [], []
        self.index = np.zeros((len(self.writes), 3), np.uint32)
        for i, w in enumerate(self.writes.w):
            avail = sum(1 << p for p in self.avail[i])
            r0, r1 = w["r0"], w["r0"] + w["touched"] - 1
            for t, b in enumerate((r0, (r0 + r1) // 2, r1)):
                kinds = row_kinds(sl, w["chunk"].nb, w["first"], w["count"],
                                  b)
                new = sum(1 << c for c in range(sl.ks) if kinds[c] == "new")
                have = sum(1 << c for c in range(sl.ks)
                           if b < w["chunk"].nb[c])
                key = (new, have, avail)
                if key not in keys:
                    rc, tbl, mask = build_table(sl, new, have, avail,
                                                range(self.nparts))
                    assert rc == LIZEC_OK, (rc, key)
                    keys[key] = len(self.tables)
                    self.tables.append(tbl)
                    masks.append(mask)
                self.index[i, t] = keys[key]
        self.masks = np.array(masks, np.uint32)
        self.tbl = np.concatenate(self.tables)

    def drop_a_mask_bit(self):
        """After set_pattern("healthy"): every table loses the lowest bit of
        its mask, so the fill column behind that slot counts as zeros
        although its table column is not zero: a call that obeys the mask
        gives other bytes than one that reads whatever has a coefficient.
        Recomputes the expectation; the case serves nothing else after."""
        sl = self.sl
        dropped = {}
        for t, m in enumerate(self.masks):
            if m:
                dropped[t] = (int(m) & -int(m)).bit_length() - 1
                self.masks[t] = int(m) & ~(1 << dropped[t])
        for i, w in enumerate(self.writes.w):
            chunk = w["chunk"]
            for j in range(w["touched"]):
                t = self.index[i, 0 if j == 0 else
                               2 if j == w["touched"] - 1 else 1]
                if t not in dropped:
                    continue
                b = w["r0"] + j
                kinds = row_kinds(sl, chunk.nb, w["first"], w["count"], b)
                assert kinds[dropped[t]] == "fill"
                cols = []
                for c in range(sl.ks):
                    if kinds[c] == "new":
                        at = w["data_off"] + (b * sl.ks + c - w["first"]) * \
                            w["data_stride"]
                        cols.append(self.data[at:at + w["size"]])
                    elif kinds[c] == "fill" and c != dropped[t]:
                        cols.append(chunk.parts[c][b, w["frm"]:w["to"]])
                    else:
                        cols.append(None)
                par = C.parity_of(sl, cols, w["size"])
                chunk.memo["dropped", j] = par   # keeps the arrays alive
                for r in range(sl.m):
                    w["par"][j, r] = par[r]
        self.size, self.want = self.writes.layout(self.lay.par_phase,
                                                  self.lay.par_stride)
        return len(dropped)

    def used_slots(self, i):
        """The slots in a mask of write i's tables."""
        m = 0
        for t in self.index[i]:
            m |= int(self.masks[t])
        return m

    def arrays(self, store_base, data_base, arena_base, spare="decoy"):
        """(writes, old_ptrs, old_nb, par_ptrs).  A slot of a lost part, and
        with spare = "zero" every slot outside the write's masks, does not
        point at the part: at the decoy with the part's count ("decoy",
        "swap": every slot outside the masks as well), nowhere with count 0
        ("zero"), or nowhere with the part's count ("null": such a slot is
        never addressed, so the call takes it)."""
        wr, _, _, pp = self.writes.arrays(store_base, data_base, arena_base)
        W = len(self.writes)
        op = np.zeros((W, self.nparts), np.uint64)
        on = np.zeros((W, self.nparts), np.uint32)
        for i, w in enumerate(self.writes.w):
            chunk, used = w["chunk"], self.used_slots(i)
            for p in range(self.nparts):
                if not chunk.old_nb[p]:
                    continue
                real = p in self.avail[i]
                if spare == "zero" and not (used >> p) & 1:
                    continue
                if spare == "swap" and not (used >> p) & 1:
                    real = False
                on[i, p] = chunk.old_nb[p]
                if spare == "null" and not (used >> p) & 1:
                    continue
                op[i, p] = store_base + (chunk.old_offs[p] if real
                                         else chunk.decoy)
        return wr, op, on, pp

    def call_args(self, wr, op, on, pp):
        """The arguments of either entry point behind the engine."""
        return (self.sl.m, self.tbl.ctypes.data_as(u8p), len(self.masks),
                self.masks.ctypes.data_as(u32p),
                self.index.ctypes.data_as(u32p),
                ctypes.c_void_p(wr.ctypes.data), len(wr),
                op.ctypes.data_as(u64p), on.ctypes.data_as(u32p),
                self.nparts, self.sl.ks, self.lay.stride,
                pp.ctypes.data_as(u64p))

    def run_host(self, spare="decoy"):
        """-> (rc, arena) through lizec_chunk_write_degraded_host."""
        from lizardfs_amd import lib as L
        arena = np.full(self.size, FILL, np.uint8)
        store = self.store.host.copy()
        data = self.data.copy()
        arrs = self.arrays(store.ctypes.data, data.ctypes.data,
                           arena.ctypes.data, spare)
        rc = L.lib().lizec_chunk_write_degraded_host(*self.call_args(*arrs))
        assert np.array_equal(store, self.store.host)
        assert np.array_equal(data, self.data)
        return rc, arena

    def check(self, arena):
        bad = np.flatnonzero(arena != self.want)
        assert bad.size == 0, (self.sl.name, self.lay.name, bad.size,
                               int(bad[0]))
