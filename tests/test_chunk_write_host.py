"""lizec_chunk_write_host and chunkwrite.write_chunks_host: the client write
on the CPU, bit-exact against the rule of lizec.h put together with numpy
and the oracle (chunk_write_cases.py).  No GPU is needed.

test_every_range makes, for every slice, every chunk length n = 1..2k+1 and
every byte range of SIZES, ONE call that holds every block range inside
[0, 2k+2): writes inside the chunk, writes that extend it and writes wholly
past its end.  The new bytes of chunk block c are the same in every write
(block c of one pool of random bytes, the write's data address pointing into
it at c * 65536 + from), so nothing is copied and the data addresses take
every phase that `from` gives them.  All parity outputs and CRC arrays of a
call lie in one arena of 0xA5, each between 256-byte canaries, at odd
phases, packet-compact (par_stride = size); the whole arena is compared.
The same writes then go through chunkwrite.write_chunks_host, one call per
first block.

test_write_gate_read_loop closes the loop for every packet list of the same
matrix for xor2, xor3, ec(2,1) and ec(3,2), in both on-disk formats;
test_write_gate_read_loop_ec82 for 5 chunk lengths and 51 block ranges of
ec(8,2) at every byte range.
"""
import ctypes
import struct

import numpy as np
import pytest

import chunk_write_cases as C
import oracle
from lizardfs_amd import chunkread, chunkwrite, scrub, writegate
from lizardfs_amd import lib as L
from lizardfs_amd import slice_traits as st

LIZEC_OK = 0
LIZEC_EINVAL = -2
BLOCK = C.BLOCK
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

SLICES = [C.Slice("xor", 2), C.Slice("xor", 3), C.Slice("ec", 2, 1),
          C.Slice("ec", 3, 2), C.Slice("ec", 8, 2)]
SIZES = [(0, 65536), (0, 1), (65535, 65536), (1, 17), (13, 65536),
         (4093, 4093 + 8192 + 3)]
PHASES = (1, 7, 13)


def slice_type(sl):
    if sl.kind[0] == "xor":
        return st.K_XOR2 + sl.ks - 2
    return st.ec_slice_type(sl.ks, sl.m)


def call_host(sl, tbl, wr, fp, fn, pp, stride, rows=None, ks=None,
              num=None):
    """Arguments as numpy arrays or None (= NULL)."""
    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    return L.lib().lizec_chunk_write_host(
        sl.m if rows is None else rows, ptr(tbl, u8p),
        None if wr is None else ctypes.c_void_p(wr.ctypes.data),
        len(wr) if num is None else num, ptr(fp, u64p), ptr(fn, u32p),
        sl.ks if ks is None else ks, stride, ptr(pp, u64p))


class Setup:
    """A chunk of n blocks in a part store, and the pool of new bytes."""

    def __init__(self, sl, n, stride=BLOCK, phase=None, seed=0):
        self.sl = sl
        self.store = C.PartStore(sl.ks, 4, stride, phase, seed=seed + 1)
        self.chunk = C.Chunk(sl, n, self.store, seed + 2)
        self.limit = 2 * sl.ks + 2
        self.pool = np.random.default_rng(seed + 3).integers(
            0, 256, self.limit * BLOCK, np.uint8)
        self.before = self.store.host.copy(), self.pool.copy()

    def add(self, writes, first, count, frm, to, **kw):
        writes.add(self.chunk, first, count, frm, to, self.pool,
                   first * BLOCK + frm, BLOCK, **kw)

    def run(self, writes, tbl, stride=None):
        size, want = writes.layout(
            lambda i, r, r0, frm: PHASES[(i + r) % 3], lambda s: s)
        arena = np.full(size, C.FILL, np.uint8)
        wr, fp, fn, pp = writes.arrays(self.store.host.ctypes.data,
                                       self.pool.ctypes.data,
                                       arena.ctypes.data)
        rc = call_host(self.sl, tbl, wr, fp, fn, pp,
                       stride or self.store.stride)
        return rc, arena, want

    def check_write_chunks_host(self, writes, frm, to):
        """The same writes (every block range, in C.block_ranges order, at
        one byte range) through chunkwrite.write_chunks_host: one call per
        first block, a batch of one write per count.  The batch's chunks are
        all this chunk and its data rows all start at the pool's block
        `first`, so both are passed as views of stride 0.  Parity, CRCs and
        packets against what layout() expects."""
        sl, t, size = self.sl, slice_type(self.sl), to - frm
        pool = self.pool.reshape(self.limit, BLOCK)
        at = 0
        for first in range(self.limit):
            S = self.limit - first
            frags = [None] * sl.nparts
            for c, part in enumerate(self.chunk.parts):
                if part.shape[0]:
                    flat = np.ascontiguousarray(part).reshape(-1)
                    frags[sl.cols[c]] = np.broadcast_to(flat, (S, flat.size))
            data = np.broadcast_to(pool[first:, frm:to], (S, S, size))
            counts = np.arange(1, S + 1)
            parity, crcs, packets = chunkwrite.write_chunks_host(
                t, frags, [self.chunk.n] * S, data, first, counts, frm, size)
            for s in range(S):
                w = writes.w[at + s]
                assert (w["first"], w["count"]) == (first, s + 1)
                for (i, r), exp in w["par"].items():
                    assert np.array_equal(parity[s, i, r], exp)
                assert list(crcs[s, :s + 1]) == w["crc"]
                plan = chunkwrite.plan_write(t, self.chunk.n, first, s + 1)
                assert [(p.part, p.block) for p in packets[s]] == plan.packets
                for p in packets[s]:
                    assert (p.offset, p.size) == (frm, size)
                    if p.part in sl.cols:
                        i = p.block * sl.ks + sl.cols.index(p.part) - first
                        assert p.crc == w["crc"][i]
                        assert p.data.ctypes.data == data[s, i].ctypes.data
                    else:
                        exp = w["par"][p.block - w["r0"],
                                       sl.parity.index(p.part)]
                        assert p.crc == self.chunk.memo["crc", id(exp)]
                        assert np.array_equal(p.data, exp)
            at += S
        assert at == len(writes)

    def sources_intact(self):
        return np.array_equal(self.store.host, self.before[0]) and \
            np.array_equal(self.pool, self.before[1])


@pytest.mark.parametrize("sl", SLICES, ids=lambda s: s.name)
def test_every_range(sl):
    tbl = C.encode_table(sl)
    for n in range(1, 2 * sl.ks + 2):
        su = Setup(sl, n, seed=10 * n)
        for frm, to in SIZES:
            writes = C.Writes(sl)
            for first, count in C.block_ranges(su.limit):
                su.add(writes, first, count, frm, to)
            rc, arena, want = su.run(writes, tbl)
            assert rc == LIZEC_OK
            bad = np.flatnonzero(arena != want)
            assert bad.size == 0, (n, frm, to, int(bad[0]))
            su.check_write_chunks_host(writes, frm, to)
        assert su.sources_intact()


@pytest.mark.parametrize("sl", SLICES, ids=lambda s: s.name)
def test_unwanted_parity_no_crcs_and_whole_rows(sl):
    """One parity unwanted (address 0: its bytes and CRC slots stay 0xA5), a
    write without a CRC array, and whole rows with every fill count 0; at
    the INTERLEAVED stride with the parts 4 past a 16-byte boundary."""
    tbl = C.encode_table(sl)
    ks = sl.ks
    su = Setup(sl, 2 * ks + 1, stride=65540, phase=lambda i: 4, seed=77)
    for frm, to in SIZES:
        writes = C.Writes(sl)
        su.add(writes, 1, ks + 1, frm, to, want=list(range(1, sl.m)))
        su.add(writes, ks + 1, 1, frm, to, crcs=False)
        su.add(writes, 0, 2 * ks, frm, to, fill=False)
        if sl.m > 1:
            su.add(writes, 2, 2 * ks, frm, to, want=[0], crcs=False)
        rc, arena, want = su.run(writes, tbl)
        assert rc == LIZEC_OK
        assert np.array_equal(arena, want), (frm, to)
    assert su.sources_intact()


def test_refusals_write_nothing():
    sl = C.Slice("ec", 3, 2)
    tbl = C.encode_table(sl)
    su = Setup(sl, 7, seed=5)
    writes = C.Writes(sl)
    su.add(writes, 1, 5, 13, 4000)
    su.add(writes, 4, 1, 0, 65536)
    size, want = writes.layout(lambda i, r, r0, frm: 0, lambda s: s)
    arena = np.full(size, C.FILL, np.uint8)
    good = writes.arrays(su.store.host.ctypes.data, su.pool.ctypes.data,
                         arena.ctypes.data)

    def refused(edit=None, **kw):
        wr, fp, fn, pp = (a.copy() for a in good)
        args = dict(wr=wr, fp=fp, fn=fn, pp=pp, tbl=tbl)
        if edit:
            edit(args)
        rc = call_host(sl, args["tbl"], args["wr"], args["fp"], args["fn"],
                       args["pp"], kw.pop("stride", BLOCK), **kw)
        assert rc == LIZEC_EINVAL
        assert (arena == C.FILL).all() and su.sources_intact()

    def field(i, name, value):
        def edit(a):
            a["wr"][name][i] = value
        return edit

    for name in ("tbl", "wr", "fp", "fn", "pp"):
        refused(lambda a, name=name: a.__setitem__(name, None),
                num=2)                                   # a NULL array
    refused(num=0)
    refused(rows=0)
    refused(rows=33)
    refused(ks=0)
    refused(ks=33)
    refused(field(0, "from", 4000))                      # from == to
    refused(field(0, "from", 4001))
    refused(field(1, "to", 65537))
    refused(field(0, "block_count", 0))
    refused(field(0, "first_block", 1048576 - 4))        # end past 2^20
    refused(field(1, "data", 0))
    refused(field(0, "data_stride", 3986))               # used, below size
    refused(field(0, "par_stride", 3986))
    refused(stride=65535)
    refused(lambda a: a["fn"].__setitem__((0, 1), 32769))
    refused(lambda a: a["fp"].__setitem__((1, 2), 0))    # count without address
    refused(field(0, "crcs", int(good[0]["crcs"][0]) + 2))
    refused(lambda a: (a["pp"].__setitem__((1, slice(None)), 0),
                       field(1, "crcs", 0)(a)))          # nothing to do

    # strides that are not used may hold anything
    wr, fp, fn, pp = (a.copy() for a in good)
    wr["data_stride"][1] = 0
    wr["par_stride"][1] = 0
    assert call_host(sl, tbl, wr, fp, fn, pp, BLOCK) == LIZEC_OK
    assert np.array_equal(arena, want)


def test_more_than_the_grid_is_refused():
    """4096 writes of 2^20 blocks of 8 KiB into ec(2,1) touch 2^19 rows
    each, one tile a row: 2^31 workgroups.  Refused on the host before any
    address is used."""
    sl = C.Slice("ec", 2, 1)
    W = 4096
    wr = np.zeros(W, C.WRITE_DTYPE)
    wr["data"], wr["crcs"] = 4096, 0
    wr["data_stride"] = wr["par_stride"] = 8192
    wr["first_block"], wr["block_count"] = 0, 1048576
    wr["from"], wr["to"] = 0, 8192
    fp = np.zeros((W, 2), np.uint64)
    fn = np.zeros((W, 2), np.uint32)
    pp = np.full((W, 1), 4096, np.uint64)
    assert call_host(sl, C.encode_table(sl), wr, fp, fn, pp,
                     BLOCK) == LIZEC_EINVAL


def test_more_crcs_than_the_ranges_kernel_takes_are_refused():
    """16385 writes of 1024 one-byte blocks with a CRC array: more than 2^24
    CRCs.  One write fewer passes the check function."""
    sl = C.Slice("ec", 2, 1)
    W = 16385
    wr = np.zeros(W, C.WRITE_DTYPE)
    wr["data"], wr["crcs"] = 4096, 4096
    wr["data_stride"] = wr["par_stride"] = 1
    wr["first_block"], wr["block_count"] = 0, 1024
    wr["from"], wr["to"] = 0, 1
    fp = np.zeros((W, 2), np.uint64)
    fn = np.zeros((W, 2), np.uint32)
    pp = np.zeros((W, 1), np.uint64)      # no parity wanted: 1024 CRCs each
    tbl = C.encode_table(sl)
    assert call_host(sl, tbl, wr, fp, fn, pp, BLOCK) == LIZEC_EINVAL
    assert check_only(sl.m, tbl, wr[:W - 1], fp, fn, sl.ks, pp) == \
        (W - 1) * 512


def check_only(rows, tbl, wr, fp, fn, ks, pp):
    """lizec_impl_chunk_write_check, the check function of both calls: the
    touched rows or LIZEC_EINVAL; it uses no address."""
    fn_ = L.lib().lizec_impl_chunk_write_check
    fn_.restype = ctypes.c_int64
    return fn_(ctypes.c_int(rows), tbl.ctypes.data_as(u8p),
               ctypes.c_void_p(wr.ctypes.data), ctypes.c_int(len(wr)),
               fp.ctypes.data_as(u64p), fn.ctypes.data_as(u32p),
               ctypes.c_int(ks), ctypes.c_uint32(BLOCK),
               pp.ctypes.data_as(u64p), None, None, None, None)


def test_the_grid_bound_is_that_of_the_passes_launched():
    """2048 writes of 2^20 blocks of 16 KiB into a slice of 2 data parts
    touch 2^30 rows: 2^30 tiles of 16 KiB, 2^31 of 8 KiB.  A call of up to 4
    parities launches the first and is taken; from 5 parities on a pass cuts
    8 KiB tiles and the call is refused; so is one of 9..12 parities, which
    launches both."""
    W = 2048
    wr = np.zeros(W, C.WRITE_DTYPE)
    wr["data"] = 4096
    wr["data_stride"] = wr["par_stride"] = 16384
    wr["first_block"], wr["block_count"] = 0, 1048576
    wr["from"], wr["to"] = 0, 16384
    fp = np.zeros((W, 2), np.uint64)
    fn = np.zeros((W, 2), np.uint32)
    tbl = np.zeros(32 * 2 * 12, np.uint8)
    for rows, want in ((1, W << 19), (4, W << 19), (5, LIZEC_EINVAL),
                       (8, LIZEC_EINVAL), (9, LIZEC_EINVAL)):
        pp = np.full((W, rows), 4096, np.uint64)
        assert check_only(rows, tbl, wr, fp, fn, 2, pp) == want, rows


def test_plan_write_by_rule():
    for sl in SLICES:
        t = slice_type(sl)
        ks = sl.ks
        for n in range(0, 2 * ks + 2):
            have = [len(range(c, n, ks)) for c in range(ks)]
            for first, count in C.block_ranges(2 * ks + 2):
                plan = chunkwrite.plan_write(t, n, first, count)
                end = first + count
                rows = list(range(first // ks, (end - 1) // ks + 1))
                assert [b for b, _ in plan.rows] == rows
                read = set()
                for b, kinds in plan.rows:
                    for c in range(ks):
                        if first <= b * ks + c < end:
                            assert kinds[c] == chunkwrite.NEW
                        elif b < have[c]:
                            assert kinds[c] == chunkwrite.FILL
                            read.add(sl.cols[c])
                        else:
                            assert kinds[c] == chunkwrite.ABSENT
                assert plan.read_parts == sorted(read)
                want = [(sl.cols[c], cb // ks) for c in range(ks)
                        for cb in range(first, end) if cb % ks == c]
                want += [(p, b) for p in sl.parity for b in rows]
                assert plan.packets == want


def test_plan_write_by_hand():
    t = st.ec_slice_type(3, 2)
    # a chunk of 5 blocks: parts of 2, 2, 1; blocks 4..7 written
    plan = chunkwrite.plan_write(t, 5, 4, 4)
    assert plan.rows == [(1, ["fill", "new", "new"]),
                         (2, ["new", "new", "absent"])]
    assert plan.read_parts == [0]
    assert plan.packets == [(0, 2), (1, 1), (1, 2), (2, 1), (3, 1), (3, 2),
                            (4, 1), (4, 2)]
    # xor3 keeps its parity at part 0; it is sent last
    plan = chunkwrite.plan_write(st.K_XOR2 + 1, 9, 4, 1)
    assert plan.rows == [(1, ["fill", "new", "fill"])]
    assert plan.read_parts == [1, 3]
    assert plan.packets == [(2, 1), (0, 1)]
    with pytest.raises(ValueError):
        chunkwrite.plan_write(st.K_STANDARD, 5, 0, 1)
    with pytest.raises(ValueError):
        chunkwrite.plan_write(t, 5, 0, 0)
    with pytest.raises(ValueError):
        chunkwrite.plan_write(t, 5, 1020, 5)


# ---- write_chunks_host, and the loop through gate, images and read ----

def zero_crc():
    return oracle.crc32(bytes(BLOCK))


def grow(img, fmt, t, nblocks):
    """The image with room for nblocks blocks, the new ones zeros with the
    CRC of zeros."""
    data_off, crc_off, bstride, cstride = scrub.image_layout(fmt, t)
    have = writegate.image_blocks(img, fmt, t)
    if nblocks <= have:
        return img
    size = nblocks * bstride if fmt == "interleaved" else \
        data_off + nblocks * bstride
    out = np.zeros(size, np.uint8)
    out[:img.size] = img
    for b in range(have, nblocks):
        out[crc_off + b * cstride:crc_off + b * cstride + 4] = \
            np.frombuffer(struct.pack(">I", zero_crc()), np.uint8)
    return out


def host_scrub(img, fmt, t):
    data_off, crc_off, bstride, cstride = scrub.image_layout(fmt, t)
    for b in range(writegate.image_blocks(img, fmt, t)):
        blk = img[data_off + b * bstride:data_off + b * bstride + BLOCK]
        stored = struct.unpack(
            ">I", bytes(img[crc_off + b * cstride:crc_off + b * cstride + 4]))
        if stored[0] != oracle.crc32(blk):
            return b
    return None


def images_of(sl, t, chunk, fmt):
    parts = sl.cut(chunk)
    return [scrub.build_chunk_image(7, 1, t, p, list(parts[p]),
                                    crc32_fn=oracle.crc32, fmt=fmt)
            for p in range(sl.nparts)]


_chunks = {}


def chunk_and_images(sl, fmt, n):
    """A chunk of n blocks and its part images, built once per (slice,
    format, length); the caller gets copies of the images."""
    key = (sl.name, fmt, n)
    if key not in _chunks:
        chunk = np.random.default_rng(1000 + n).integers(
            0, 256, (n, BLOCK), np.uint8)
        _chunks[key] = chunk, images_of(sl, slice_type(sl), chunk, fmt)
    chunk, images = _chunks[key]
    return chunk, [img.copy() for img in images]


def write_and_close_the_loop(sl, fmt, n, first, count, frm, to, rng,
                             want_parity=None):
    t = slice_type(sl)
    ks = sl.ks
    chunk, images = chunk_and_images(sl, fmt, n)
    data = rng.integers(0, 256, (1, count, to - frm), np.uint8)
    frags = [img[None, :] for img in images]
    parity, crcs, packets = chunkwrite.write_chunks_host(
        t, frags, [n], data, first, count, frm, to - frm, fmt=fmt,
        want_parity=want_parity)
    (packets,) = packets
    plan = chunkwrite.plan_write(t, n, first, count)
    wanted = [sl.parity[r] for r in
              (range(sl.m) if want_parity is None else want_parity)]
    assert [(p.part, p.block) for p in packets] == \
        [pb for pb in plan.packets if pb[0] in sl.cols or pb[0] in wanted]
    for p in packets:
        assert (p.offset, p.size) == (frm, to - frm)
        assert p.crc == oracle.crc32(p.data)
        if p.part in sl.cols:
            i = p.block * ks + sl.cols.index(p.part) - first
            assert np.shares_memory(p.data, data) and \
                p.data.ctypes.data == data[0, i].ctypes.data
    if want_parity is not None:
        return
    # the gate, against the images as they are
    ops = [writegate.make_op(images[p.part], fmt, t, p.block, p.offset,
                             p.data, 0, p.size, p.crc) for p in packets]
    status, newcrc = writegate.gate_host(ops)
    assert (status == writegate.OK).all()
    # apply: the images grow to the new chunk length, the bytes go in, the
    # gate's CRCs are stored
    n2 = max(n, first + count)
    data_off, crc_off, bstride, cstride = scrub.image_layout(fmt, t)
    for p in range(sl.nparts):
        images[p] = grow(images[p], fmt, t, sl.count(p, n2))
    for p, crc in zip(packets, newcrc):
        img = images[p.part]
        at = data_off + p.block * bstride + p.offset
        img[at:at + p.size] = p.data
        img[crc_off + p.block * cstride:crc_off + p.block * cstride + 4] = \
            np.frombuffer(struct.pack(">I", int(crc)), np.uint8)
    expect = np.zeros((n2, BLOCK), np.uint8)
    expect[:n] = chunk
    expect[first:first + count, frm:to] = data[0]
    for p in range(sl.nparts):
        assert host_scrub(images[p], fmt, t) is None
    # a part without a block: an image of no bytes has no address to pass
    frags = [img[data_off:][None, :] if img.size > data_off
             else np.zeros((1, 16), np.uint8) for img in images]
    losses = [()] + [tuple(sl.cols[:e]) for e in range(1, sl.m + 1)]
    for lost in losses:
        got = chunkread.read_chunks_host(t, frags, [n2], 0, n2,
                                         erased=[list(lost)],
                                         src_stride=bstride)
        assert np.array_equal(got.reshape(n2, BLOCK), expect), lost


@pytest.mark.parametrize("fmt", scrub.FORMATS)
@pytest.mark.parametrize("sl", SLICES[:4], ids=lambda s: s.name)
def test_write_gate_read_loop(sl, fmt):
    """Every chunk length 1..2k+1, every block range inside [0, 2k+2), every
    byte range of SIZES: the packets of write_chunks_host pass the write
    gate against the old images, and after they are applied the chunk reads
    back updated, through the parities as well, and the images scrub
    clean."""
    rng = np.random.default_rng(3)
    limit = 2 * sl.ks + 2
    for n in range(1, limit):
        for first, count in C.block_ranges(limit):
            for frm, to in SIZES:
                write_and_close_the_loop(sl, fmt, n, first, count, frm, to,
                                         rng)


EC82_LENGTHS = (1, 7, 9, 16, 17)


def ec82_block_ranges():
    """Of the 171 block ranges inside [0, 18): every first block with counts
    of 1, one block into the next row, and up to block 17."""
    out = set()
    for first in range(18):
        to_row_end = 8 - first % 8
        for count in (1, to_row_end + 1, 18 - first):
            if first + count <= 18:
                out.add((first, count))
    return sorted(out)


@pytest.mark.parametrize("fmt", scrub.FORMATS)
def test_write_gate_read_loop_ec82(fmt):
    """The loop for ec(8,2) over a part of the matrix (all of it goes
    through write_chunks_host in test_every_range): 5 chunk lengths, the
    block ranges of ec82_block_ranges, every byte range of SIZES."""
    sl = SLICES[4]
    rng = np.random.default_rng(4)
    ranges = ec82_block_ranges()
    assert len(ranges) == 51
    for n in EC82_LENGTHS:
        for first, count in ranges:
            for frm, to in SIZES:
                write_and_close_the_loop(sl, fmt, n, first, count, frm, to,
                                         rng)


def test_write_chunks_host_with_an_unwanted_parity():
    rng = np.random.default_rng(5)
    write_and_close_the_loop(SLICES[3], "interleaved", 7, 2, 5, 0, 4096, rng,
                             want_parity=[1])
    write_and_close_the_loop(SLICES[4], "moosefs", 17, 7, 10, 13, 65536, rng,
                             want_parity=[0])


def test_a_batch_of_writes_in_one_call():
    """Per-chunk ranges, raw block rows (fmt = None)."""
    sl = SLICES[3]
    t = slice_type(sl)
    rng = np.random.default_rng(6)
    ns, firsts, counts = [7, 4, 2], [2, 3, 6], [5, 1, 2]
    chunks = [rng.integers(0, 256, (n, BLOCK), np.uint8) for n in ns]
    frags = []
    for c in range(sl.ks):
        rows = np.zeros((3, 3 * BLOCK), np.uint8)
        for s, ch in enumerate(chunks):
            part = ch[c::sl.ks]
            rows[s, :part.size] = part.reshape(-1)
        frags.append(rows)
    frags += [None, None]
    data = rng.integers(0, 256, (3, 5, 1000), np.uint8)
    parity, crcs, packets = chunkwrite.write_chunks_host(
        t, frags, ns, data, firsts, counts, offset=100, size=1000)
    assert parity.shape == (3, 3, 2, 1000)
    store = C.PartStore(sl.ks * 3, 4)
    for s in range(3):
        w = C.Writes(sl)
        ch = C.Chunk(sl, ns[s], store, 0)
        ch.parts = [chunks[s][c::sl.ks] for c in range(sl.ks)]
        flat = np.ascontiguousarray(data[s]).reshape(-1)
        w.add(ch, firsts[s], counts[s], 100, 1100, flat, 0, 1000)
        e = w.w[0]
        for (i, r), p in e["par"].items():
            assert np.array_equal(parity[s, i, r], p)
        assert list(crcs[s, :counts[s]]) == e["crc"]
        assert len(packets[s]) == counts[s] + 2 * e["touched"]


def test_argument_errors_need_no_library(monkeypatch):
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("library used"))
    t = st.ec_slice_type(3, 2)
    data = np.zeros((1, 2, 100), np.uint8)
    frag = np.zeros((1, 3 * BLOCK), np.uint8)
    ok = dict(slice_type=t, fragments=[frag] * 3 + [None] * 2,
              chunk_blocks=[7], data=data, first_block=1, block_count=2,
              offset=0, size=100)

    def bad(**kw):
        with pytest.raises(ValueError):
            chunkwrite.write_chunks_host(**{**ok, **kw})
    bad(slice_type=st.K_STANDARD)
    bad(size=0)
    bad(offset=65500)
    bad(block_count=0)
    bad(first_block=1023)
    bad(block_count=3)                       # data holds two blocks
    bad(size=99)
    bad(fragments=[frag] * 3)
    bad(fragments=[None] * 5)                # a fill part is missing
    bad(fragments=[frag[:, :BLOCK]] * 3 + [None] * 2)
    bad(want_parity=[2])
    bad(chunk_blocks=[1025])
    bad(fmt="ext4")


def test_symbols_are_exported():
    lib = L.lib()
    assert lib.lizec_chunk_write_batch and lib.lizec_chunk_write_host
    import lizardfs_amd
    assert lizardfs_amd.chunkwrite is chunkwrite
