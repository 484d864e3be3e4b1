"""lizec_chunk_write_batch through the C ABI: the parity of byte ranges written
into the blocks of a slice and the CRC of every packet, bit-exact against the
rule of lizec.h put together with numpy and the oracle
(chunk_write_cases.py).

Cell ids are [slice-layout].  The slices: xor3, ec(2,1) (one parity),
ec(3,2), ec(5,2) (two), the first 3..7 parities of ec(8,7) (a call with
rows = 3..7) and ec(2,9) (rows = 9: a pass of 8 and a pass of 1, which cut
tiles of different sizes).  The layouts:

  fast   parts at stride 65536, every address, stride, `from` and size a
         multiple of 16, parity in place in an image of stride 65536: the
         aligned kernel form.  The byte ranges that are no multiples of 16
         cannot be part of such a call; the cell makes a second call with
         them, which runs the general form at aligned addresses.
  il     parts and parity images at the INTERLEAVED stride 65540, 4 past a
         16-byte boundary, parity in place (address = block 0 + r0 * 65540 +
         from)
  data4  data at 4, 8, 12 mod 16, packed at stride = size
  odd    data at 1, 7, 13 and parity at 13, 1, 7 mod 16, both packed at
         stride = size (packet-compact)

Every cell holds, in one call, seven writes, each into a chunk of its own:

  write  chunk blocks  range                bytes            what it is for
  0      2k+1          block k+1            whole block      one block mid-row
  1      2k+1          1 .. 2k              whole blocks     from mid-row over
                                                             three rows, ends
                                                             mid-row
  2      2k+1          0 .. 2k-1            whole blocks     whole rows, every
                                                             fill count 0
  3      2k-1          block k              [13, 65536)      the last, short
                                                             row: new, fill
                                                             and absent
  4      k+1           2k-1, 2k             [4093, +8195)    append past the
                                                             end over absent
                                                             columns
  5      2k+1          block 1              [65535, 65536)   one byte
  6      2k+1          k-1 .. 2k-1          [13, +20485)     partial last
                                                             tile, tail of 5

(fast: [16, 65536), [4096, +8240), [65520, 65536), [4096, +20528) in the
first call; writes 5 and 6 as above in the second.)

Every part has room for one block more than its chunk gives any part, in a
buffer of random bytes.  All parity outputs and CRC arrays lie in one arena
of 0xA5, each between 256-byte canaries; after a call the whole arena is
compared, and so are the sources.
"""
import ctypes
import struct

import numpy as np
import pytest

import chunk_write_cases as C
import oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
BLOCK = C.BLOCK
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

SLICES = {s.name: s for s in
          [C.Slice("xor", 3), C.Slice("ec", 2, 1), C.Slice("ec", 3, 2),
           C.Slice("ec", 5, 2), C.Slice("ec", 2, 9)] +
          [C.FirstRows(8, 7, r) for r in range(3, 8)]}


class Layout:
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

CELLS = [(s, l) for s in SLICES for l in LAYOUTS]


def the_writes(ks, aligned):
    """(chunk blocks, first, count, from, to, fill) of writes 0..6."""
    n = 2 * ks + 1
    if aligned:
        r3, r4, r5, r6 = (16, 65536), (4096, 4096 + 8240), (65520, 65536), \
            (4096, 4096 + 20528)
    else:
        r3, r4, r5, r6 = (13, 65536), (4093, 4093 + 8195), (65535, 65536), \
            (13, 13 + 20485)
    return [(n, ks + 1, 1, 0, 65536, True),
            (n, 1, 2 * ks, 0, 65536, True),
            (n, 0, 2 * ks, 0, 65536, False),
            (2 * ks - 1, ks, 1) + r3 + (True,),
            (ks + 1, 2 * ks - 1, 2) + r4 + (True,),
            (n, 1, 1) + r5 + (True,),
            (n, ks - 1, ks + 1) + r6 + (True,)]


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    lib = L.lib()
    lib.lizec_chunk_write_batch   # a missing symbol fails here
    return lib, L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def call_write(abi, rows, tbl, wr, fp, fn, ks, stride, pp, num=None,
               engine="abi"):
    """Arguments as numpy arrays or None (= NULL)."""
    lib, eng = abi

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    return lib.lizec_chunk_write_batch(
        eng if engine == "abi" else engine, rows, ptr(tbl, u8p),
        None if wr is None else ctypes.c_void_p(wr.ctypes.data),
        (0 if wr is None else len(wr)) if num is None else num,
        ptr(fp, u64p), ptr(fn, u32p), ks, stride, ptr(pp, u64p),
        stream_arg())


class Case:
    """Some writes of a slice in a layout: the part store, the data buffer,
    the arena and what it has to hold, on the host and on the device."""

    def __init__(self, sl, lay, specs, seed=1, want=None, crcs=True):
        self.sl, self.lay = sl, lay
        self.store = C.PartStore(sl.ks * len(specs), 4, lay.stride,
                                 lambda i: lay.phase, seed=seed)
        rng = np.random.default_rng(seed + 1)
        at, where = 0, []
        for i, (n, first, count, frm, to, fill) in enumerate(specs):
            ds = lay.data_stride(to - frm)
            where.append((at + C.GUARD + lay.data_phase[i % 3], ds))
            at += (C.GUARD + 16 + count * ds + 15) // 16 * 16
        self.data = rng.integers(0, 256, at + C.GUARD, np.uint8)
        self.writes = C.Writes(sl)
        for i, (n, first, count, frm, to, fill) in enumerate(specs):
            chunk = C.Chunk(sl, n, self.store, seed + 10 + i)
            self.writes.add(chunk, first, count, frm, to, self.data,
                            where[i][0], where[i][1], fill=fill,
                            want=want, crcs=crcs)
        self.size, self.want = self.writes.layout(lay.par_phase,
                                                  lay.par_stride)
        self.tbl = C.encode_table(sl)
        self.d_store = torch.from_numpy(self.store.host).cuda()
        self.d_data = torch.from_numpy(self.data).cuda()
        self.d_arena = torch.full((self.size,), C.FILL, dtype=torch.uint8,
                                  device="cuda")
        for t in (self.d_store, self.d_data, self.d_arena):
            assert t.data_ptr() % 16 == 0

    def arrays(self):
        return self.writes.arrays(self.d_store.data_ptr(),
                                  self.d_data.data_ptr(),
                                  self.d_arena.data_ptr())

    def run(self, abi):
        wr, fp, fn, pp = self.arrays()
        return call_write(abi, self.sl.m, self.tbl, wr, fp, fn, self.sl.ks,
                          self.lay.stride, pp)

    def run_host(self):
        from lizardfs_amd import lib as L
        arena = np.full(self.size, C.FILL, np.uint8)
        wr, fp, fn, pp = self.writes.arrays(self.store.host.ctypes.data,
                                            self.data.ctypes.data,
                                            arena.ctypes.data)
        rc = L.lib().lizec_chunk_write_host(
            self.sl.m, self.tbl.ctypes.data_as(u8p),
            ctypes.c_void_p(wr.ctypes.data), len(wr),
            fp.ctypes.data_as(u64p), fn.ctypes.data_as(u32p), self.sl.ks,
            self.lay.stride, pp.ctypes.data_as(u64p))
        assert rc == LIZEC_OK
        return arena

    def check(self):
        torch.cuda.synchronize()
        got = self.d_arena.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, (self.sl.name, self.lay.name, bad.size,
                               int(bad[0]))
        assert np.array_equal(self.d_store.cpu().numpy(), self.store.host)
        assert np.array_equal(self.d_data.cpu().numpy(), self.data)


def test_the_cells_are_the_ones_listed():
    assert sorted(SLICES) == sorted(
        ["xor3", "ec21", "ec32", "ec52", "ec29"] +
        [f"ec87-rows{r}" for r in range(3, 8)])
    assert [SLICES[s].m for s in SLICES] == [1, 1, 2, 2, 9, 3, 4, 5, 6, 7]
    assert len(CELLS) == 40


@pytest.mark.parametrize("name,layout", CELLS,
                         ids=[f"{s}-{l}" for s, l in CELLS])
def test_cell(abi, name, layout):
    sl, lay = SLICES[name], LAYOUTS[layout]
    specs = the_writes(sl.ks, aligned=layout == "fast")
    case = Case(sl, lay, specs)
    if layout == "fast":
        wr, fp, fn, pp = case.arrays()
        bits = 0
        for a in (wr["data"], wr["data_stride"], wr["par_stride"],
                  wr["from"], wr["to"], fp, pp):
            bits |= int(np.bitwise_or.reduce(a.reshape(-1)))
        assert bits % 16 == 0      # the call takes the aligned form
    assert case.run(abi) == LIZEC_OK
    case.check()
    if layout == "fast":
        rest = Case(sl, lay, the_writes(sl.ks, False)[5:], seed=3)
        assert rest.run(abi) == LIZEC_OK
        rest.check()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_and_host_twins_agree(abi, layout):
    sl, lay = SLICES["ec32"], LAYOUTS[layout]
    case = Case(sl, lay, the_writes(sl.ks, aligned=layout == "fast"), seed=5)
    assert case.run(abi) == LIZEC_OK
    case.check()
    assert np.array_equal(case.run_host(), case.d_arena.cpu().numpy())


@pytest.mark.parametrize("name", ["ec32", "ec29"])
def test_unwanted_parities_and_no_crcs(abi, name):
    """Parity 0 unwanted: its bytes and CRC slots stay 0xA5 (for ec(2,9) the
    other eight of its pass are still written, and with only parity 8 wanted
    the first pass returns at once); then a call without CRC arrays."""
    sl, lay = SLICES[name], LAYOUTS["odd"]
    specs = the_writes(sl.ks, False)
    for want, crcs in ((list(range(1, sl.m)), True), ([sl.m - 1], True),
                       (None, False)):
        case = Case(sl, lay, specs, seed=7, want=want, crcs=crcs)
        assert case.run(abi) == LIZEC_OK
        case.check()


def test_call_sequence_on_one_stream(abi):
    """Large, small, large with other rows, with no synchronisation between
    them: the stream's scratch is reused and grows."""
    k5, k2 = SLICES["ec52"], SLICES["ec29"]
    lay = LAYOUTS["il"]
    big = Case(k5, lay, [(11, 0, 10, 0, 65536, False)] * 12 +
               the_writes(5, False), seed=11)
    small = Case(k5, LAYOUTS["odd"], [(11, 1, 1, 65535, 65536, True)],
                 seed=12)
    other = Case(k2, LAYOUTS["data4"], the_writes(2, False) * 6, seed=13)
    again = Case(k5, LAYOUTS["fast"], the_writes(5, True), seed=14)
    for case in (big, small, other, again):
        assert case.run(abi) == LIZEC_OK
    for case in (big, small, other, again):
        case.check()


def test_refusals_then_a_good_call(abi):
    sl, lay = SLICES["ec32"], LAYOUTS["odd"]
    case = Case(sl, lay, the_writes(sl.ks, False)[:4], seed=17)
    good = case.arrays()

    def refused(edit=None, **kw):
        wr, fp, fn, pp = (a.copy() for a in good)
        a = dict(wr=wr, fp=fp, fn=fn, pp=pp, tbl=case.tbl)
        if edit:
            edit(a)
        rc = call_write(abi, kw.pop("rows", sl.m), a["tbl"], a["wr"],
                        a["fp"], a["fn"], kw.pop("ks", sl.ks),
                        kw.pop("stride", lay.stride), a["pp"], **kw)
        assert rc == LIZEC_EINVAL

    def field(i, name, value):
        def edit(a):
            a["wr"][name][i] = value
        return edit

    for name in ("tbl", "wr", "fp", "fn", "pp"):
        refused(lambda a, name=name: a.__setitem__(name, None), num=4)
    refused(engine=None)
    refused(num=0)
    refused(rows=0)
    refused(rows=33)
    refused(ks=0)
    refused(ks=33)
    refused(field(0, "from", 65536))
    refused(field(3, "to", 65537))
    refused(field(3, "to", 13))
    refused(field(1, "block_count", 0))
    refused(field(1, "first_block", 1048576 - 5))
    refused(field(2, "data", 0))
    refused(field(1, "data_stride", 65535))
    refused(field(1, "par_stride", 65535))
    refused(stride=65535)
    refused(lambda a: a["fn"].__setitem__((0, 1), 32769))
    refused(lambda a: a["fp"].__setitem__((0, 0), 0))
    refused(field(0, "crcs", int(good[0]["crcs"][0]) + 1))
    refused(lambda a: (a["pp"].__setitem__((2, slice(None)), 0),
                       field(2, "crcs", 0)(a)))
    torch.cuda.synchronize()
    assert (case.d_arena.cpu().numpy() == C.FILL).all()
    assert case.run(abi) == LIZEC_OK
    case.check()


@pytest.mark.parametrize("fmt", ["moosefs", "interleaved"])
def test_write_gate_read_scrub_loop(fmt):
    """write_chunks -> writegate.gate_batch (all OK, the new CRCs stored)
    -> chunkread.read_chunks returns the updated chunk -> scrub clean."""
    from lizardfs_amd import chunkread, chunkwrite, scrub, writegate
    from lizardfs_amd import slice_traits as st
    sl = C.Slice("ec", 3, 2)
    t = st.ec_slice_type(3, 2)
    n, first, count, frm, to = 7, 2, 5, 4093, 4093 + 8195
    rng = np.random.default_rng(21)
    chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    images = [torch.from_numpy(scrub.build_chunk_image(
        7, 1, t, p, list(parts[p]), crc32_fn=oracle.crc32, fmt=fmt)).cuda()
        for p in range(sl.nparts)]
    new = rng.integers(0, 256, (1, count, to - frm), np.uint8)
    data = torch.from_numpy(new).cuda()
    parity, crcs, packets = chunkwrite.write_chunks(
        t, [img[None, :] for img in images], [n], data, first, count, frm,
        to - frm, fmt=fmt)
    (packets,) = packets
    plan = chunkwrite.plan_write(t, n, first, count)
    assert [(p.part, p.block) for p in packets] == plan.packets
    for p in packets:
        assert p.crc == oracle.crc32(p.data.cpu().numpy())
        if p.part in sl.cols:
            i = p.block * sl.ks + sl.cols.index(p.part) - first
            assert p.data.data_ptr() == data[0, i].data_ptr()
    ops = [writegate.make_op(images[p.part], fmt, t, p.block, p.offset,
                             p.data, 0, p.size, p.crc) for p in packets]
    status, newcrc = writegate.gate_batch(ops)
    assert (status.cpu().numpy() == writegate.OK).all()
    newcrc = newcrc.cpu().numpy().view(np.uint32)
    data_off, crc_off, bstride, cstride = scrub.image_layout(fmt, t)
    for p, crc in zip(packets, newcrc):
        img = images[p.part]
        at = data_off + p.block * bstride + p.offset
        img[at:at + p.size] = p.data
        img[crc_off + p.block * cstride:crc_off + p.block * cstride + 4] = \
            torch.from_numpy(np.frombuffer(struct.pack(">I", int(crc)),
                                           np.uint8).copy()).cuda()
    expect = chunk.copy()
    expect[first:first + count, frm:to] = new[0]
    frags = [img[data_off:][None, :] for img in images]
    for lost in ((), (0,), (0, 1)):
        got = chunkread.read_chunks(t, frags, [n], 0, n, erased=[list(lost)],
                                    src_stride=bstride)
        assert np.array_equal(got.cpu().numpy().reshape(n, BLOCK), expect)
    assert scrub.scrub_batch([(img, t, fmt) for img in images]) == \
        [None] * sl.nparts
