"""lizec_chunk_write_degraded_batch through the C ABI and
chunkwrite.write_chunks_degraded: the parity of byte ranges written into a
slice with lost parts and the CRC of every packet, bit-exact against the
reference's route through the oracle (chunk_write_degraded_cases.py) and
against the host twin.

Cell ids are [slice-layout], the slices and layouts of
test_gpu_chunk_write.py.  A cell holds the eight writes of the helper, each
into a chunk of its own, and makes one call per availability pattern (healthy;
a lost part that is FILL in the first touched row; FILL in the last row only;
NEW wherever the write touches it; m data parts; a data part and a parity
part), every write taking the pattern where it has a column of the kind.
The `fast` cells make a second call per pattern with the two byte ranges
that cannot be part of an aligned call.  Every call has one slot per part;
the slot of a lost part points at random bytes with the part's block count.
All parity outputs and CRC arrays lie in one arena of 0xA5, each between
256-byte canaries; after a call the whole arena is compared with the
expectation and with the host twin's arena, and so are the sources.
"""
import ctypes
import struct

import numpy as np
import pytest

import chunk_write_cases as C
import chunk_write_degraded_cases as D
import oracle
from test_chunk_write_degraded_host import (SHORT, call_edited,
                                            check_short_chunk_packets,
                                            refusal_edits, short_chunk_case,
                                            slice_type)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK, LIZEC_EINVAL = D.LIZEC_OK, D.LIZEC_EINVAL
BLOCK = C.BLOCK

CELLS = [(s, l) for s in D.SLICES for l in D.LAYOUTS]


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    lib = L.lib()
    lib.lizec_chunk_write_degraded_batch   # a missing symbol fails here
    return lib, L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


class Device:
    """A helper case on the device: store and data uploaded once, an arena
    per call."""

    def __init__(self, case):
        self.case = case
        self.store = torch.from_numpy(case.store.host).cuda()
        self.data = torch.from_numpy(case.data).cuda()
        self.arena = None

    def arrays(self, spare="decoy"):
        self.arena = torch.full((self.case.size,), C.FILL, dtype=torch.uint8,
                                device="cuda")
        for t in (self.store, self.data, self.arena):
            assert t.data_ptr() % 16 == 0
        return self.case.arrays(self.store.data_ptr(), self.data.data_ptr(),
                                self.arena.data_ptr(), spare)

    def run(self, abi, spare="decoy"):
        lib, eng = abi
        arrs = self.arrays(spare)
        return lib.lizec_chunk_write_degraded_batch(
            eng, *self.case.call_args(*arrs), stream_arg())

    def check(self, host=True):
        torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        self.case.check(got)
        assert np.array_equal(self.store.cpu().numpy(),
                              self.case.store.host)
        assert np.array_equal(self.data.cpu().numpy(), self.case.data)
        if host:
            rc, arena = self.case.run_host()
            assert rc == LIZEC_OK
            assert np.array_equal(arena, got)


@pytest.mark.parametrize("name,layout", CELLS,
                         ids=[f"{s}-{l}" for s, l in CELLS])
def test_cell(abi, name, layout):
    assert len(CELLS) == 40 and len(D.PATTERNS) == 6
    assert sorted(D.LAYOUTS) == ["data4", "fast", "il", "odd"]
    sl, lay = D.SLICES[name], D.LAYOUTS[layout]
    cases = [D.Case(sl, lay, D.the_writes(sl.ks, layout == "fast"))]
    if layout == "fast":
        cases.append(D.Case(sl, lay, D.the_writes(sl.ks, False)[5:7], seed=3))
    for n, case in enumerate(cases):
        dev = Device(case)
        for pattern in D.PATTERNS:
            if not case.set_pattern(pattern) and pattern != "healthy":
                continue
            if layout == "fast" and n == 0:
                wr, op, on, pp = dev.arrays()
                bits = 0
                for a in (wr["data"], wr["data_stride"], wr["par_stride"],
                          wr["from"], wr["to"], op, pp):
                    bits |= int(np.bitwise_or.reduce(a.reshape(-1)))
                assert bits % 16 == 0   # the call takes the aligned form
            assert dev.run(abi) == LIZEC_OK
            dev.check()


@pytest.mark.parametrize("name,layout", [("xor3", "odd"), ("ec32", "il"),
                                         ("ec29", "odd"),
                                         ("ec87-rows5", "fast")])
def test_the_mask_is_obeyed(abi, name, layout):
    """Slots outside the masks of a write's tables point at random bytes
    with the part's count, carry address 0 and count 0, or address 0 with
    the part's count."""
    sl, lay = D.SLICES[name], D.LAYOUTS[layout]
    case = D.Case(sl, lay, D.the_writes(sl.ks, layout == "fast"), seed=3)
    dev = Device(case)
    for pattern in ("healthy", "fill-first", "m-data"):
        case.set_pattern(pattern)
        for spare in ("swap", "zero", "null"):
            assert dev.run(abi, spare) == LIZEC_OK
            dev.check(host=False)


@pytest.mark.parametrize("name,layout", [("xor3", "odd"), ("ec32", "fast"),
                                         ("ec87-rows5", "il")])
def test_a_slot_with_a_coefficient_outside_the_mask_is_not_read(abi, name,
                                                                layout):
    """The builder's masks leave out only slots whose column is zero, which
    no output can tell from a slot that was read.  Here every mask loses a
    fill slot whose column is not zero: that column counts as zeros."""
    sl, lay = D.SLICES[name], D.LAYOUTS[layout]
    case = D.Case(sl, lay, D.the_writes(sl.ks, layout == "fast"), seed=9)
    case.set_pattern("healthy")
    before = case.want.copy()
    assert case.drop_a_mask_bit() >= 2
    assert not np.array_equal(before, case.want)
    dev = Device(case)
    assert dev.run(abi) == LIZEC_OK
    dev.check()


@pytest.mark.parametrize("name", ["xor3", "ec52", "ec29"])
def test_a_healthy_call_equals_the_healthy_entry(abi, name):
    from lizardfs_amd import lib as L
    sl, lay = D.SLICES[name], D.LAYOUTS["odd"]
    case = D.Case(sl, lay, D.the_writes(sl.ks, False), seed=5)
    case.set_pattern("healthy")
    dev = Device(case)
    assert dev.run(abi) == LIZEC_OK
    dev.check()
    other = np.full(case.size, C.FILL, np.uint8)
    wr, fp, fn, pp = case.writes.arrays(case.store.host.ctypes.data,
                                        case.data.ctypes.data,
                                        other.ctypes.data)
    rc = L.lib().lizec_chunk_write_host(
        sl.m, C.encode_table(sl).ctypes.data_as(D.u8p),
        ctypes.c_void_p(wr.ctypes.data), len(wr), fp.ctypes.data_as(D.u64p),
        fn.ctypes.data_as(D.u32p), sl.ks, lay.stride,
        pp.ctypes.data_as(D.u64p))
    assert rc == LIZEC_OK
    assert np.array_equal(dev.arena.cpu().numpy(), other)


def test_unwanted_parities_and_no_crcs(abi):
    """ec(2,9) with both data parts lost: only the last parity wanted (the
    first pass returns at once), then a call without CRC arrays."""
    sl, lay = D.SLICES["ec29"], D.LAYOUTS["odd"]
    case = D.Case(sl, lay, D.the_writes(sl.ks, False), seed=7)
    dev = Device(case)
    lost = [D.lost_parts(sl, "m-data", w["chunk"].nb, w["first"],
                         w["count"]) or [] for w in case.writes.w]
    for want, crcs in (([sl.m - 1], True), (None, False)):
        assert case.set_lost(lost, crcs=crcs, want=want)
        assert dev.run(abi) == LIZEC_OK
        dev.check()


def test_call_sequence_on_one_stream(abi):
    """A degraded call, a healthy lizec_chunk_write_batch and a degraded call
    with more tables and more writes, with no synchronisation between them:
    the stream's scratch is reused and grows."""
    lib, eng = abi
    k5, k8 = D.SLICES["ec52"], D.SLICES["ec87-rows5"]
    first = D.Case(k5, D.LAYOUTS["odd"], D.the_writes(5, False)[:3], seed=11)
    first.set_pattern("fill-first")
    third = D.Case(k8, D.LAYOUTS["il"], D.the_writes(8, False) * 3, seed=13)
    lost = [D.lost_parts(k8, D.PATTERNS[i % 6], w["chunk"].nb, w["first"],
                         w["count"]) or []
            for i, w in enumerate(third.writes.w)]
    assert third.set_lost(lost)
    assert len(third.masks) > len(first.masks)
    healthy = D.Case(k5, D.LAYOUTS["data4"], D.the_writes(5, False), seed=12)
    healthy.set_pattern("healthy")
    d1, d2, d3 = Device(first), Device(healthy), Device(third)
    assert d1.run(abi) == LIZEC_OK
    d2.arena = torch.full((healthy.size,), C.FILL, dtype=torch.uint8,
                          device="cuda")
    wr, fp, fn, pp = healthy.writes.arrays(
        d2.store.data_ptr(), d2.data.data_ptr(), d2.arena.data_ptr())
    assert lib.lizec_chunk_write_batch(
        eng, k5.m, C.encode_table(k5).ctypes.data_as(D.u8p),
        ctypes.c_void_p(wr.ctypes.data), len(wr), fp.ctypes.data_as(D.u64p),
        fn.ctypes.data_as(D.u32p), k5.ks, healthy.lay.stride,
        pp.ctypes.data_as(D.u64p), stream_arg()) == LIZEC_OK
    assert d3.run(abi) == LIZEC_OK
    for dev in (d1, d2, d3):
        dev.check(host=False)


def test_refusals_then_a_good_call(abi):
    lib, eng = abi
    sl, lay = D.SLICES["ec32"], D.LAYOUTS["odd"]
    case = D.Case(sl, lay, D.the_writes(sl.ks, False)[:4], seed=17)
    case.set_pattern("fill-first")
    dev = Device(case)
    good = dev.arrays()
    fn = lib.lizec_chunk_write_degraded_batch
    for edit, kw in refusal_edits(case, good):
        assert call_edited(case, fn, (eng,), (stream_arg(),), good, edit,
                           kw) == LIZEC_EINVAL
    assert call_edited(case, fn, (None,), (stream_arg(),), good, None,
                       {}) == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert (dev.arena.cpu().numpy() == C.FILL).all()
    assert call_edited(case, fn, (eng,), (stream_arg(),), good, None,
                       {}) == LIZEC_OK
    dev.check()


@pytest.mark.parametrize("name,n,first,count,avail", SHORT)
def test_write_chunks_degraded_single_short_chunk(name, n, first, count,
                                                  avail):
    """The slots are the parts the plan reads, and the plan leaves out a
    survivor that does not reach the row."""
    from lizardfs_amd import chunkwrite
    t, frags, data, want = short_chunk_case(name, n, first, count, avail)
    frags = [None if f is None else torch.from_numpy(f).cuda()
             for f in frags]
    _, _, (packets,) = chunkwrite.write_chunks_degraded(
        t, frags, [n], torch.from_numpy(data).cuda(), first, count, avail,
        4093, 8195)
    check_short_chunk_packets(t, packets, want, n, first, count, avail)


def test_write_chunks_degraded_refuses_before_the_gpu():
    from lizardfs_amd import chunkwrite
    t = slice_type("ec32")
    frags = [torch.zeros((1, 4 * BLOCK), dtype=torch.uint8, device="cuda")
             for _ in range(5)]
    data = torch.zeros((1, 2, 100), dtype=torch.uint8, device="cuda")
    ok = dict(slice_type=t, fragments=frags, chunk_blocks=[7], data=data,
              first_block=1, block_count=2, available_parts=[1, 2, 3, 4],
              offset=5, size=100)
    chunkwrite.write_chunks_degraded(**ok)
    for kw in (dict(available_parts=[1, 4]),
               dict(available_parts=[1, 2, 3, 5]),
               dict(fragments=frags[:3] + [None] + frags[4:]),
               dict(fragments=frags[:3] + [frags[3].cpu()] + frags[4:]),
               dict(data=data.cpu()), dict(offset=65500)):
        with pytest.raises(ValueError):
            chunkwrite.write_chunks_degraded(**{**ok, **kw})


@pytest.mark.parametrize("name,fmt,lost", [("ec32", "moosefs", 1),
                                           ("ec32", "interleaved", 0),
                                           ("xor3", "interleaved", 2)])
def test_degraded_write_gate_read_loop(name, fmt, lost):
    """A degraded write that overwrites blocks of the lost part (their new
    bytes are stored nowhere) and fills from it -> writegate.gate_batch
    into images of the available parts -> a degraded chunkread.read_chunks
    returns the new chunk, the lost column included."""
    from lizardfs_amd import chunkread, chunkwrite, scrub, writegate
    sl = C.Slice(*D.SLICES[name].kind)
    t = slice_type(name)
    n, first, count, frm, to = 7, 2, 4, 4093, 4093 + 8195
    rng = np.random.default_rng(21)
    chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    avail = [p for p in range(sl.nparts) if p != lost]
    images = [torch.from_numpy(scrub.build_chunk_image(
        7, 1, t, p, list(parts[p]), crc32_fn=oracle.crc32, fmt=fmt)).cuda()
        if p in avail else None for p in range(sl.nparts)]
    new = rng.integers(0, 256, (1, count, to - frm), np.uint8)
    data = torch.from_numpy(new).cuda()
    plan = chunkwrite.plan_write_degraded(t, avail, n, first, count)
    kinds = [k for _, row in plan.rows for k in row]
    assert chunkwrite.LOST in kinds          # the lost part fills a row
    c = sl.cols.index(lost)
    assert any(row[c] == chunkwrite.NEW for _, row in plan.rows)
    parity, crcs, packets = chunkwrite.write_chunks_degraded(
        t, [None if img is None else img[None, :] for img in images], [n],
        data, first, count, avail, frm, to - frm, fmt=fmt)
    (packets,) = packets
    assert [(p.part, p.block) for p in packets] == plan.packets
    assert lost not in {p.part for p in packets}
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
    frags = [None if img is None else img[data_off:][None, :]
             for img in images]
    got = chunkread.read_chunks(t, frags, [n], 0, n, erased=[[lost]],
                                src_stride=bstride)
    assert np.array_equal(got.cpu().numpy().reshape(n, BLOCK), expect)
    assert scrub.scrub_batch([(images[p], t, fmt) for p in avail]) == \
        [None] * len(avail)
