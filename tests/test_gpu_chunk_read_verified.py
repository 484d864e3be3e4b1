"""lizec_chunk_read_verified_batch through the C ABI and read_chunks_verified
through Python, on the GPU: the CRC check of every source block a chunk read
consumes (chunk_read_verified_cases.py has the layouts and the load rule).

Cell ids are [slice-loss-layout].  Losses, by view column: none; data1
(column 1); data-parity (column 1 and the first parity part).  Layouts:

  flat    blocks at stride 65536, 16-byte aligned, the CRCs as arrays at
          stride 4; outputs at stride 65536
  inline  [CRC][block] at stride 65540, the data of successive parts at 4, 8
          and 12 mod 16; outputs at stride 65540 at the same phases

Every cell holds the six reads of test_gpu_chunk_read.py in one call: the
whole chunk, a range with clipped head and tail rows, a recover-only row, a
copy-only row, a range past the chunk's end, and a read of a second chunk
whose unused slots have count 0 and address 0.  The outputs lie in one arena
of 0xA5, each between 256-byte canaries.  After a call the whole arena is
compared with the arena of lizec_chunk_read_batch over the same arguments
(and, for clean sources, with the chunks), the sources and the CRCs with
their pristine copies, and the masks with what is expected: dev_bad_out is
poisoned before every call, so a mask that is not written shows.

Whatever lies behind a part's count is random bytes, data and CRC alike, in
bounds: a check of such a block would set a bit.
"""
import ctypes

import numpy as np
import pytest

import chunk_read_cases as C
import chunk_read_verified_cases as V

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
BLOCK = C.BLOCK
POISON = 0x5EEDBAAD
PHASES = (4, 8, 12)
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

SLICES = {s.name: s for s in (C.Slice("xor", 3), C.Slice("ec", 3, 2),
                              C.Slice("ec", 5, 2))}
LAYOUTS = ("flat", "inline")


def lost_parts(sl, loss):
    parts = [] if loss == "none" else [sl.cols[1]]
    if loss == "data-parity":
        parts.append(sl.parity[0])
    return tuple(parts)


CELLS = [(name, loss, lay) for name, sl in SLICES.items()
         for loss in ("none", "data1", "data-parity")
         if sl.bearable(lost_parts(sl, loss)) for lay in LAYOUTS]


def test_the_cells_are_the_ones_listed():
    assert len(CELLS) == 2 * (2 + 3 + 3)


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    lib = L.lib()
    lib.lizec_chunk_read_verified_batch   # a missing symbol fails here
    return lib, L.engine(0)


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def head_args(reads, tbl, ntables, index, sp, nb, cmap, first, count, dp,
              sstride, dstride):
    return (reads.sl.srcs, reads.rows, ptr(tbl, u8p), ntables,
            ptr(index, u32p), ptr(sp, u64p), ptr(nb, u32p), reads.sl.ks,
            ptr(cmap, u8p), ptr(first, u32p), ptr(count, u32p),
            ptr(dp, u64p), len(reads), sstride, dstride)


class Chunks:
    """nchunks chunks of 2k+1 blocks, cut into parts that lie with their
    CRCs in one uploaded VerifiedStore."""

    def __init__(self, sl, layout, nchunks=2):
        self.sl, self.n, self.layout = sl, 2 * sl.ks + 1, layout
        rng = np.random.default_rng(sl.ks * 100 + sl.m + 7)
        self.chunks = [rng.integers(0, 256, (self.n, BLOCK), np.uint8)
                       for _ in range(nchunks)]
        inline = layout == "inline"
        self.store = V.VerifiedStore(
            nchunks * sl.nparts, 4, "inline" if inline else "array",
            phase=(lambda i: PHASES[i % 3]) if inline else None,
            seed=sl.ks + 50)
        self.where = [[self.store.put(p) for p in sl.cut(ch)]
                      for ch in self.chunks]
        self.dstride = V.INLINE if inline else BLOCK
        self.upload()

    def upload(self):
        """(Re)load the device copies from the host store."""
        st = self.store
        self.dev = torch.from_numpy(st.data).cuda()
        self.dev_crc = self.dev if st.inline else \
            torch.from_numpy(st.crc).cuda()
        self.pristine = self.dev.clone(), self.dev_crc.clone()
        assert self.dev.data_ptr() % 16 == 0

    def add(self, reads, which, lost, first, count, index=0, verify=None):
        sl = self.sl
        srcs, cmap, _ = sl.plan(lost)
        verify = verify or [True] * len(srcs)
        reads.add([self.where[which][p][0] for p in srcs],
                  [sl.count(p, self.n) for p in srcs], cmap, first, count,
                  C.chunk_blocks(self.chunks[which], first, count), index,
                  crc_offs=[self.where[which][p][1] if v else None
                            for p, v in zip(srcs, verify)])
        reads.parts = getattr(reads, "parts", []) + [(which, srcs)]

    def flip(self, which, part, block, byte=None, crc_byte=None):
        """XOR one byte of a block, or of its CRC, in the host store."""
        st, (off, coff) = self.store, self.where[which][part]
        if byte is not None:
            st.data[off + block * st.stride + byte] ^= 0xA0 | (part + 1)
        if crc_byte is not None:
            st.crc[coff + block * st.crc_stride + crc_byte] ^= 0x01


_chunks = {}


def chunks_of(name, layout):
    """Kept per slice: the cells of a slice run in a row."""
    if not any(k[0] == name for k in _chunks):
        _chunks.clear()
    if (name, layout) not in _chunks:
        _chunks[name, layout] = Chunks(SLICES[name], layout)
    return _chunks[name, layout]


def six_reads(ch, lost):
    sl, n, ks = ch.sl, ch.n, ch.sl.ks
    _, _, tbl = sl.plan(lost)
    rows = 0 if tbl is None else tbl.size // (32 * sl.srcs)
    reads = V.VReads(sl, rows)
    for f, c in ((0, n), (1, ks + 1), (ks + 1, 1), (ks, 1), (n - 1, ks + 2)):
        ch.add(reads, 0, lost, f, c)
    # read 5: the longest run of columns of row 1 that chunk 0 has not lost;
    # the other slots have count 0, address 0 and CRC address 0
    gone = [c for c, p in enumerate(sl.cols) if p in lost]
    runs, start = [], 0
    for c in gone + [ks]:
        runs.append((c - start, start))
        start = c + 1
    width, c0 = max(runs)
    reads.add([None if c in gone else ch.where[1][sl.cols[c]][0]
               for c in range(ks)],
              [0 if c in gone else sl.count(sl.cols[c], n)
               for c in range(ks)],
              [C.UNMAPPED if c in gone else c for c in range(ks)],
              ks + c0, width, ch.chunks[1][ks + c0:ks + c0 + width],
              crc_offs=[None if c in gone else ch.where[1][sl.cols[c]][1]
                        for c in range(ks)])
    return reads, tbl


def run_gpu(abi, reads, tbl, ntables, ch, use_index=False, clean=True):
    """One verified and one plain call; returns (masks, arena)."""
    lib, eng = abi
    st = ch.store
    dphase = (lambda i: PHASES[i % 3]) if st.inline else None
    offs, size = reads.out_layout(ch.dstride, dphase)
    arenas = [torch.full((size,), C.FILL, dtype=torch.uint8, device="cuda")
              for _ in range(2)]
    bad = torch.from_numpy(
        np.full(len(reads), POISON, np.uint32).view(np.int32)).cuda()
    for verified, arena in zip((True, False), arenas):
        assert arena.data_ptr() % 16 == 0
        sp, nb, cmap, first, count, dp, index = reads.arrays(
            ch.dev.data_ptr(), arena.data_ptr(), offs)
        head = head_args(reads, tbl, ntables, index if use_index else None,
                         sp, nb, cmap, first, count, dp, st.stride,
                         ch.dstride)
        if verified:
            cp = reads.crc_ptrs(ch.dev_crc.data_ptr())
            r = lib.lizec_chunk_read_verified_batch(
                eng, *head, ptr(cp, u64p), st.crc_stride,
                ctypes.c_void_p(bad.data_ptr()), stream_arg())
        else:
            r = lib.lizec_chunk_read_batch(eng, *head, stream_arg())
        assert r == LIZEC_OK
    torch.cuda.synchronize()
    got = arenas[0].cpu().numpy()
    assert np.array_equal(got, arenas[1].cpu().numpy()), \
        "the verified read wrote other bytes than the plain one"
    if clean:
        want = reads.expected_arena(offs, size, ch.dstride)
        if not np.array_equal(got, want):
            diff = np.flatnonzero(got != want)
            pytest.fail(f"{diff.size} bytes differ, first at "
                        f"{diff[:6].tolist()}, outputs at {offs}")
    assert torch.equal(ch.dev, ch.pristine[0]), "a source changed"
    assert torch.equal(ch.dev_crc, ch.pristine[1]), "a CRC changed"
    return bad.cpu().numpy().view(np.uint32), got


def run_host(reads, tbl, ntables, ch, use_index=False):
    """The host twin over the host store: (masks, arena)."""
    from lizardfs_amd import lib as L
    st = ch.store
    dphase = (lambda i: PHASES[i % 3]) if st.inline else None
    offs, size = reads.out_layout(ch.dstride, dphase)
    arena = np.full(size + 16, C.FILL, np.uint8)
    skew = -arena.ctypes.data % 16
    sp, nb, cmap, first, count, dp, index = reads.arrays(
        st.data.ctypes.data, arena.ctypes.data + skew, offs)
    cp = reads.crc_ptrs(st.crc.ctypes.data)
    bad = np.full(len(reads), POISON, np.uint32)
    assert L.lib().lizec_chunk_read_verified_host(
        *head_args(reads, tbl, ntables, index if use_index else None, sp,
                   nb, cmap, first, count, dp, st.stride, ch.dstride),
        ptr(cp, u64p), st.crc_stride,
        ctypes.c_void_p(bad.ctypes.data)) == LIZEC_OK
    return bad, arena[skew:skew + size]


@pytest.mark.parametrize("name,loss,layout", CELLS,
                         ids=["-".join(c) for c in CELLS])
def test_clean_cell(abi, name, loss, layout):
    ch = chunks_of(name, layout)
    reads, tbl = six_reads(ch, lost_parts(ch.sl, loss))
    bad, _ = run_gpu(abi, reads, tbl, 1 if reads.rows else 0, ch)
    assert bad.tolist() == [0] * 6


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(SLICES))
def test_corruption(abi, name, layout):
    """Eight reads, one chunk each, in one call: bad slot 0, the last slot,
    two at once, none; first and last blocks of a part; bytes 0, 65535 and
    interior ones; a CRC byte; corruption that the read does not look at."""
    sl = SLICES[name]
    ch = Chunks(sl, layout, nchunks=8)
    n, ks = ch.n, sl.ks
    lost = (sl.cols[1],)
    srcs, _, tbl = sl.plan(lost)
    last = srcs[-1]
    # the part behind column 0: its last block (row 2) is the chunk's last
    # and is read by every whole-chunk read; the other parts' row 2 is not
    p0 = sl.cols[0]
    j0 = srcs.index(p0)
    other = [p for p in srcs if p != p0][0]
    reads = V.VReads(sl, 1)
    ch.add(reads, 0, lost, 0, n)
    ch.flip(0, srcs[0], 0, byte=0)                       # slot 0, first block
    ch.add(reads, 1, lost, 0, n)
    ch.flip(1, last, 0, byte=BLOCK - 1)                  # the last slot
    ch.add(reads, 2, lost, 0, n)                         # two slots at once:
    ch.flip(2, p0, sl.count(p0, n) - 1, byte=30001)      # a part's last block
    ch.flip(2, last, 1, byte=12345)
    ch.add(reads, 3, lost, 0, n)                         # none
    ch.add(reads, 4, lost, 0, n)
    ch.flip(4, srcs[1], 0, crc_byte=2)                   # a stored CRC
    ch.add(reads, 5, (), 0, n)                           # healthy, in a rows
    ch.flip(5, sl.cols[1], 1, byte=BLOCK - 1)            # = 1 call: column 1
    ch.flip(5, sl.parity[0], 0, byte=0)                  # parity: not read
    ch.add(reads, 6, lost, ks, 1)                        # copy-only row 1
    ch.flip(6, other, 1, byte=5)                         # not loaded
    ch.flip(6, p0, 0, byte=5)                            # row 0: not touched
    ch.add(reads, 7, lost, 1, ks + 1,
           verify=[False] + [True] * (ks - 1))           # slot 0 unverified
    ch.flip(7, srcs[0], 0, byte=1)
    ch.upload()
    assert j0 != ks - 1
    want = [1, 1 << (ks - 1), 1 << j0 | 1 << (ks - 1), 0, 2, 2, 0, 0]
    host_bad, host_arena = run_host(reads, tbl, 1, ch)
    assert host_bad.tolist() == want
    bad, arena = run_gpu(abi, reads, tbl, 1, ch, clean=False)
    assert bad.tolist() == want
    assert np.array_equal(arena, host_arena)


def test_gpu_and_host_twins_agree(abi):
    """ec(3,2), two tables, healthy and degraded reads, some bad blocks."""
    sl = SLICES["ec32"]
    ch = Chunks(sl, "inline", nchunks=2)
    reads, tables = V.VReads(sl, 2), []
    for i, (lost, f, c) in enumerate((((0, 1), 0, 7), ((1, 4), 6, 5),
                                      ((0, 1), 2, 2), ((1, 4), 1, 4))):
        _, _, tbl = sl.plan(lost)
        full = np.zeros(32 * 3 * 2, np.uint8)
        full[:tbl.size] = tbl
        tables.append(full)
        ch.add(reads, i % 2, lost, f, c, index=i % 2)
    tables = np.concatenate(tables[:2])
    for f, c in ((0, 7), (4, 2)):
        ch.add(reads, 0, (), f, c)
    ch.flip(0, 2, 0, byte=777)          # chunk 0: part 2 and parity 3
    ch.flip(0, 3, 2, crc_byte=0)
    ch.flip(1, 0, 2, byte=BLOCK - 1)    # chunk 1: part 0's last block
    ch.upload()
    host_bad, host_arena = run_host(reads, tables, 2, ch, True)
    bad, arena = run_gpu(abi, reads, tables, 2, ch, True, clean=False)
    assert bad.tolist() == host_bad.tolist()
    assert any(bad) and not all(bad)
    assert np.array_equal(arena, host_arena)
    model = [V.expected_mask(
        3, reads.cmap[i], reads.nb[i], reads.first[i], reads.count[i],
        reads.crc[i],
        [(srcs.index(p), b) for w, p, b in ((0, 2, 0), (0, 3, 2), (1, 0, 2))
         if w == which and p in srcs])
        for i, (which, srcs) in enumerate(reads.parts)]
    assert bad.tolist() == model


def test_refusals_enqueue_nothing(abi):
    lib, eng = abi
    ch = chunks_of("ec32", "flat")
    reads, tbl = six_reads(ch, (ch.sl.cols[1],))
    offs, size = reads.out_layout()
    arena = torch.full((size,), C.FILL, dtype=torch.uint8, device="cuda")
    bad = torch.from_numpy(
        np.full(6, POISON, np.uint32).view(np.int32)).cuda()
    base = dict(zip(("sp", "nb", "cmap", "first", "count", "dp"),
                    reads.arrays(ch.dev.data_ptr(), arena.data_ptr(), offs)))
    base["cp"] = reads.crc_ptrs(ch.dev_crc.data_ptr())

    def call(tbl=tbl, sstride=BLOCK, dstride=BLOCK, cstride=4, engine=eng,
             bad_ptr=bad.data_ptr(), **change):
        a = {k: v.copy() for k, v in base.items()}
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                a[k].reshape(-1)[v[0]] = v[1]
        return lib.lizec_chunk_read_verified_batch(
            engine, *head_args(reads, tbl, 1, None, a["sp"], a["nb"],
                               a["cmap"], a["first"], a["count"], a["dp"],
                               sstride, dstride),
            ptr(a["cp"], u64p), cstride, ctypes.c_void_p(bad_ptr),
            stream_arg())

    refused = {
        "crc_dptrs NULL": dict(cp=None),
        "dev_bad_out NULL": dict(bad_ptr=None),
        "crc_block_stride 3": dict(cstride=3),
        "crc_block_stride 0": dict(cstride=0),
        "engine NULL": dict(engine=None),
        "source address 0 with a count": dict(sp=(1, 0)),
        "source address 2 mod 4": dict(sp=(0, int(base["sp"][0, 0]) + 2)),
        "source stride 65538": dict(sstride=65538),
        "destination stride 65532": dict(dstride=65532),
        "tables NULL at rows 1": dict(tbl=None),
        "col_map names slot 3": dict(cmap=(0, 3)),
        "a requested column unmapped": dict(cmap=(0, 0xFF)),
        "block_count 0": dict(count=(1, 0)),
        "destination address 0": dict(dp=(0, 0)),
        "dst_dptrs NULL": dict(dp=None),
    }
    for what, change in refused.items():
        assert call(**change) == LIZEC_EINVAL, what
    torch.cuda.synchronize()
    assert bool((arena == C.FILL).all())
    assert (bad.cpu().numpy().view(np.uint32) == POISON).all()
    # and the call they are one change away from
    assert call() == LIZEC_OK
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(),
                          reads.expected_arena(offs, size))
    assert bad.cpu().numpy().tolist() == [0] * 6


def test_write_gate_read_loop_closes_through_the_crc_field():
    """write_chunks fills INTERLEAVED images; readgate.read_packets turns
    them into whole-block READ_DATA payloads, [CRC][block]; those are the
    fragments of read_chunks_verified with inline CRCs."""
    import oracle
    from lizardfs_amd import chunkread, chunkwrite, readgate, scrub
    from lizardfs_amd import slice_traits as st
    sl = C.Slice("ec", 3, 2)
    t = st.ec_slice_type(3, 2)
    n = 7
    rng = np.random.default_rng(31)
    old = rng.integers(0, 256, (n, BLOCK), np.uint8)
    images = [torch.from_numpy(scrub.build_chunk_image(
        9, 1, t, p, list(part), crc32_fn=oracle.crc32,
        fmt="interleaved")).cuda() for p, part in enumerate(sl.cut(old))]
    chunk = rng.integers(0, 256, (1, n, BLOCK), np.uint8)
    data = torch.from_numpy(chunk).cuda()
    _, _, packets = chunkwrite.write_chunks(
        t, [img[None, :] for img in images], [n], data, 0, n,
        fmt="interleaved")
    data_off, crc_off, bstride, cstride = scrub.image_layout("interleaved", t)
    assert (data_off, crc_off, bstride) == (4, 0, V.INLINE)
    for p in packets[0]:
        img = images[p.part]
        img[data_off + p.block * bstride:][:BLOCK] = p.data
        img[crc_off + p.block * cstride:][:4] = torch.from_numpy(
            np.array([p.crc], ">u4").view(np.uint8)).cuda()

    def received():
        frags = []
        for p, img in enumerate(images):
            pk, starts, status = readgate.read_packets(
                img, "interleaved", t,
                [(b, 0, BLOCK) for b in range(sl.count(p, n))])
            assert (status.cpu().numpy() == readgate.OK).all()
            assert starts.tolist() == [b * V.INLINE
                                       for b in range(sl.count(p, n))]
            frags.append(pk[None, :])
        return frags

    def read(frags, **kw):
        r = chunkread.read_chunks_verified(
            t, frags, None, [n], 0, n, src_stride=V.INLINE,
            inline_crcs=True, **kw)
        assert np.array_equal(r.out.cpu().numpy().reshape(n, BLOCK),
                              chunk[0])
        return r

    frags = received()
    r = read(frags)
    assert r.corrupt == [()] and r.unreadable == [False]
    r = read(frags, erased={0, 2})
    assert r.corrupt == [()] and r.unreadable == [False]
    # a byte of one received stream flips on the way
    frags[1][0, 4 + V.INLINE + 99] ^= 0x08
    r = read(frags)
    assert r.corrupt == [(1,)] and r.unreadable == [False]
    r = read(frags, erased={0})
    assert r.corrupt == [(1,)] and r.unreadable == [False]
    # the images themselves are such fragments: a byte of one flips after
    # the packets were made, and a read straight from the images names it
    images[2][data_off + 5] ^= 0x80
    r = read([img[None, :] for img in images])
    assert r.corrupt == [(2,)] and r.unreadable == [False]
