"""lizec_chunk_read_batch through the C ABI: block ranges of chunks gathered
from the parts of a slice, lost parts rebuilt on the way, bit-exact against
the chunk that the parts were cut from (chunk_read_cases.py).

Cell ids are [slice-loss-layout].  The losses, by view column (column 0
always survives):

  none         rows = 0, tables NULL: the pure gather
  data1        column 1
  data2        columns 1 and ks-1
  data-parity  column 1 and the first parity part
  data9        columns 1..9 of ec(32,9): rows = 9, the second pass
  rowsR        columns 1..R of ec(8,7), R = 3..7: the row counts that the
               slices above do not reach

Every cell holds, in one call, six reads.  Reads 0-4 are on a degraded chunk
A of n = 2*ks + 1 blocks, read 5 on a healthy chunk B of as many:

  read  range                          what it is for
  0     the whole chunk                a short last row, parts of different
                                       counts, a lost column absent from the
                                       last row
  1     first 1, count ks + 1          partial head and tail rows; block 0
                                       must not be written
  2     block ks + 1                   a lost column (at loss none: any) of
                                       row 1 alone: recover-only row
  3     block ks                       a surviving column alone: copy-only
                                       row in a rows > 0 call
  4     first n - 1, count ks + 2      blocks past the chunk's end are zeros
  5     chunk B, the longest run of    mixed batch; the slots of the columns
        columns of row 1 that are      lost in A have count 0 and address 0
        not lost in A                  and their columns are unmapped

Every part has room for one block more than its chunk gives any part, in a
buffer of random bytes, so a read past a count changes the result.  The
outputs lie in one arena of 0xA5, each between 256-byte canaries; after a
call the whole arena is compared, so the canaries, the blocks around a
range and the gaps between two output blocks must still be 0xA5.  The
sources are compared after every call as well.
"""
import ctypes

import numpy as np
import pytest

import chunk_read_cases as C

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
BLOCK = C.BLOCK
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

SLICES = {s.name: s for s in (C.Slice("xor", 3), C.Slice("ec", 2, 1),
                              C.Slice("ec", 3, 2), C.Slice("ec", 5, 2),
                              C.Slice("ec", 32, 9), C.Slice("ec", 8, 7))}
# name -> ((source stride, phase), (destination stride, phase))
LAYOUTS = {
    "il-il": ((65540, 4), (65540, 4)),
    "flat-il": ((65536, 0), (65540, 4)),
    "il-flat": ((65540, 4), (65536, 0)),
    "al-strided": ((65552, 0), (65600, 0)),
}
PHASES = (4, 8, 12)


def lost_parts(sl, loss):
    """The parts of chunk A that are gone."""
    cols = {"none": [], "data1": [1], "data2": [1, sl.ks - 1],
            "data-parity": [1], "data9": list(range(1, 10))}.get(loss)
    if cols is None:
        cols = list(range(1, int(loss[4:]) + 1))
    parts = [sl.cols[c] for c in sorted(set(cols))]
    if loss == "data-parity":
        parts.append(sl.parity[0])
    return tuple(parts)


def cells():
    out = []
    for name in ("xor3", "ec21", "ec32", "ec52", "ec329"):
        sl = SLICES[name]
        losses = ["none", "data1", "data2", "data-parity"]
        if name == "ec329":
            losses.append("data9")
        for loss in losses:
            lost = lost_parts(sl, loss)
            # a loss the slice cannot bear, or (ks = 2: columns 1 and ks-1
            # are one) that is another cell's
            two = loss in ("data2", "data-parity")
            if not sl.bearable(lost) or (two and len(set(lost)) < 2):
                continue
            out += [(name, loss, lay) for lay in LAYOUTS]
    out += [("ec87", f"rows{r}", lay) for r in range(3, 8) for lay in LAYOUTS]
    return out


CELLS = cells()


def test_the_cells_are_the_ones_listed():
    per = {}
    for name, loss, _ in CELLS:
        per.setdefault(name, []).append(loss)
    assert {k: sorted(set(v)) for k, v in per.items()} == {
        "xor3": ["data1", "none"], "ec21": ["data1", "none"],
        "ec32": ["data-parity", "data1", "data2", "none"],
        "ec52": ["data-parity", "data1", "data2", "none"],
        "ec329": ["data-parity", "data1", "data2", "data9", "none"],
        "ec87": ["rows3", "rows4", "rows5", "rows6", "rows7"]}
    assert len(CELLS) == 4 * (2 + 2 + 4 + 4 + 5 + 5)


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    lib = L.lib()
    lib.lizec_chunk_read_batch   # a missing symbol fails here
    return lib, L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def call_read(abi, srcs, rows, tbl, ntables, index, sp, nb, ks, cmap, first,
              count, dp, num_reads, sstride, dstride, engine="abi"):
    """Arguments as numpy arrays or None (= NULL)."""
    lib, eng = abi

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    return lib.lizec_chunk_read_batch(
        eng if engine == "abi" else engine, srcs, rows, ptr(tbl, u8p),
        ntables, ptr(index, u32p), ptr(sp, u64p), ptr(nb, u32p), ks,
        ptr(cmap, u8p), ptr(first, u32p), ptr(count, u32p), ptr(dp, u64p),
        num_reads, sstride, dstride, stream_arg())


class Chunks:
    """Chunks A and B of a slice, cut into parts that lie in one uploaded
    PartStore of a source layout."""

    def __init__(self, sl, sstride, sphase, nchunks=2):
        self.sl, self.n = sl, 2 * sl.ks + 1
        rng = np.random.default_rng(sl.ks * 100 + sl.m)
        self.chunks = [rng.integers(0, 256, (self.n, BLOCK), np.uint8)
                       for _ in range(nchunks)]
        self.store = C.PartStore(
            nchunks * sl.nparts, 4, sstride,
            (lambda i: PHASES[i % 3]) if sphase else None,
            seed=sl.ks + sphase)
        self.where = [[self.store.put(p) for p in sl.cut(ch)]
                      for ch in self.chunks]
        self.dev = torch.from_numpy(self.store.host).cuda()
        self.pristine = self.dev.clone()
        assert self.dev.data_ptr() % 16 == 0

    def add(self, reads, which, lost, first, count, index=0):
        """A read of chunk `which` whose parts `lost` are gone."""
        sl = self.sl
        srcs, cmap, _ = sl.plan(lost)
        reads.add([self.where[which][p] for p in srcs],
                  [sl.count(p, self.n) for p in srcs], cmap, first, count,
                  C.chunk_blocks(self.chunks[which], first, count), index)


_chunks = {}


def chunks_of(name, sstride, sphase):
    """Kept per slice: the layouts of a cell run in a row, and the cells of
    a slice too."""
    if not any(k[0] == name for k in _chunks):
        _chunks.clear()
    key = (name, sstride, sphase)
    if key not in _chunks:
        _chunks[key] = Chunks(SLICES[name], sstride, sphase)
    return _chunks[key]


def six_reads(ch, lost):
    sl, n, ks = ch.sl, ch.n, ch.sl.ks
    _, _, tbl = sl.plan(lost)
    rows = 0 if tbl is None else tbl.size // (32 * sl.srcs)
    reads = C.Reads(sl, rows)
    ch.add(reads, 0, lost, 0, n)
    ch.add(reads, 0, lost, 1, ks + 1)
    ch.add(reads, 0, lost, ks + 1, 1)
    ch.add(reads, 0, lost, ks, 1)
    ch.add(reads, 0, lost, n - 1, ks + 2)
    # read 5: the longest run of columns of row 1 that A has not lost
    gone = [c for c, p in enumerate(sl.cols) if p in lost]
    runs, start = [], 0
    for c in gone + [ks]:
        runs.append((c - start, start))
        start = c + 1
    width, c0 = max(runs)
    assert width >= 1
    reads.add([None if c in gone else ch.where[1][sl.cols[c]]
               for c in range(ks)],
              [0 if c in gone else sl.count(sl.cols[c], n)
               for c in range(ks)],
              [C.UNMAPPED if c in gone else c for c in range(ks)],
              ks + c0, width, ch.chunks[1][ks + c0:ks + c0 + width])
    return reads, tbl


def run_gpu(abi, reads, tbl, ntables, ch, sstride, dstride, dphase,
            use_index=False):
    """One call; returns the output arena as downloaded, compared whole."""
    offs, size = reads.out_layout(
        dstride, (lambda i: PHASES[i % 3]) if dphase else None)
    arena = torch.full((size,), C.FILL, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    sp, nb, cmap, first, count, dp, index = reads.arrays(
        ch.dev.data_ptr(), arena.data_ptr(), offs)
    r = call_read(abi, reads.sl.srcs, reads.rows, tbl, ntables,
                  index if use_index else None, sp, nb, reads.sl.ks, cmap,
                  first, count, dp, len(reads), sstride, dstride)
    assert r == LIZEC_OK
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    want = reads.expected_arena(offs, size, dstride)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        inside = want != C.FILL
        pytest.fail(f"{bad.size} bytes differ, about "
                    f"{int((~inside[bad]).sum())} of them outside every "
                    f"requested block; first at {bad[:6].tolist()}, outputs "
                    f"at {offs}")
    assert torch.equal(ch.dev, ch.pristine), "a source changed"
    return got


@pytest.mark.parametrize("name,loss,layout", CELLS,
                         ids=["-".join(c) for c in CELLS])
def test_read_cell(abi, name, loss, layout):
    (ss, sph), (ds, dph) = LAYOUTS[layout]
    ch = chunks_of(name, ss, sph)
    lost = lost_parts(ch.sl, loss)
    reads, tbl = six_reads(ch, lost)
    assert reads.rows == len([p for p in lost if p in ch.sl.cols])
    run_gpu(abi, reads, tbl, 1 if reads.rows else 0, ch, ss, ds, dph)


def test_standard_copy_is_a_pure_gather(abi):
    """view_parts = 1, srcs = 1, rows = 0, tables NULL."""
    sl = C.Slice("std")
    ch = Chunks(sl, 65540, 4)
    reads = C.Reads(sl, 0)
    for which, f, c in ((0, 0, 3), (1, 1, 2), (0, 2, 3), (1, 1, 1)):
        ch.add(reads, which, (), f, c)
    run_gpu(abi, reads, None, 0, ch, 65540, 65536, 0)


def two_table_reads(ch):
    """ec(3,2): reads that alternate between the tables of two losses, the
    second with one row only."""
    reads, tables = C.Reads(ch.sl, 2), []
    for i, (lost, f, c) in enumerate((((0, 1), 0, 7), ((1, 4), 6, 5),
                                      ((0, 1), 2, 2), ((1, 4), 1, 4))):
        _, _, tbl = ch.sl.plan(lost)
        full = np.zeros(32 * 3 * 2, np.uint8)
        full[:tbl.size] = tbl
        tables.append(full)
        ch.add(reads, i % 2, lost, f, c, index=i % 2)
    return reads, np.concatenate(tables[:2])


def test_a_table_per_read(abi):
    ch = chunks_of("ec32", 65536, 0)
    reads, tables = two_table_reads(ch)
    run_gpu(abi, reads, tables, 2, ch, 65536, 65536, 0, use_index=True)


def test_gpu_and_host_twins_agree(abi):
    """The same arguments, bar the addresses, through both calls."""
    lib, _ = abi
    ch = chunks_of("ec32", 65540, 4)
    reads, tables = two_table_reads(ch)
    six, _ = six_reads(ch, ())
    for r in range(len(six)):
        reads.add(six.src[r], six.nb[r], six.cmap[r], six.first[r],
                  six.count[r], six.expect[r])
    got = run_gpu(abi, reads, tables, 2, ch, 65540, 65552, 4, use_index=True)
    offs, size = reads.out_layout(65552, lambda i: PHASES[i % 3])
    arena = np.full(size + 16, C.FILL, np.uint8)
    skew = -arena.ctypes.data % 16
    sp, nb, cmap, first, count, dp, index = reads.arrays(
        ch.store.host.ctypes.data, arena.ctypes.data + skew, offs)
    assert lib.lizec_chunk_read_host(
        3, 2, tables.ctypes.data_as(u8p), 2, index.ctypes.data_as(u32p),
        sp.ctypes.data_as(u64p), nb.ctypes.data_as(u32p), 3,
        cmap.ctypes.data_as(u8p), first.ctypes.data_as(u32p),
        count.ctypes.data_as(u32p), dp.ctypes.data_as(u64p), len(reads),
        65540, 65552) == LIZEC_OK
    assert np.array_equal(arena[skew:skew + size], got)


def test_refusals_leave_the_arena_alone(abi):
    ch = chunks_of("ec32", 65536, 0)
    reads, tbl = six_reads(ch, (ch.sl.cols[1],))
    offs, size = reads.out_layout()
    arena = torch.full((size,), C.FILL, dtype=torch.uint8, device="cuda")
    base = reads.arrays(ch.dev.data_ptr(), arena.data_ptr(), offs)

    def call(srcs=3, rows=1, tbl=tbl, ntables=1, ks=3, num_reads=6,
             sstride=BLOCK, dstride=BLOCK, engine="abi", **change):
        a = dict(zip(("sp", "nb", "cmap", "first", "count", "dp"),
                     [x.copy() for x in base[:6]]))
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                a[k].reshape(-1)[v[0]] = v[1]
        return call_read(abi, srcs, rows, tbl, ntables, None, a["sp"],
                         a["nb"], ks, a["cmap"], a["first"], a["count"],
                         a["dp"], num_reads, sstride, dstride, engine)

    refused = {
        "engine NULL": dict(engine=None),
        "source address 0 with a count": dict(sp=(1, 0)),
        "source address 2 mod 4": dict(sp=(0, int(base[0][0, 0]) + 2)),
        "source count above 32768": dict(nb=(0, 32769)),
        "source stride 65538": dict(sstride=65538),
        "destination stride 65532": dict(dstride=65532),
        "tables NULL at rows 1": dict(tbl=None),
        "ntables 0": dict(ntables=0),
        "view_parts 33": dict(ks=33),
        "srcs 0": dict(srcs=0),
        "rows 33": dict(rows=33),
        "col_map names slot 3": dict(cmap=(0, 3)),
        "col_map names row 1": dict(cmap=(1, 0x81)),
        "col_map names a slot twice": dict(cmap=(2, 0)),
        "a requested column unmapped": dict(cmap=(0, 0xFF)),
        "a requested column's slot has address 0": dict(sp=(0, 0),
                                                        nb=(0, 0)),
        "block_count 0": dict(count=(1, 0)),
        "past block 1048576": dict(first=(1, 1048575)),
        "destination address 0": dict(dp=(0, 0)),
        "destination address 2 mod 4": dict(dp=(3, int(base[5][3]) + 2)),
        "col_map NULL": dict(cmap=None),
        "dst_dptrs NULL": dict(dp=None),
        "num_reads 0": dict(num_reads=0),
    }
    for what, change in refused.items():
        assert call(**change) == LIZEC_EINVAL, what
    torch.cuda.synchronize()
    assert bool((arena == C.FILL).all())
    # and the call they are one change away from
    assert call() == LIZEC_OK
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(),
                          reads.expected_arena(offs, size))


@pytest.mark.parametrize("kind", [("ec", 3, 2), ("xor", 3)],
                         ids=["ec32", "xor3"])
def test_read_chunks_through_python(kind):
    """read_chunks: three chunks of different lengths, a range, a loss each;
    out = None, then into rows at dst_stride 65540 whose gaps survive."""
    from lizardfs_amd import chunkread
    from lizardfs_amd import slice_traits as st
    sl = C.Slice(*kind)
    t = st.ec_slice_type(3, 2) if kind[0] == "ec" else st.K_XOR2 + 1
    rng = np.random.default_rng(11)
    ns, S = [7, 4, 2], 3
    chunks = [rng.integers(0, 256, (n, BLOCK), np.uint8) for n in ns]
    cut = [sl.cut(c) for c in chunks]
    frags = []
    for p in range(sl.nparts):
        f = rng.integers(0, 256, (S, 4 * BLOCK), np.uint8)
        for s in range(S):
            f[s, :cut[s][p].size] = cut[s][p].reshape(-1)
        frags.append(torch.from_numpy(f).cuda())
    first, count = [0, 1, 1], [7, 3, 4]
    erased = [{1, 2}, {0}, set()] if kind[0] == "ec" else [{2}, {0}, set()]
    want = [C.chunk_blocks(chunks[s], first[s], count[s]) for s in range(S)]
    got = chunkread.read_chunks(t, frags, ns, first, count, erased=erased)
    assert got.shape == (S, 7 * BLOCK)
    got = got.cpu().numpy()
    for s in range(S):
        assert np.array_equal(got[s, :count[s] * BLOCK].reshape(-1, BLOCK),
                              want[s])
    out = torch.full((S, 4 + 7 * 65540), C.FILL, dtype=torch.uint8,
                     device="cuda")
    ret = chunkread.read_chunks(t, frags, ns, first, count, erased=erased,
                                out=out[:, 4:], dst_stride=65540)
    assert ret.data_ptr() == out.data_ptr() + 4
    exp = np.full((S, 4 + 7 * 65540), C.FILL, np.uint8)
    for s in range(S):
        for i in range(count[s]):
            exp[s, 4 + i * 65540:4 + i * 65540 + BLOCK] = want[s][i]
    assert np.array_equal(out.cpu().numpy(), exp)
    for f, h in zip(frags, cut[0]):
        assert np.array_equal(f[0, :h.size].cpu().numpy(), h.reshape(-1))
