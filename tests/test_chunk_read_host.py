"""The chunk read without a GPU: lizec_chunk_read_host through the C ABI and
read_chunks_host through lizardfs_amd.chunkread, bit-exact against the chunk
that the parts were cut from (chunk_read_cases.py); plan_read against cases
derived by hand from the reference; every refusal of the call and every
ValueError of the Python layer.

Every part lies in a buffer of random bytes with a random block behind its
own count, so a read past a count changes the result.  The outputs of a call
lie in one arena of 0xA5, each between 256-byte canaries; the whole arena and
the sources are compared after each call.

test_every_range runs, for every slice and every chunk length n in
1..(2k+1), every (first_block, block_count) range inside the chunk.  The loss
patterns (none, every single part, for m = 2 every pair) are dealt round the
ranges in turn, so each range is read once and each pattern meets ranges of
every shape; on top of that every pattern reads the whole chunk at every n,
and [1, k+2) at n = 2k+1.  The full product of ranges and patterns would be
some 60000 reads of ec(8,2) alone; dealt like this the file takes about ten
seconds.  All reads of one (n, pattern) are one call.
"""
import ctypes

import numpy as np
import pytest

import chunk_read_cases as C
from lizardfs_amd import chunkread
from lizardfs_amd import lib as L
from lizardfs_amd import slice_traits as st

BLOCK = C.BLOCK
LIZEC_OK, LIZEC_EINVAL = 0, -2
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

SLICES = [C.Slice("std"), C.Slice("xor", 2), C.Slice("xor", 3),
          C.Slice("xor", 9), C.Slice("ec", 2, 1), C.Slice("ec", 3, 2),
          C.Slice("ec", 5, 1), C.Slice("ec", 8, 2)]


def slice_type(sl):
    if sl.kind[0] == "std":
        return st.K_STANDARD
    if sl.kind[0] == "xor":
        return st.K_XOR2 + sl.kind[1] - 2
    return st.ec_slice_type(sl.kind[1], sl.kind[2])


def host_call(srcs, rows, tbl, ntables, index, sp, nb, ks, cmap, first,
              count, dp, num_reads, sstride=BLOCK, dstride=BLOCK):
    """Arguments as numpy arrays or None (= NULL)."""
    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    return L.lib().lizec_chunk_read_host(
        srcs, rows, ptr(tbl, u8p), ntables, ptr(index, u32p), ptr(sp, u64p),
        ptr(nb, u32p), ks, ptr(cmap, u8p), ptr(first, u32p),
        ptr(count, u32p), ptr(dp, u64p), num_reads, sstride, dstride)


def run_reads(reads, store, tbl, what):
    """One host call over `reads`; the output arena and the part store are
    compared whole."""
    offs, size = reads.out_layout()
    arena = np.full(size, C.FILL, np.uint8)
    before = store.host.copy()
    sp, nb, cmap, first, count, dp, index = reads.arrays(
        store.host.ctypes.data, arena.ctypes.data, offs)
    r = host_call(reads.sl.srcs, reads.rows, tbl, 1 if reads.rows else 0,
                  None, sp, nb, reads.sl.ks, cmap, first, count, dp,
                  len(reads))
    assert r == LIZEC_OK, what
    assert np.array_equal(store.host, before), f"{what}: a source changed"
    want = reads.expected_arena(offs, size)
    if not np.array_equal(arena, want):
        bad = np.flatnonzero(arena != want)
        pytest.fail(f"{what}: {bad.size} bytes differ, first at "
                    f"{bad[:4].tolist()} (output offsets {offs[:4]})")


def python_reads(sl, parts, n, lost, ranges, chunk, what):
    """The same ranges through read_chunks_host: the chunk stands in every
    row of the batch (row stride 0), one range per row."""
    rng = np.random.default_rng(n)
    frags = []
    for p in range(sl.nparts):
        if p in lost:
            frags.append(None)
            continue
        row = np.concatenate([parts[p].reshape(-1),
                              rng.integers(0, 256, BLOCK, np.uint8)])
        frags.append(np.broadcast_to(row[None, :], (len(ranges), row.size)))
    got = chunkread.read_chunks_host(
        slice_type(sl), frags, [n] * len(ranges), [f for f, _ in ranges],
        [c for _, c in ranges])
    for i, (f, c) in enumerate(ranges):
        assert np.array_equal(got[i, :c * BLOCK].reshape(c, BLOCK),
                              C.chunk_blocks(chunk, f, c)), f"{what} {f}+{c}"
        assert not got[i, c * BLOCK:].any()


@pytest.mark.parametrize("sl", SLICES, ids=lambda s: s.name)
def test_every_range(sl):
    rng = np.random.default_rng(sl.ks * 10 + sl.m)
    losses = sl.losses()
    top = 2 * sl.ks + 1
    for n in range(1, top + 1):
        chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
        parts = sl.cut(chunk)
        store = C.PartStore(sl.nparts, -(-n // sl.ks) + 1, seed=n)
        where = [store.put(p) for p in parts]
        ranges = [(f, c) for f in range(n) for c in range(1, n - f + 1)]
        dealt = {lost: [] for lost in losses}
        for i, r in enumerate(ranges):
            dealt[losses[i % len(losses)]].append(r)
        for lost in losses:
            dealt[lost].append((0, n))
            if n == top:
                dealt[lost].append((1, sl.ks + 1))
        for lost, rs in dealt.items():
            if not rs:
                continue
            srcs, cmap, tbl = sl.plan(lost)
            rows = 0 if tbl is None else tbl.size // (32 * sl.srcs)
            reads = C.Reads(sl, rows)
            for f, c in rs:
                reads.add([where[p] for p in srcs],
                          [sl.count(p, n) for p in srcs], cmap, f, c,
                          C.chunk_blocks(chunk, f, c))
            what = f"{sl.name} n={n} lost={lost}"
            run_reads(reads, store, tbl, what)
            python_reads(sl, parts, n, lost, rs, chunk, what)


def test_past_the_end_strides_and_two_tables():
    """What test_every_range leaves out: blocks past the chunk's end, both
    strides above 65536 with the gaps left alone, a table per read, an
    unused slot of address 0 and an unmapped column."""
    sl = C.Slice("ec", 3, 2)
    rng = np.random.default_rng(77)
    n = 7
    chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    sstride, dstride = 65540, 65552
    store = C.PartStore(sl.nparts, 5, stride=sstride,
                        phase=lambda i: (4, 8, 12)[i % 3], seed=3)
    where = [store.put(p) for p in parts]
    reads = C.Reads(sl, 2)
    tables = []
    for i, (lost, f, c) in enumerate((((0, 1), 0, 7), ((1, 4), 6, 5),
                                      ((0, 1), 2, 2))):
        srcs, cmap, tbl = sl.plan(lost)
        full = np.zeros(32 * 3 * 2, np.uint8)
        full[:tbl.size] = tbl
        tables.append(full)
        reads.add([where[p] for p in srcs], [sl.count(p, n) for p in srcs],
                  cmap, f, c, C.chunk_blocks(chunk, f, c), index=i % 2)
    tables = np.concatenate(tables[:2])
    # healthy, one block of column 2: the other slots unused, address 0
    reads.add([None, None, where[2]], [0, 0, sl.count(2, n)],
              [C.UNMAPPED, C.UNMAPPED, 2], 5, 1, chunk[5:6])
    offs, size = reads.out_layout(dstride, lambda i: (12, 4, 8)[i % 3])
    arena = np.full(size, C.FILL, np.uint8)
    before = store.host.copy()
    sp, nb, cmap, first, count, dp, index = reads.arrays(
        store.host.ctypes.data, arena.ctypes.data, offs)
    assert host_call(3, 2, tables, 2, index, sp, nb, 3, cmap, first, count,
                     dp, len(reads), sstride, dstride) == LIZEC_OK
    assert np.array_equal(store.host, before)
    assert np.array_equal(arena, reads.expected_arena(offs, size, dstride))


# ---- plan_read -------------------------------------------------------------

STD = st.K_STANDARD
XOR3 = st.K_XOR2 + 1
EC32 = st.ec_slice_type(3, 2)
U = chunkread.UNMAPPED
X = chunkread.LOST


def test_plan_read_by_hand():
    """getRequiredParts (chunk_read_planner.h:182-206): block_count >= k
    needs every data part, fewer blocks the parts of columns (first + i) % k.
    isReadingPossible (slice_read_planner.cc:46-51): all of those there, or
    any k parts.  The degraded ec plan reads the first k available parts
    (ec_read_plan.h:126-133), the xor one all the others."""
    plan = chunkread.plan_read
    # standard: one column, one part
    assert plan(STD, [0], 3, 2) == ([0], [0], [])
    assert plan(STD, [], 0, 1) is None
    # ec(3,2), all there: a whole row needs parts 0..2 and no parity
    assert plan(EC32, range(5), 0, 3) == ([0, 1, 2], [0, 1, 2], [])
    # blocks 4, 5 are columns 1, 2: part 0 is not read
    assert plan(EC32, range(5), 4, 2) == ([1, 2], [U, 0, 1], [])
    # blocks 5, 6 are columns 2, 0: asked for in that order, read ascending
    assert plan(EC32, [0, 2], 5, 2) == ([0, 2], [0, U, 1], [])
    # part 1 gone but not required
    assert plan(EC32, [0, 2, 3, 4], 5, 2) == ([0, 2], [0, U, 1], [])
    # part 1 gone and required: the first three of 0, 2, 3, 4
    assert plan(EC32, [0, 2, 3, 4], 0, 3) == ([0, 2, 3], [0, X, 1], [1])
    assert plan(EC32, [0, 2, 3, 4], 4, 1) == ([0, 2, 3], [0, X, 1], [1])
    # two data parts gone; only the required one is rebuilt
    assert plan(EC32, [2, 3, 4], 0, 7) == ([2, 3, 4], [X, X + 1, 0], [0, 1])
    assert plan(EC32, [2, 3, 4], 1, 1) == ([2, 3, 4], [U, X, 0], [1])
    # a data and a parity part gone
    assert plan(EC32, [0, 1, 4], 0, 3) == ([0, 1, 4], [0, 1, X], [2])
    # two parts are not enough, unless they are the required ones
    assert plan(EC32, [0, 4], 0, 3) is None
    assert plan(EC32, [0, 4], 3, 1) == ([0], [0, U, U], [])
    # xor3: columns are parts 1..3, the parity is part 0
    assert plan(XOR3, [0, 1, 2, 3], 0, 3) == ([1, 2, 3], [0, 1, 2], [])
    assert plan(XOR3, [1, 2, 3], 1, 2) == ([2, 3], [U, 0, 1], [])
    assert plan(XOR3, [0, 1, 3], 0, 3) == ([0, 1, 3], [1, X, 2], [2])
    assert plan(XOR3, [0, 1, 3], 3, 1) == ([1], [0, U, U], [])
    assert plan(XOR3, [0, 3], 1, 1) is None
    assert plan(XOR3, [0, 3], 2, 1) == ([3], [U, U, 0], [])
    for bad in ((st.K_TAPE, [0], 0, 1), (EC32, [5], 0, 1), (EC32, [0], 0, 0),
                (EC32, [0], -1, 1)):
        with pytest.raises(ValueError):
            plan(*bad)


# ---- refusals ----------------------------------------------------------------

def test_refusals_write_nothing():
    sl = C.Slice("ec", 3, 2)
    n = 7
    chunk = np.random.default_rng(5).integers(0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    store = C.PartStore(sl.nparts, 4, seed=9)
    where = [store.put(p) for p in parts]
    srcs, cmap, tbl = sl.plan((1,))
    reads = C.Reads(sl, 1)
    for f, c in ((0, 7), (4, 2)):
        reads.add([where[p] for p in srcs], [sl.count(p, n) for p in srcs],
                  cmap, f, c, C.chunk_blocks(chunk, f, c))
    offs, size = reads.out_layout()
    arena = np.full(size, C.FILL, np.uint8)
    base = reads.arrays(store.host.ctypes.data, arena.ctypes.data, offs)

    def call(srcs=3, rows=1, tbl=tbl, ntables=1, index="keep", ks=3,
             num_reads=2, sstride=BLOCK, dstride=BLOCK, **change):
        a = dict(zip(("sp", "nb", "cmap", "first", "count", "dp", "index"),
                     [x.copy() for x in base]))
        for k, v in change.items():
            if callable(v):
                v(a[k])
            else:
                a[k] = v
        if not isinstance(index, str):
            a["index"] = index
        return host_call(srcs, rows, tbl, ntables, a["index"], a["sp"],
                         a["nb"], ks, a["cmap"], a["first"], a["count"],
                         a["dp"], num_reads, sstride, dstride)

    def set_(i, v):
        def f(a):
            a.reshape(-1)[i] = v
        return f

    refused = {
        # what the ragged call refuses about sources, tables and strides
        "source address 0 with a count": dict(sp=set_(1, 0)),
        "source address 2 mod 4": dict(sp=lambda a: a.__iadd__(2)),
        "source count above 32768": dict(nb=set_(0, 32769)),
        "source stride 65538": dict(sstride=65538),
        "source stride 65532": dict(sstride=65532),
        "destination stride 65538": dict(dstride=65538),
        "destination stride 65532": dict(dstride=65532),
        "ntables 0": dict(ntables=0),
        "tables NULL at rows 1": dict(tbl=None),
        "tbl_index 1 of 1": dict(index=np.array([0, 1], np.uint32)),
        "ntables beyond 2^30 bytes": dict(ntables=(1 << 30) // 96 + 1),
        # the call's own
        "view_parts 0": dict(ks=0),
        "view_parts 33": dict(ks=33),
        "srcs 0": dict(srcs=0),
        "srcs 33": dict(srcs=33),
        "rows -1": dict(rows=-1),
        "rows 33": dict(rows=33),
        "col_map names slot 3": dict(cmap=set_(0, 3)),
        "col_map names slot 0x7f": dict(cmap=set_(0, 0x7F)),
        "col_map names row 1": dict(cmap=set_(1, 0x81)),
        "col_map names row 0x7e": dict(cmap=set_(1, 0xFE)),
        "col_map names a slot twice": dict(cmap=set_(2, 0)),
        "col_map names a row twice": dict(cmap=set_(2, 0x80)),
        "a requested column unmapped": dict(cmap=set_(0, 0xFF)),
        "a requested column unmapped, short range": dict(cmap=set_(5, 0xFF)),
        "a requested column's slot has address 0": dict(
            sp=set_(0, 0), nb=set_(0, 0)),
        "block_count 0": dict(count=set_(1, 0)),
        "past block 1048576": dict(first=set_(1, 1048575)),
        "first_block + block_count wraps": dict(first=set_(1, 0xFFFFFFFF)),
        "destination address 0": dict(dp=set_(0, 0)),
        "destination address 2 mod 4": dict(dp=lambda a: a.__iadd__(2)),
        "src_dptrs NULL": dict(sp=None),
        "src_nblocks NULL": dict(nb=None),
        "col_map NULL": dict(cmap=None),
        "first_block NULL": dict(first=None),
        "block_count NULL": dict(count=None),
        "dst_dptrs NULL": dict(dp=None),
        "num_reads 0": dict(num_reads=0),
        "num_reads -1": dict(num_reads=-1),
    }
    for what, change in refused.items():
        assert call(**change) == LIZEC_EINVAL, what
        assert (arena == C.FILL).all(), what
    # the call that all of the above are one change away from (tbl_index
    # NULL = table 0; an unmapped column and a slot of address 0 that no
    # block needs are in test_past_the_end_strides_and_two_tables)
    assert call(index=None) == LIZEC_OK
    assert np.array_equal(arena, reads.expected_arena(offs, size))


def test_a_row_map_beyond_the_grid_is_refused():
    """2^31 / 8 block rows: 2^20 one-column reads of 256 rows each.  The
    check runs before any address is used, so the sources are one count-0
    slot and the destinations an address that is never written."""
    R = (1 << 20) + 1
    sp, nb = np.zeros(R, np.uint64), np.zeros(R, np.uint32)
    cmap = np.zeros(R, np.uint8)
    first, count = np.zeros(R, np.uint32), np.full(R, 256, np.uint32)
    probe = np.full(16, C.FILL, np.uint8)
    dp = np.full(R, probe.ctypes.data // 16 * 16 + 16, np.uint64)
    sp[:] = dp[0]
    assert host_call(1, 0, None, 0, None, sp, nb, 1, cmap, first, count, dp,
                     R) == LIZEC_EINVAL
    assert (probe == C.FILL).all()


def test_argument_errors_need_no_library(monkeypatch):
    def no_call(*a, **kw):
        raise AssertionError("the library was used")
    monkeypatch.setattr(L, "lib", no_call)
    monkeypatch.setattr(L, "engine", no_call)
    S, cb = 3, [1, 4, 7]
    frag = np.zeros((S, 3 * BLOCK), np.uint8)
    f5 = [frag] * 5

    def refused(*a, **kw):
        with pytest.raises(ValueError):
            chunkread.read_chunks_host(*a, **kw)

    refused(st.K_TAPE, [frag], cb, 0, 1)
    refused(EC32, f5, [0, 4, 7], 0, 1)
    refused(EC32, f5, [1, 4, 1025], 0, 1)
    refused(EC32, f5, [cb], 0, 1)
    refused(EC32, f5, [1.0, 4.0, 7.0], 0, 1)
    refused(EC32, f5, [], 0, 1)
    refused(EC32, f5[:4], cb, 0, 1)                     # k+m fragment slots
    refused(XOR3, [frag] * 3, cb, 0, 1)                 # N+1 of them
    refused(EC32, f5, cb, 0, 0)                         # empty range
    refused(EC32, f5, cb, -1, 1)
    refused(EC32, f5, cb, 1000, 25)                     # past block 1024
    refused(EC32, f5, cb, [0, 1], 1)                    # one value per chunk
    refused(EC32, f5, cb, 0, [1, 1, 1, 1])
    refused(EC32, f5, cb, 0.0, 1)
    refused(EC32, f5, cb, 0, 1, src_stride=65538)
    refused(EC32, f5, cb, 0, 1, src_stride=65532)
    refused(EC32, f5, cb, 0, 1, dst_stride=65538)
    refused(EC32, f5, cb, 0, 1, dst_stride=65532)
    refused(EC32, f5, cb, 0, 3, erased={5})
    refused(EC32, f5, cb, 0, 3, erased=[{0}, {1}])      # one set per chunk
    refused(EC32, f5, cb, 0, 3, erased={0, 1, 2})       # unreadable
    refused(EC32, [None, frag, frag, None, frag], cb, 0, 3, erased={1})
    refused(XOR3, [frag, None, frag, frag], cb, 0, 3, erased={2})
    refused(STD, [None], cb, 0, 1)
    refused(EC32, f5, cb, 0, 3, erased=[{0}, {1}, {0, 1, 2}])
    # the fragments themselves
    refused(EC32, [frag[:2]] * 5, cb, 0, 3)             # rows
    refused(EC32, [frag[:, :BLOCK]] * 5, cb, 0, 3)      # 3 blocks needed
    refused(EC32, [frag[:, 1:]] * 5, [1, 1, 1], 0, 1)   # alignment
    refused(EC32, [frag[:, ::2]] * 5, [1, 1, 1], 0, 1)  # contiguous rows
    refused(EC32, [frag.astype(np.int8)] * 5, cb, 0, 3)
    refused(EC32, f5, cb, 0, 3, out=np.zeros((S, BLOCK), np.uint8))
    refused(EC32, f5, cb, 0, 3, out=np.zeros((2, 3 * BLOCK), np.uint8))
    # read_chunks: the same checks, then tensors that are not on a GPU
    torch = pytest.importorskip("torch")
    t5 = [torch.zeros((S, 3 * BLOCK), dtype=torch.uint8)] * 5
    for a, kw in (((EC32, t5, cb, 0, 0), {}),
                  ((EC32, t5, cb, 0, 3), dict(erased={0, 1, 2})),
                  ((EC32, t5, cb, 0, 3), dict(dst_stride=65538)),
                  ((EC32, t5, cb, 0, 3), {}),
                  ((EC32, f5, cb, 0, 3), {})):
        with pytest.raises(ValueError):
            chunkread.read_chunks(*a, **kw)


def test_symbols_are_exported():
    lib = L.lib()
    for name in ("lizec_chunk_read_batch", "lizec_chunk_read_host",
                 "lizec_impl_chunk_read_check"):
        assert getattr(lib, name) is not None
    assert chunkread.LOST == C.LOST and chunkread.UNMAPPED == C.UNMAPPED
