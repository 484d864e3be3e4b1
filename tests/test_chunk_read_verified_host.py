"""The verified chunk read without a GPU: lizec_chunk_read_verified_host
through the C ABI and read_chunks_verified_host through lizardfs_amd.chunkread.

Every comparison is bit-exact.  Outputs are compared with what
lizec_chunk_read_host writes for the same arguments (and, where the sources
are clean, with the chunk the parts were cut from); masks with
chunk_read_verified_cases.expected_mask, the load rule written down a second
time.  The outputs of a call lie in one arena of 0xA5 between 256-byte
canaries; the arena and the sources are compared whole after each call.

A corruption is always one byte XORed with a non-zero value: a burst of at
most 8 bits always changes a CRC-32, so no case depends on chance.

test_clean deals the loss patterns round the ranges as test_chunk_read_host
does (every range is read once, every pattern meets ranges of every shape,
and every pattern reads the whole chunk at every length).
"""
import ctypes

import numpy as np
import pytest

import chunk_read_cases as C
import chunk_read_verified_cases as V
from lizardfs_amd import chunkread
from lizardfs_amd import lib as L
from lizardfs_amd import slice_traits as st

BLOCK = C.BLOCK
LIZEC_OK, LIZEC_EINVAL = 0, -2
POISON = 0xDEADBEEF
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)

SLICES = [C.Slice("std"), C.Slice("xor", 3), C.Slice("ec", 2, 1),
          C.Slice("ec", 3, 2), C.Slice("ec", 8, 2)]


def slice_type(sl):
    if sl.kind[0] == "std":
        return st.K_STANDARD
    if sl.kind[0] == "xor":
        return st.K_XOR2 + sl.kind[1] - 2
    return st.ec_slice_type(sl.kind[1], sl.kind[2])


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def plain_call(srcs, rows, tbl, ntables, index, sp, nb, ks, cmap, first,
               count, dp, num_reads, sstride, dstride):
    return L.lib().lizec_chunk_read_host(
        srcs, rows, ptr(tbl, u8p), ntables, ptr(index, u32p), ptr(sp, u64p),
        ptr(nb, u32p), ks, ptr(cmap, u8p), ptr(first, u32p),
        ptr(count, u32p), ptr(dp, u64p), num_reads, sstride, dstride)


def verified_call(srcs, rows, tbl, ntables, index, sp, nb, ks, cmap, first,
                  count, dp, num_reads, sstride, dstride, cp, cstride, bad):
    return L.lib().lizec_chunk_read_verified_host(
        srcs, rows, ptr(tbl, u8p), ntables, ptr(index, u32p), ptr(sp, u64p),
        ptr(nb, u32p), ks, ptr(cmap, u8p), ptr(first, u32p),
        ptr(count, u32p), ptr(dp, u64p), num_reads, sstride, dstride,
        ptr(cp, u64p), cstride,
        None if bad is None else ctypes.c_void_p(bad.ctypes.data))


def run_both(reads, store, tbl, what, ntables=None, use_index=False,
             dstride=BLOCK):
    """One verified and one plain host call over `reads`: the arenas must be
    equal and the sources unchanged.  Returns (masks, arena)."""
    offs, size = reads.out_layout(dstride)
    arenas = [np.full(size, C.FILL, np.uint8) for _ in range(2)]
    before = store.data.copy(), store.crc.copy()
    if ntables is None:
        ntables = 1 if reads.rows else 0
    bad = np.full(len(reads), POISON, np.uint32)
    for verified, arena in zip((True, False), arenas):
        sp, nb, cmap, first, count, dp, index = reads.arrays(
            store.data.ctypes.data, arena.ctypes.data, offs)
        args = (reads.sl.srcs, reads.rows, tbl, ntables,
                index if use_index else None, sp, nb, reads.sl.ks, cmap,
                first, count, dp, len(reads), store.stride, dstride)
        if verified:
            r = verified_call(*args, reads.crc_ptrs(store.crc.ctypes.data),
                              store.crc_stride, bad)
        else:
            r = plain_call(*args)
        assert r == LIZEC_OK, what
    assert np.array_equal(store.data, before[0]), f"{what}: a source changed"
    assert np.array_equal(store.crc, before[1]), f"{what}: a CRC changed"
    assert np.array_equal(arenas[0], arenas[1]), \
        f"{what}: the verified read wrote other bytes than the plain one"
    return bad, arenas[0]


def masks_of(reads, bad_blocks):
    """bad_blocks[i]: the corrupt (slot, block) pairs of read i."""
    return np.array([V.expected_mask(reads.sl.ks, reads.cmap[i], reads.nb[i],
                                     reads.first[i], reads.count[i],
                                     reads.crc[i], bad_blocks[i])
                     for i in range(len(reads))], np.uint32)


# ---- clean ---------------------------------------------------------------------

@pytest.mark.parametrize("sl", SLICES, ids=lambda s: s.name)
def test_clean(sl):
    rng = np.random.default_rng(sl.ks * 10 + sl.m + 1)
    losses = sl.losses()
    top = 2 * sl.ks + 1
    for n in range(1, top + 1):
        chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
        parts = sl.cut(chunk)
        inline = n % 2 == 0
        store = V.VerifiedStore(sl.nparts, -(-n // sl.ks) + 1,
                                "inline" if inline else "array", seed=n,
                                phase=(lambda i: 4) if inline else None,
                                odd=n % 4 == 1)
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
            srcs, cmap, tbl = sl.plan(lost)
            rows = 0 if tbl is None else tbl.size // (32 * sl.srcs)
            reads = V.VReads(sl, rows)
            for f, c in rs:
                reads.add([where[p][0] for p in srcs],
                          [sl.count(p, n) for p in srcs], cmap, f, c,
                          C.chunk_blocks(chunk, f, c),
                          crc_offs=[where[p][1] for p in srcs])
            what = f"{sl.name} n={n} lost={lost}"
            bad, arena = run_both(reads, store, tbl, what)
            assert not bad.any(), what
            offs, size = reads.out_layout()
            assert np.array_equal(arena, reads.expected_arena(offs, size)), \
                what


# ---- every single corrupted block ------------------------------------------------

def corruption_reads(sl, store, where, chunk, n):
    """Reads of one chunk of n = 2k+1 blocks that between them meet every
    branch of the load rule; every slot verified."""
    ks = sl.ks
    reads, tables = V.VReads(sl, sl.m if sl.kind[0] == "ec" else 1), []
    lost1 = (sl.cols[1],)
    both = (sl.cols[1], sl.parity[0])
    shapes = [((), 0, n),            # healthy: parities never read
              ((), 1, ks + 1),       # healthy, clipped head and tail rows
              ((), ks + 2, 1),       # healthy: one column of row 1 alone
              ((), 2 * ks, 1),       # the short last row alone
              (lost1, 0, n),         # degraded: every present slot of a row
              (lost1, ks, 1),        # degraded, copy-only row
              (lost1, ks + 1, 1),    # degraded, recover-only row
              (lost1, n - 1, ks + 2)]   # past the chunk's end
    if sl.bearable(both):
        shapes.append((both, 1, ks + 1))
    index = {}
    for lost, f, c in shapes:
        srcs, cmap, tbl = sl.plan(lost)
        if tbl is not None and lost not in index:
            full = np.zeros(32 * sl.srcs * reads.rows, np.uint8)
            full[:tbl.size] = tbl
            index[lost] = len(tables)
            tables.append(full)
        reads.add([where[p][0] for p in srcs],
                  [sl.count(p, n) for p in srcs], cmap, f, c,
                  C.chunk_blocks(chunk, f, c), index.get(lost, 0),
                  crc_offs=[where[p][1] for p in srcs])
        reads.parts = getattr(reads, "parts", []) + [srcs]
    return reads, np.concatenate(tables), len(tables)


@pytest.mark.parametrize("layout", ["array", "inline"])
@pytest.mark.parametrize("sl", [C.Slice("ec", 3, 2), C.Slice("xor", 3)],
                         ids=lambda s: s.name)
def test_every_single_corrupted_block(sl, layout):
    n = 2 * sl.ks + 1
    chunk = np.random.default_rng(40 + sl.m).integers(
        0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    room = max(p.shape[0] for p in parts) + 1
    store = V.VerifiedStore(sl.nparts, room, layout, seed=6,
                            phase=(lambda i: 4) if layout == "inline"
                            else None)
    where = [store.put(p) for p in parts]
    reads, tables, nt = corruption_reads(sl, store, where, chunk, n)
    bad, _ = run_both(reads, store, tables, "clean", nt, True)
    assert not bad.any()
    seen = set()
    for p in range(sl.nparts):
        for b in range(room):
            # data bytes 0, 65535 and an interior one, then a CRC byte
            spots = [(store.data, where[p][0] + b * store.stride + o)
                     for o in (0, BLOCK - 1, 4097 * (b + 1) + p)]
            spots.append((store.crc,
                          where[p][1] + b * store.crc_stride + (p + b) % 4))
            for buf, at in spots:
                buf[at] ^= 0x10 | (p + 1)
                blocks = [[(srcs.index(p), b)] if p in srcs else []
                          for srcs in reads.parts]
                want = masks_of(reads, blocks)
                what = f"part {p} block {b} byte {at}"
                got, _ = run_both(reads, store, tables, what, nt, True)
                buf[at] ^= 0x10 | (p + 1)
                assert np.array_equal(got, want), \
                    f"{what}: {got.tolist()} != {want.tolist()}"
                seen.update((i, p, b, bool(m)) for i, m in enumerate(want))
    # the cases that must stay silent, and that some read is flagged at all
    count = [parts[p].shape[0] for p in range(sl.nparts)]
    par = sl.parity[0]
    assert (0, par, 0, False) in seen          # a parity block, healthy read
    assert (2, sl.cols[0], 0, False) in seen   # a row the range does not touch
    assert (2, sl.cols[0], 1, False) in seen   # an unrequested column
    assert all((i, p, count[p], False) in seen  # at the part's count
               for i in range(len(reads)) for p in range(sl.nparts)
               if p in reads.parts[i])
    assert (4, par, 0, True) in seen and (0, sl.cols[0], 0, True) in seen
    assert (5, par, 1, False) in seen          # copy-only row reads no parity
    assert (6, par, 1, True) in seen and (6, sl.cols[0], 1, True) in seen


def test_the_load_rule_by_hand():
    """ec(3,2), n = 7: part 0 has blocks 0..2, parts 1, 2 have 0..1."""
    ld = V.loads
    healthy, nb = [0, 1, 2], [3, 2, 2]
    assert ld(3, healthy, nb, 0, 7, 0, 2) and not ld(3, healthy, nb, 0, 7, 1, 2)
    assert ld(3, healthy, nb, 4, 1, 1, 1)
    assert not ld(3, healthy, nb, 4, 1, 0, 1)     # unrequested column
    assert not ld(3, healthy, nb, 4, 1, 1, 0)     # untouched row
    # part 1 lost: slots are parts 0, 2, 3
    deg, nb = [0, C.LOST, 1], [3, 2, 3]
    assert all(ld(3, deg, nb, 4, 1, j, 1) for j in range(3))
    assert ld(3, deg, nb, 3, 1, 0, 1)             # copy-only row: slot 0 ...
    assert not ld(3, deg, nb, 3, 1, 1, 1)         # ... and nothing else
    assert not ld(3, deg, nb, 3, 1, 2, 1)
    assert not ld(3, deg, nb, 0, 7, 1, 2)         # past the part's count


# ---- several bad slots, an unverified slot, an odd CRC address -----------------------

@pytest.mark.parametrize("layout,odd", [("array", False), ("array", True),
                                        ("inline", False)])
def test_several_bad_slots_in_one_read(layout, odd):
    sl = C.Slice("ec", 3, 2)
    n = 7
    chunk = np.random.default_rng(8).integers(0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    store = V.VerifiedStore(sl.nparts, 4, layout, seed=2, odd=odd,
                            phase=(lambda i: 4) if layout == "inline"
                            else None)
    where = [store.put(p) for p in parts]
    if odd:
        assert all((store.crc.ctypes.data + w[1]) % 2 == 1 for w in where)
    srcs, cmap, tbl = sl.plan((1,))          # slots: parts 0, 2, 3
    reads = V.VReads(sl, 1)

    def add(f, c, verify=(True, True, True)):
        reads.add([where[p][0] for p in srcs],
                  [sl.count(p, n) for p in srcs], cmap, f, c,
                  C.chunk_blocks(chunk, f, c),
                  crc_offs=[where[p][1] if v else None
                            for p, v in zip(srcs, verify)])

    add(0, n)                                # slots 0, 1 and 2 bad
    add(0, n, (True, False, True))           # slot 1 unverified
    add(0, n, (False, False, False))         # nothing verified
    add(3, 1)                                # copy-only row 1: slot 0 alone
    add(6, 1)                                # row 2: only part 0's block 2
    for p, b, o in ((0, 1, 5), (2, 0, 0), (2, 1, BLOCK - 1), (3, 1, 77)):
        store.data[where[p][0] + b * store.stride + o] ^= 0xFF
    bad, _ = run_both(reads, store, tbl, "several")
    # parts 0 (block 1), 2 (blocks 0, 1) and 3 (block 1) are slots 0, 1, 2
    assert bad.tolist() == [0b111, 0b101, 0, 0b001, 0]


# ---- the Python rounds ---------------------------------------------------------------

def py_parts(sl, ns, inline=False, seed=3):
    """(chunks, fragments, crcs) for read_chunks_verified_host: S chunks of
    ns blocks, every part with a random block behind the longest count."""
    rng = np.random.default_rng(seed)
    S = len(ns)
    chunks = [rng.integers(0, 256, (n, BLOCK), np.uint8) for n in ns]
    cut = [sl.cut(c) for c in chunks]
    room = -(-max(ns) // sl.ks) + 1
    stride = V.INLINE if inline else BLOCK
    frags, crcs = [], []
    for p in range(sl.nparts):
        f = rng.integers(0, 256, (S, room * stride), np.uint8)
        c = rng.integers(0, 256, (S, 4 * room), np.uint8)
        for s in range(S):
            crc = V.crc_bytes(cut[s][p])
            for b in range(cut[s][p].shape[0]):
                if inline:
                    f[s, b * stride:b * stride + 4] = crc[4 * b:4 * b + 4]
                    f[s, b * stride + 4:b * stride + 4 + BLOCK] = cut[s][p][b]
                else:
                    f[s, b * BLOCK:(b + 1) * BLOCK] = cut[s][p][b]
            c[s, :crc.size] = crc
        frags.append(f)
        crcs.append(c)
    return chunks, frags, (None if inline else crcs)


def flip(frags, p, s=0, at=BLOCK + 9):
    frags[p][s, at] ^= 0x40


EC32 = st.ec_slice_type(3, 2)
XOR3 = st.K_XOR2 + 1


def whole(result, chunks, ns):
    for s, n in enumerate(ns):
        assert np.array_equal(result.out[s, :n * BLOCK].reshape(n, BLOCK),
                              chunks[s]), f"chunk {s}"


@pytest.mark.parametrize("sl", SLICES, ids=lambda s: s.name)
def test_clean_through_python(sl):
    """read_chunks_verified_host returns what read_chunks_host returns, under
    every loss pattern, for three chunks of different lengths and ranges."""
    top = 2 * sl.ks + 1
    ns = [top, 1, sl.ks + 1]
    first, count = [0, 0, 1], [top, 1, sl.ks]
    chunks, frags, crcs = py_parts(sl, ns)
    for lost in sl.losses():
        r = chunkread.read_chunks_verified_host(
            slice_type(sl), frags, crcs, ns, first, count, erased=set(lost))
        plain = chunkread.read_chunks_host(
            slice_type(sl), frags, ns, first, count, erased=set(lost))
        assert np.array_equal(r.out, plain), lost
        assert r.corrupt == [()] * 3 and r.unreadable == [False] * 3
        for s in range(3):
            assert np.array_equal(
                r.out[s, :count[s] * BLOCK].reshape(-1, BLOCK),
                C.chunk_blocks(chunks[s], first[s], count[s]))


@pytest.mark.parametrize("inline", [False, True], ids=["array", "inline"])
def test_rounds_ec32(inline):
    sl, ns = C.Slice("ec", 3, 2), [7]
    kw = dict(inline_crcs=True, src_stride=V.INLINE) if inline else {}

    def read(frags, crcs, **more):
        return chunkread.read_chunks_verified_host(
            EC32, frags, crcs, ns, 0, 7, **kw, **more)

    chunks, frags, crcs = py_parts(sl, ns, inline)
    r = read(frags, crcs)
    whole(r, chunks, ns)
    assert r.corrupt == [()] and r.unreadable == [False]
    # one corrupt data part, for each of them
    for p in range(3):
        chunks, frags, crcs = py_parts(sl, ns, inline)
        flip(frags, p)
        r = read(frags, crcs)
        whole(r, chunks, ns)
        assert r.corrupt == [(p,)] and r.unreadable == [False]
        one = read(frags, crcs, retry=False)
        assert one.corrupt == [(p,)] and one.unreadable == [True]
    # two: the second round reads parity 3 too, the third parity 4
    chunks, frags, crcs = py_parts(sl, ns, inline)
    flip(frags, 1)
    flip(frags, 3)
    r = read(frags, crcs)
    whole(r, chunks, ns)
    assert r.corrupt == [(1, 3)] and r.unreadable == [False]
    # three are too many
    flip(frags, 0)
    r = read(frags, crcs)
    assert r.corrupt == [(0, 1, 3)] and r.unreadable == [True]
    # a corrupt part on top of an erased one
    chunks, frags, crcs = py_parts(sl, ns, inline)
    flip(frags, 2)
    r = read(frags, crcs, erased={0})
    whole(r, chunks, ns)
    assert r.corrupt == [(2,)] and r.unreadable == [False]
    # a data part lost and parity 3 corrupt: only the degraded round reads
    # parity 3, the next one uses parity 4
    chunks, frags, crcs = py_parts(sl, ns, inline)
    flip(frags, 3)
    frags[0] = None
    r = read(frags, crcs)
    whole(r, chunks, ns)
    assert r.corrupt == [(3,)] and r.unreadable == [False]
    # ... and a healthy read never looks at it
    chunks, frags, crcs = py_parts(sl, ns, inline)
    flip(frags, 3)
    flip(frags, 4)
    r = read(frags, crcs)
    whole(r, chunks, ns)
    assert r.corrupt == [()]


def test_rounds_other_slices():
    sl, ns = C.Slice("xor", 3), [7]
    chunks, frags, crcs = py_parts(sl, ns)
    flip(frags, 2)
    r = chunkread.read_chunks_verified_host(XOR3, frags, crcs, ns, 0, 7)
    whole(r, chunks, ns)
    assert r.corrupt == [(2,)] and r.unreadable == [False]
    flip(frags, 0)                       # the parity, read by round 1
    r = chunkread.read_chunks_verified_host(XOR3, frags, crcs, ns, 0, 7)
    assert r.corrupt == [(0, 2)] and r.unreadable == [True]
    sl = C.Slice("std")
    chunks, frags, crcs = py_parts(sl, [3])
    r = chunkread.read_chunks_verified_host(st.K_STANDARD, frags, crcs, [3],
                                            0, 3)
    whole(r, chunks, [3])
    flip(frags, 0)
    r = chunkread.read_chunks_verified_host(st.K_STANDARD, frags, crcs, [3],
                                            0, 3)
    assert r.corrupt == [(0,)] and r.unreadable == [True]
    # a part without CRCs is used as it is
    crcs[0] = None
    r = chunkread.read_chunks_verified_host(st.K_STANDARD, frags, crcs, [3],
                                            0, 3)
    assert r.corrupt == [()] and r.unreadable == [False]


def test_rounds_keep_chunks_apart(monkeypatch):
    """Three chunks, one bad: round 1 holds that chunk alone, the other rows
    are written once and stay as round 0 left them."""
    sl, ns = C.Slice("ec", 3, 2), [7, 4, 5]
    chunks, frags, crcs = py_parts(sl, ns)
    flip(frags, 1, s=1, at=7)
    rounds = []
    real = chunkread._verified_call

    def spy(fn, head, b, dst, *rest):
        rounds.append((list(b.chunks), [int(d) for d in dst]))
        return real(fn, head, b, dst, *rest)
    monkeypatch.setattr(chunkread, "_verified_call", spy)
    out = np.full((3, 7 * BLOCK), C.FILL, np.uint8)
    r = chunkread.read_chunks_verified_host(
        EC32, frags, crcs, ns, [0, 1, 2], [7, 3, 3], out=out)
    assert r.out is out
    assert r.corrupt == [(), (1,), ()] and r.unreadable == [False] * 3
    base, pitch = out.ctypes.data, out.strides[0]
    assert rounds == [([0, 1, 2], [base, base + pitch, base + 2 * pitch]),
                      ([1], [base + pitch])]
    for s, (f, c) in enumerate(((0, 7), (1, 3), (2, 3))):
        assert np.array_equal(out[s, :c * BLOCK].reshape(c, BLOCK),
                              C.chunk_blocks(chunks[s], f, c))
        assert (out[s, c * BLOCK:] == C.FILL).all()


# ---- refusals ------------------------------------------------------------------------

def test_refusals_write_nothing():
    sl = C.Slice("ec", 3, 2)
    n = 7
    chunk = np.random.default_rng(5).integers(0, 256, (n, BLOCK), np.uint8)
    parts = sl.cut(chunk)
    store = V.VerifiedStore(sl.nparts, 4, seed=9)
    where = [store.put(p) for p in parts]
    srcs, cmap, tbl = sl.plan((1,))
    reads = V.VReads(sl, 1)
    for f, c in ((0, 7), (4, 2)):
        reads.add([where[p][0] for p in srcs],
                  [sl.count(p, n) for p in srcs], cmap, f, c,
                  C.chunk_blocks(chunk, f, c),
                  crc_offs=[where[p][1] for p in srcs])
    offs, size = reads.out_layout()
    arena = np.full(size, C.FILL, np.uint8)
    bad = np.full(2, POISON, np.uint32)
    before = store.data.copy(), store.crc.copy()
    base = dict(zip(("sp", "nb", "cmap", "first", "count", "dp"),
                    reads.arrays(store.data.ctypes.data, arena.ctypes.data,
                                 offs)))
    base["cp"] = reads.crc_ptrs(store.crc.ctypes.data)

    def call(srcs=3, rows=1, tbl=tbl, ntables=1, ks=3, num_reads=2,
             sstride=BLOCK, dstride=BLOCK, cstride=4, bad=bad, **change):
        a = {k: v.copy() for k, v in base.items()}
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                a[k].reshape(-1)[v[0]] = v[1]
        return verified_call(srcs, rows, tbl, ntables, None, a["sp"],
                             a["nb"], ks, a["cmap"], a["first"], a["count"],
                             a["dp"], num_reads, sstride, dstride, a["cp"],
                             cstride, bad)

    refused = {
        # the call's own
        "crc_dptrs NULL": dict(cp=None),
        "bad_out NULL": dict(bad=None),
        "crc_block_stride 3": dict(cstride=3),
        "crc_block_stride 0": dict(cstride=0),
        # a sample of what the plain read refuses
        "source address 0 with a count": dict(sp=(1, 0)),
        "source address 2 mod 4": dict(sp=(0, int(base["sp"][0, 0]) + 2)),
        "source stride 65538": dict(sstride=65538),
        "destination stride 65532": dict(dstride=65532),
        "tables NULL at rows 1": dict(tbl=None),
        "srcs 33": dict(srcs=33),
        "col_map names slot 3": dict(cmap=(0, 3)),
        "a requested column unmapped": dict(cmap=(0, 0xFF)),
        "block_count 0": dict(count=(1, 0)),
        "past block 1048576": dict(first=(1, 1048575)),
        "destination address 0": dict(dp=(0, 0)),
        "src_nblocks NULL": dict(nb=None),
        "num_reads 0": dict(num_reads=0),
    }
    for what, change in refused.items():
        assert call(**change) == LIZEC_EINVAL, what
        assert (arena == C.FILL).all(), what
        assert (bad == POISON).all(), what
    assert np.array_equal(store.data, before[0])
    assert np.array_equal(store.crc, before[1])
    # the call that all of the above are one change away from
    assert call() == LIZEC_OK
    assert np.array_equal(arena, reads.expected_arena(offs, size))
    assert bad.tolist() == [0, 0]


def test_argument_errors_need_no_library(monkeypatch):
    def no_call(*a, **kw):
        raise AssertionError("the library was used")
    monkeypatch.setattr(L, "lib", no_call)
    monkeypatch.setattr(L, "engine", no_call)
    S, cb = 3, [1, 4, 7]
    frag = np.zeros((S, 3 * BLOCK), np.uint8)
    crc = np.zeros((S, 12), np.uint8)
    f5, c5 = [frag] * 5, [crc] * 5
    wide = [np.zeros((S, 3 * V.INLINE), np.uint8)] * 5

    def refused(*a, **kw):
        with pytest.raises(ValueError):
            chunkread.read_chunks_verified_host(*a, **kw)

    # what read_chunks_host refuses
    refused(st.K_TAPE, [frag], [crc], cb, 0, 1)
    refused(EC32, f5, c5, [0, 4, 7], 0, 1)
    refused(EC32, f5[:4], c5, cb, 0, 1)
    refused(EC32, f5, c5, cb, 0, 0)
    refused(EC32, f5, c5, cb, 0, 1, src_stride=65538)
    refused(EC32, f5, c5, cb, 0, 1, dst_stride=65532)
    refused(EC32, f5, c5, cb, 0, 3, erased={0, 1, 2})       # unreadable
    refused(EC32, [frag[:, 1:]] * 5, c5, [1, 1, 1], 0, 1)   # alignment
    refused(EC32, f5, c5, cb, 0, 3, out=np.zeros((S, BLOCK), np.uint8))
    # the CRCs
    refused(EC32, f5, None, cb, 0, 3)
    refused(EC32, f5, c5[:4], cb, 0, 3)                     # one per part
    refused(EC32, f5, [crc[:2]] * 5, cb, 0, 3)              # rows
    refused(EC32, f5, [crc[:, :8]] * 5, cb, 0, 3)           # 3 blocks: 12
    refused(EC32, f5, [crc.astype(np.int8)] * 5, cb, 0, 3)
    refused(EC32, f5, [crc[:, ::2]] * 5, [1, 1, 1], 0, 1)   # contiguous rows
    refused(EC32, f5, [crc.reshape(-1)] * 5, cb, 0, 3)      # [S, L]
    refused(EC32, f5, [None, None, None, None, list(crc)], cb, 0, 3)
    # inline
    refused(EC32, wide, c5, cb, 0, 3, inline_crcs=True, src_stride=V.INLINE)
    refused(EC32, wide, None, cb, 0, 3, inline_crcs=True)   # stride 65536
    refused(EC32, wide, None, cb, 0, 3, inline_crcs=True, src_stride=65538)
    refused(EC32, [w[:, :3 * V.INLINE - 4] for w in wide], None, cb, 0, 3,
            inline_crcs=True, src_stride=V.INLINE)          # CRC + 3 blocks
    # read_chunks_verified: the same checks, then tensors not on a GPU
    torch = pytest.importorskip("torch")
    t5 = [torch.zeros((S, 3 * BLOCK), dtype=torch.uint8)] * 5
    for a, kw in (((EC32, f5, c5, cb, 0, 3), {}),
                  ((EC32, t5, c5, cb, 0, 3), {}),
                  ((EC32, t5, None, cb, 0, 3), dict(inline_crcs=True))):
        with pytest.raises(ValueError):
            chunkread.read_chunks_verified(*a, **kw)


def test_symbols_are_exported():
    lib = L.lib()
    for name in ("lizec_chunk_read_verified_batch",
                 "lizec_chunk_read_verified_host"):
        assert getattr(lib, name) is not None
