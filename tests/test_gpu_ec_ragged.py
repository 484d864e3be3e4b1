"""lizec_ec_encode_batch_ragged through the C ABI: parts of different lengths
in one batch (a block count per source and per destination of every stripe,
a coefficient table per stripe), bit-exact against oracle.ec_encode_data on
zero-padded sources.

Every cell has five stripes of at most three blocks per part:

  stripe  destination counts        source counts
  0       3                         source 0 has 2 (shorter than source 1),
                                    the last source 1, the others 3
  1       1                         source 0 has 3 (longer than every
                                    destination), the last source 0 blocks
                                    and address 0, the others 1
  2       0 (addresses 0)           3: the stripe is legal and costs nothing
  3       2                         1 everywhere: block 1 has every source
                                    absent and must come out as zeros
  4       2 (even l), 3 (odd l)     sources 0 and 1, one unrolled pair, have
                                    1; with 32 sources (4, 5) have (2, 0) and
                                    (7, 8), across two pairs, have 0

With one or two sources some of these coincide (stripe 0 of a one-source
cell is a block that nothing covers).  dests = 9 and 17 run passes with
dest_base > 0; at dests = 9 the second pass holds destination 8 alone, whose
2 blocks in stripe 4 leave the workgroups of block 2 with nothing to store.

Sources sit in an arena of random bytes: the blocks beyond a source's count
hold random bytes too, so reading one changes the result.  Destinations sit
in an arena of 0xA5, each part between 256-byte canaries; after a call the
whole arena is compared, so blocks beyond a destination's count, canaries
and the CRC slots between blocks must still be 0xA5.  The sources are
compared after every call as well.
"""
import ctypes

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
BLOCK = 65536
NB = 3
S = 5
GUARD = 256
FILL = 0xA5
SPECIALS = (0, 1, 2, 0x80, 0xFF)

DESTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 17)
SRCS = (1, 2, 3, 32)
# name -> ((source stride, phase), (destination stride, phase))
LAYOUTS = {
    "il-il": ((65540, 4), (65540, 4)),
    "flat-il": ((65536, 0), (65540, 4)),
    "il-flat": ((65540, 4), (65536, 0)),
    "al-strided": ((65552, 0), (65600, 0)),
}
# where the stripes of a misaligned side start, mod 16
PHASES = (4, 8, 12, 4, 8)

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def coef_matrices(dests, srcs, seed):
    """Random coefficient matrices for one cell, row 1 all zero (when there
    is a row 1) and SPECIALS at fixed positions outside it.  A matrix too
    small to hold all five is replaced by several that together do; a
    one-row cell gets a further all-zero matrix for its zero row."""
    rng = np.random.default_rng(seed)
    zero_row = 1 if dests >= 2 else None
    free = [(l, j) for l in range(dests) if l != zero_row
            for j in range(srcs)]
    per = min(len(free), len(SPECIALS))
    mats = []
    for first in range(0, len(SPECIALS), per):
        c = rng.integers(0, 256, (dests, srcs), np.uint8)
        if zero_row is not None:
            c[zero_row] = 0
        for i, v in enumerate(SPECIALS[first:first + per]):
            c[free[(i * len(free)) // per]] = v
        mats.append(c)
    if zero_row is None:
        mats.append(np.zeros((dests, srcs), np.uint8))
    return mats


def dst_counts(dests):
    c = np.empty((S, dests), np.uint32)
    c[0], c[1], c[2], c[3] = 3, 1, 0, 2
    c[4] = [2 if l % 2 == 0 else 3 for l in range(dests)]
    return c


def src_counts(srcs):
    c = np.empty((S, srcs), np.uint32)
    c[0] = 3
    c[0, -1] = 1
    c[0, 0] = 2
    if srcs == 2:
        c[0] = (2, 3)       # "the last source shorter" is stripe 1's then
    c[1] = 1
    c[1, -1] = 0
    c[1, 0] = 3
    c[2] = 3
    c[3] = 1
    c[4] = 3
    c[4, :2] = 1
    if srcs == 32:
        c[4, 4:6] = (2, 0)
        c[4, 7:9] = 0
    return c


def test_the_cells_hold_what_they_claim():
    """The count tables above, checked on the host (needs no GPU work)."""
    for srcs in SRCS:
        sc = src_counts(srcs)
        assert sc.max() <= NB
        for dests in (1, 2, 9):
            dc = dst_counts(dests)
            rows = dc.max(axis=1)
            assert rows.tolist() == [3, 1, 0, 2, 3 if dests > 1 else 2]
            # a block row that no source covers
            assert any((sc[s] <= b).all() for s in range(S)
                       for b in range(rows[s]))
            # a source longer than every destination of its stripe
            assert (sc[1].max() > dc[1].max())
        if srcs >= 2:
            assert sc[0, 0] < sc[0, 1]
            assert sc[1, -1] == 0 < sc[1, -2]
        if srcs >= 3:
            assert sc[0, 0] < sc[0, 1] and sc[0, -1] < sc[0, -2]
            # an unrolled pair absent in a block that other sources cover
            assert (sc[4, :2] <= 1).all() and sc[4, 2] > 1


_pool = None


def source_pool():
    """Random [S, 32, NB * BLOCK] bytes shared (read-only) by all cells."""
    global _pool
    if _pool is None:
        _pool = np.random.default_rng(3276).integers(
            0, 256, (S, 32, NB * BLOCK), np.uint8)
        _pool.setflags(write=False)
    return _pool


def padded_sources(srcs, counts=None):
    """The pool's first `srcs` parts with everything from each source's
    count on replaced by zeros: what the reference would read."""
    counts = src_counts(srcs) if counts is None else counts
    p = np.array(source_pool()[:, :srcs])
    for s in range(S):
        for j in range(srcs):
            p[s, j, int(counts[s, j]) * BLOCK:] = 0
    return p


def oracle_encode(tbl, padded, dests):
    """exp [S, dests, NB*BLOCK] of one table over zero-padded sources."""
    srcs = padded.shape[1]
    exp = np.empty((S, dests, NB * BLOCK), np.uint8)
    for s in range(S):
        outs = [np.full(NB * BLOCK, 0x77, np.uint8) for _ in range(dests)]
        oracle.ec_encode_data(
            tbl, [np.ascontiguousarray(padded[s, j]) for j in range(srcs)],
            outs)
        exp[s] = np.stack(outs)
    return exp


_expected = {}


def expected(dests, srcs):
    """[(coef, tables, exp [S, dests, NB*BLOCK])] for one cell, from the
    oracle; the last cell is kept, the layouts of one cell run in a row."""
    key = (dests, srcs)
    if key not in _expected:
        _expected.clear()
        padded = padded_sources(srcs)
        out = []
        for coef in coef_matrices(dests, srcs, 100 * dests + srcs):
            tbl = oracle.init_tables(coef)
            out.append((coef, tbl, oracle_encode(tbl, padded, dests)))
        _expected[key] = out
    return _expected[key]


class Arena:
    """S * nparts parts of NB blocks at `stride`, each between GUARD bytes;
    stripe s of a misaligned side starts PHASES[s] bytes past a 16-byte
    boundary."""

    def __init__(self, nparts, stride, phase, fill=None, seed=0):
        self.nparts, self.stride = nparts, stride
        self.span = (NB - 1) * stride + BLOCK
        self.slot = (GUARD + 16 + self.span + GUARD + 15) // 16 * 16
        n = S * nparts * self.slot
        if fill is None:
            self.host = np.random.default_rng(seed).integers(0, 256, n,
                                                             np.uint8)
        else:
            self.host = np.full(n, fill, np.uint8)
        self.offs = np.array(
            [(s * nparts + p) * self.slot + GUARD + (PHASES[s] if phase else 0)
             for s in range(S) for p in range(nparts)], np.int64)

    def place(self, data, counts=None):
        """data [S, nparts, NB*BLOCK] -> the blocks of self.host, of part
        (s, p) only those below counts[s, p]."""
        flat = data.reshape(S * self.nparts, NB, BLOCK)
        for i, off in enumerate(self.offs):
            n = NB if counts is None else int(counts.reshape(-1)[i])
            for b in range(n):
                at = off + b * self.stride
                self.host[at:at + BLOCK] = flat[i, b]

    def upload(self):
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = (np.uint64(self.dev.data_ptr()) +
                     self.offs.astype(np.uint64))
        return self


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    lib = L.lib()
    lib.lizec_ec_encode_batch_ragged   # a missing symbol fails here
    return lib, L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def call_ragged(abi, tbls, srcs, dests, src_ptrs, src_nb, dst_ptrs, dst_nb,
                sstride, dstride, index=None):
    """tbls: one table or a list of them; index None = NULL."""
    lib, eng = abi
    if isinstance(tbls, (list, tuple)):
        ntables, tbl = len(tbls), np.concatenate(tbls)
    else:
        ntables, tbl = 1, tbls
    assert tbl.size == ntables * 32 * srcs * dests
    sp = np.ascontiguousarray(src_ptrs, np.uint64)
    dp = np.ascontiguousarray(dst_ptrs, np.uint64)
    sn = np.ascontiguousarray(src_nb, np.uint32)
    dn = np.ascontiguousarray(dst_nb, np.uint32)
    assert sp.size == sn.size == S * srcs and dp.size == dn.size == S * dests
    ix = None
    if index is not None:
        ix = np.ascontiguousarray(index, np.uint32)
        assert ix.size == S
        ix = ix.ctypes.data_as(u32p)
    return lib.lizec_ec_encode_batch_ragged(
        eng, srcs, dests, tbl.ctypes.data_as(u8p), ntables, ix,
        sp.ctypes.data_as(u64p), sn.ctypes.data_as(u32p),
        dp.ctypes.data_as(u64p), dn.ctypes.data_as(u32p), S, sstride,
        dstride, stream_arg())


def check_arena(dst, exp, counts, what):
    """The whole destination arena: the counted blocks equal exp, all else
    FILL."""
    torch.cuda.synchronize()
    got = dst.dev.cpu().numpy()
    want = Arena(dst.nparts, dst.stride, 0, fill=FILL)
    want.offs = dst.offs
    want.place(exp, counts)
    if not np.array_equal(got, want.host):
        bad = np.flatnonzero(got != want.host)
        inside = np.zeros(got.size, bool)
        for i, off in enumerate(dst.offs):
            for b in range(int(counts.reshape(-1)[i])):
                inside[off + b * dst.stride:off + b * dst.stride + BLOCK] = True
        pytest.fail(f"{what}: {bad.size} bytes differ, "
                    f"{int((~inside[bad]).sum())} of them outside every "
                    f"counted destination block; first offsets "
                    f"{bad[:6].tolist()}")


def cell_ptrs(src, dst, sc, dc):
    """Addresses of a cell: 0 wherever the count is 0."""
    return (np.where(sc.reshape(-1) > 0, src.ptrs, np.uint64(0)),
            np.where(dc.reshape(-1) > 0, dst.ptrs, np.uint64(0)))


def source_arena(srcs, ss, sph, seed):
    src = Arena(srcs, ss, sph, seed=seed)
    src.place(np.ascontiguousarray(source_pool()[:, :srcs]))
    return src.upload()


def run_cell(abi, dests, srcs, layout):
    (ss, sph), (ds, dph) = LAYOUTS[layout]
    sc, dc = src_counts(srcs), dst_counts(dests)
    src = source_arena(srcs, ss, sph, srcs)
    for coef, tbl, exp in expected(dests, srcs):
        dst = Arena(dests, ds, dph, fill=FILL).upload()
        sp, dp = cell_ptrs(src, dst, sc, dc)
        # the flags the host derives: aligned iff the stride and every
        # address in use are
        assert (all(p % 16 == 0 for p in sp) and ss % 16 == 0) == (sph == 0)
        assert (all(p % 16 == 0 for p in dp) and ds % 16 == 0) == (dph == 0)
        assert call_ragged(abi, tbl, srcs, dests, sp, sc, dp, dc, ss,
                           ds) == LIZEC_OK
        check_arena(dst, exp, dc, f"{layout} dests={dests} srcs={srcs}")
        assert np.array_equal(src.dev.cpu().numpy(), src.host), \
            "the sources were modified"


@pytest.mark.parametrize("layout", tuple(LAYOUTS))
@pytest.mark.parametrize("srcs", SRCS)
@pytest.mark.parametrize("dests", DESTS)
def test_ragged_cell(abi, dests, srcs, layout):
    run_cell(abi, dests, srcs, layout)


@pytest.mark.parametrize("dests", (2, 9))
def test_table_per_stripe(abi, dests):
    """Two tables, tbl_index alternating: every stripe is encoded with its
    own table, in the passes with dest_base > 0 too (dests = 9)."""
    srcs = 3
    (ss, sph), (ds, dph) = LAYOUTS["il-il"]
    sc, dc = src_counts(srcs), dst_counts(dests)
    src = source_arena(srcs, ss, sph, 7)
    coefs = [coef_matrices(dests, srcs, 11)[0],
             np.random.default_rng(12).integers(1, 256, (dests, srcs),
                                                np.uint8)]
    tbls = [oracle.init_tables(c) for c in coefs]
    padded = padded_sources(srcs)
    per_table = [oracle_encode(t, padded, dests) for t in tbls]
    index = np.array([0, 1, 0, 1, 0], np.uint32)
    exp = np.stack([per_table[index[s]][s] for s in range(S)])
    dst = Arena(dests, ds, dph, fill=FILL).upload()
    sp, dp = cell_ptrs(src, dst, sc, dc)
    assert call_ragged(abi, tbls, srcs, dests, sp, sc, dp, dc, ss, ds,
                       index=index) == LIZEC_OK
    check_arena(dst, exp, dc, f"alternating tables, dests={dests}")
    assert np.array_equal(src.dev.cpu().numpy(), src.host)


def test_null_index_is_table_zero(abi):
    dests, srcs = 2, 3
    (ss, sph), (ds, dph) = LAYOUTS["il-il"]
    sc, dc = src_counts(srcs), dst_counts(dests)
    src = source_arena(srcs, ss, sph, 8)
    coefs = [coef_matrices(dests, srcs, 11)[0],
             np.random.default_rng(12).integers(1, 256, (dests, srcs),
                                                np.uint8)]
    tbls = [oracle.init_tables(c) for c in coefs]
    exp = oracle_encode(tbls[0], padded_sources(srcs), dests)
    a = Arena(dests, ds, dph, fill=FILL).upload()
    b = Arena(dests, ds, dph, fill=FILL).upload()
    sp, dpa = cell_ptrs(src, a, sc, dc)
    _, dpb = cell_ptrs(src, b, sc, dc)
    assert call_ragged(abi, tbls, srcs, dests, sp, sc, dpa, dc, ss, ds,
                       index=None) == LIZEC_OK
    assert call_ragged(abi, tbls, srcs, dests, sp, sc, dpb, dc, ss, ds,
                       index=np.zeros(S, np.uint32)) == LIZEC_OK
    check_arena(a, exp, dc, "tbl_index = NULL")
    check_arena(b, exp, dc, "tbl_index all zero")
    assert torch.equal(a.dev, b.dev)


@pytest.mark.parametrize("layout", ("il-il", "al-strided"))
def test_equal_counts_equal_strided_call(abi, layout):
    """All counts equal: byte-identical to lizec_ec_encode_batch_strided,
    and both equal the oracle."""
    lib, eng = abi
    dests, srcs = 5, 3
    (ss, sph), (ds, dph) = LAYOUTS[layout]
    src = source_arena(srcs, ss, sph, 9)
    sc = np.full((S, srcs), NB, np.uint32)
    dc = np.full((S, dests), NB, np.uint32)
    coef = coef_matrices(dests, srcs, 500 + srcs)[0]
    tbl = oracle.init_tables(coef)
    exp = oracle_encode(tbl, padded_sources(srcs, sc), dests)
    a = Arena(dests, ds, dph, fill=FILL).upload()
    b = Arena(dests, ds, dph, fill=FILL).upload()
    assert call_ragged(abi, tbl, srcs, dests, src.ptrs, sc, a.ptrs, dc, ss,
                       ds) == LIZEC_OK
    assert lib.lizec_ec_encode_batch_strided(
        eng, NB, srcs, dests, tbl.ctypes.data_as(u8p),
        src.ptrs.ctypes.data_as(u64p), b.ptrs.ctypes.data_as(u64p), S, ss, ds,
        stream_arg()) == LIZEC_OK
    check_arena(a, exp, dc, "ragged call")
    check_arena(b, exp, dc, "strided call")
    assert torch.equal(a.dev, b.dev)


REFUSALS = ("src address 2 mod 4", "dst address 2 mod 4", "src stride 65538",
            "dst stride 65538", "src stride 65532", "dst stride 65532",
            "src count 32769", "dst count 32769", "src count with address 0",
            "dst count with address 0", "index >= ntables", "all counts zero")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(abi, what):
    """Each returns LIZEC_EINVAL from the host and leaves the arena as it
    was.  The buffers are those of a valid il-il call, so the same call
    with the offending argument put right succeeds."""
    dests, srcs = 2, 3
    (ss, sph), (ds, dph) = LAYOUTS["il-il"]
    sc, dc = src_counts(srcs), dst_counts(dests)
    src = source_arena(srcs, ss, sph, 2)
    dst = Arena(dests, ds, dph, fill=FILL).upload()
    coef, tbl, exp = expected(dests, srcs)[0]
    sp, dp = cell_ptrs(src, dst, sc, dc)
    good = dict(src_ptrs=sp, src_nb=sc, dst_ptrs=dp, dst_nb=dc, sstride=ss,
                dstride=ds, index=np.zeros(S, np.uint32))
    bad = dict(good)
    side = "src" if what.startswith("src") else "dst"
    if what.endswith("address 2 mod 4"):
        p = bad[side + "_ptrs"].copy()
        assert bad[side + "_nb"].reshape(-1)[0] > 0   # an address in use
        p[0] -= 2
        bad[side + "_ptrs"] = p
    elif what.endswith("with address 0"):
        p = bad[side + "_ptrs"].copy()
        assert bad[side + "_nb"].reshape(-1)[1] > 0
        p[1] = 0
        bad[side + "_ptrs"] = p
    elif "stride" in what:
        bad[side[0] + "stride"] = int(what.split()[-1])
    elif "count 32769" in what:
        c = bad[side + "_nb"].copy()
        c[0, 0] = 32769
        bad[side + "_nb"] = c
    elif what == "index >= ntables":
        bad["index"] = np.array([0, 0, 0, 0, 1], np.uint32)
    else:
        bad["dst_nb"] = np.zeros_like(dc)

    def call(kw):
        return call_ragged(abi, tbl, srcs, dests, kw["src_ptrs"],
                           kw["src_nb"], kw["dst_ptrs"], kw["dst_nb"],
                           kw["sstride"], kw["dstride"], index=kw["index"])

    assert call(bad) == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert bool((dst.dev == FILL).all()), "a refused call wrote the arena"
    assert call(good) == LIZEC_OK
    check_arena(dst, exp, dc, "the valid call")
    assert np.array_equal(src.dev.cpu().numpy(), src.host)
