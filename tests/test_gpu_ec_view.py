"""lizec_ec_encode_batch_view through the C ABI: parts of a target slice cut
from a chunk that is held in another slice type (the chunk view), bit-exact
against oracle.ec_encode_data over rows that numpy cuts from the assembled,
zero-padded chunk.

Cell ids are [dests-srcs-ks-layout].  row_cols = srcs, except 3 at srcs = 1,
where the first column is 1, 2, 0, 1, 2, 0 across the stripes (a data
target).  Every cell has six stripes of at most three block rows; rc stands
for row_cols, n for the chunk's block count:

  stripe  n          destination counts   what it is for
  0       2*rc + 1   3                    (a) the last row has one source
                                          present, the loop bound cuts the
                                          rest; at srcs = 1 its one source
                                          would be chunk block n itself
  1       ks*rc + 1  3                    (b) the walk wraps through every view
                                          part, with both remainders; at
                                          ks >= 3 the chunk is longer than every
                                          destination
  2       1          1                    (c) one block; view parts 1.. are
                                          unused and have address 0
  3       3*rc       0, addresses 0       (d) no map entry, no workgroup
  4       rc + 1     one above the rows   (e) that row is stored as zeros
                     that a source reaches
  5       3*rc       2 (even l), 3 (odd)  (f) destinations of one stripe that
                                          differ; at dests = 9 the second pass
                                          has nothing to store in row 2

Every view part is VB = ceil(3*rc / ks) + 1 blocks of random bytes in an
arena of random bytes, so a part holds random bytes beyond its own block
count and the chunk blocks from n on are random too: reading one changes
the result.  Destinations sit in an arena of 0xA5, each part between
256-byte canaries; after a call the whole arena is compared, so blocks
beyond a destination's count, canaries and the CRC slots between blocks must
still be 0xA5.  The sources are compared after every call as well.
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
NB = 3                      # block rows of a cell
S = 6
GUARD = 256
FILL = 0xA5
SPECIALS = (0, 1, 2, 0x80, 0xFF)

DESTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 17)
SRCS = (1, 2, 3, 32)
KS = (1, 2, 3, 5)
# name -> ((source stride, phase), (destination stride, phase))
LAYOUTS = {
    "il-il": ((65540, 4), (65540, 4)),
    "flat-il": ((65536, 0), (65540, 4)),
    "il-flat": ((65540, 4), (65536, 0)),
    "al-strided": ((65552, 0), (65600, 0)),
}
# where the stripes of a misaligned side start, mod 16
PHASES = (4, 8, 12, 4, 8, 12)

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


def row_cols_of(srcs):
    return 3 if srcs == 1 else srcs


def first_cols(srcs):
    """col0 per stripe: a data target's part index at srcs = 1, else 0."""
    if srcs == 1:
        return np.array([(s + 1) % 3 for s in range(S)], np.uint32)
    return np.zeros(S, np.uint32)


def chunk_counts(srcs, ks):
    rc = row_cols_of(srcs)
    return np.array([2 * rc + 1, ks * rc + 1, 1, 3 * rc, rc + 1, 3 * rc],
                    np.uint32)


def rows_reached(n, rc, col0):
    """Block rows in which at least the first source exists."""
    return max(0, -(-(int(n) - int(col0)) // rc))


def dst_counts(dests, srcs, ks):
    rc = row_cols_of(srcs)
    n, col0 = chunk_counts(srcs, ks), first_cols(srcs)
    c = np.empty((S, dests), np.uint32)
    c[0], c[1], c[2], c[3] = 3, 3, 1, 0
    c[4] = rows_reached(n[4], rc, col0[4]) + 1
    c[5] = [2 if l % 2 == 0 else 3 for l in range(dests)]
    return c


def view_blocks(srcs, ks):
    """VB: blocks of every view part of a cell."""
    return -(-NB * row_cols_of(srcs) // ks) + 1


def test_the_cells_hold_what_they_claim(abi):
    """The stripe table above, checked on the host (no GPU work; `abi` only
    ties it to the call whose cells these are)."""
    for srcs in SRCS:
        rc = row_cols_of(srcs)
        for ks in KS:
            n, col0 = chunk_counts(srcs, ks), first_cols(srcs)
            dc = dst_counts(9, srcs, ks)
            assert dc.max() <= NB and (dc[3] == 0).all()
            assert (col0 + srcs <= rc).all()
            # (a) the last row of stripe 0 starts at the chunk's last block
            assert n[0] - 2 * rc == 1 and dc[0].max() == 3
            if srcs == 1:       # there the last row's source is block n
                assert 2 * rc + col0[0] == n[0] >= max(KS)
            # (b) the first NB rows of stripe 1 use every view part
            used = {c % ks for c in range(min(int(n[1]), NB * rc))}
            assert used == set(range(ks))
            # (e) one row more than any source reaches
            assert dc[4, 0] == rows_reached(n[4], rc, col0[4]) + 1 <= NB
            # (f)
            assert set(dc[5].tolist()) == {2, 3}
            # every chunk block that a correct or an off-by-one kernel can
            # touch lies inside its view part
            assert (NB * rc) // ks < view_blocks(srcs, ks)


class Arena:
    """S * nparts parts of nb blocks at `stride`, each between GUARD bytes;
    stripe s of a misaligned side starts PHASES[s] bytes past a 16-byte
    boundary."""

    def __init__(self, nparts, nb, stride, phase, fill=None, seed=0):
        self.nparts, self.nb, self.stride = nparts, nb, stride
        self.span = (nb - 1) * stride + BLOCK
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

    def block(self, s, p, b):
        at = self.offs[s * self.nparts + p] + b * self.stride
        return self.host[at:at + BLOCK]

    def place(self, data, counts):
        """data [S, nparts, nb*BLOCK] -> the blocks of self.host, of part
        (s, p) only those below counts[s, p]."""
        for s in range(S):
            for p in range(self.nparts):
                for b in range(int(counts[s, p])):
                    self.block(s, p, b)[:] = \
                        data[s, p, b * BLOCK:(b + 1) * BLOCK]

    def upload(self):
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptrs = (np.uint64(self.dev.data_ptr()) +
                     self.offs.astype(np.uint64)).reshape(S, self.nparts)
        return self


def target_sources(view, srcs, ks, n, col0):
    """What the reference would hand to the encoder, from the view arena's
    host bytes alone: [S, srcs, NB*BLOCK].  The chunk is assembled from the
    view parts, zero-padded to NB whole rows and cut into rows of rc."""
    rc = row_cols_of(srcs)
    out = np.zeros((S, srcs, NB * BLOCK), np.uint8)
    for s in range(S):
        chunk = np.zeros((NB * rc, BLOCK), np.uint8)
        for c in range(min(int(n[s]), NB * rc)):
            chunk[c] = view.block(s, c % ks, c // ks)
        rows = chunk.reshape(NB, rc, BLOCK)
        for j in range(srcs):
            out[s, j] = rows[:, int(col0[s]) + j].reshape(-1)
    return out


def oracle_encode(tbl, sources, dests):
    """exp [S, dests, NB*BLOCK] of one table over the cut sources."""
    srcs = sources.shape[1]
    exp = np.empty((S, dests, NB * BLOCK), np.uint8)
    for s in range(S):
        outs = [np.full(NB * BLOCK, 0x77, np.uint8) for _ in range(dests)]
        oracle.ec_encode_data(
            tbl, [np.ascontiguousarray(sources[s, j]) for j in range(srcs)],
            outs)
        exp[s] = np.stack(outs)
    return exp


_views = {}


def view_arena(srcs, ks, ss, sph):
    """The uploaded view arena of (srcs, ks, source layout) and the sources
    numpy cuts from it; the last one is kept, as the layouts of one cell run
    in a row and two of them share a source layout."""
    key = (srcs, ks, ss, sph)
    if key not in _views:
        _views.clear()
        view = Arena(ks, view_blocks(srcs, ks), ss, sph,
                     seed=1000 * srcs + 10 * ks + sph)
        cut = target_sources(view, srcs, ks, chunk_counts(srcs, ks),
                             first_cols(srcs))
        _views[key] = (view.upload(), cut)
    return _views[key]


_expected = {}


def expected(dests, srcs, ks, ss, sph):
    """[(tables, exp [S, dests, NB*BLOCK])] for one cell, from the oracle."""
    key = (dests, srcs, ks, ss, sph)
    if key not in _expected:
        _expected.clear()
        _, cut = view_arena(srcs, ks, ss, sph)
        out = []
        for coef in coef_matrices(dests, srcs, 100 * dests + srcs):
            tbl = oracle.init_tables(coef)
            out.append((tbl, oracle_encode(tbl, cut, dests)))
        _expected[key] = out
    return _expected[key]


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    lib = L.lib()
    lib.lizec_ec_encode_batch_view   # a missing symbol fails here
    return lib, L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def call_view(abi, tbls, srcs, dests, view_ptrs, ks, chunk_nb, rc, col0,
              dst_ptrs, dst_nb, sstride, dstride, index=None):
    """tbls: one table or a list of them; index / col0 None = NULL."""
    lib, eng = abi
    if isinstance(tbls, (list, tuple)):
        ntables, tbl = len(tbls), np.concatenate(tbls)
    else:
        ntables, tbl = 1, tbls
    assert tbl.size == ntables * 32 * srcs * dests
    vp = np.ascontiguousarray(view_ptrs, np.uint64)
    cb = np.ascontiguousarray(chunk_nb, np.uint32)
    dp = np.ascontiguousarray(dst_ptrs, np.uint64)
    dn = np.ascontiguousarray(dst_nb, np.uint32)
    assert vp.size == S * ks and cb.size == S
    assert dp.size == dn.size == S * dests
    ix = c0 = None
    if index is not None:
        ix = np.ascontiguousarray(index, np.uint32)
        assert ix.size == S
        ix = ix.ctypes.data_as(u32p)
    if col0 is not None:
        c0 = np.ascontiguousarray(col0, np.uint32)
        assert c0.size == S
        c0 = c0.ctypes.data_as(u32p)
    return lib.lizec_ec_encode_batch_view(
        eng, srcs, dests, tbl.ctypes.data_as(u8p), ntables, ix,
        vp.ctypes.data_as(u64p), ks, cb.ctypes.data_as(u32p), rc, c0,
        dp.ctypes.data_as(u64p), dn.ctypes.data_as(u32p), S, sstride,
        dstride, stream_arg())


def check_arena(dst, exp, counts, what):
    """The whole destination arena: the counted blocks equal exp, all else
    FILL."""
    torch.cuda.synchronize()
    got = dst.dev.cpu().numpy()
    want = Arena(dst.nparts, NB, dst.stride, 0, fill=FILL)
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


def used_view_ptrs(view, n, ks):
    """Addresses of a cell's view: 0 for the parts that hold no block."""
    used = np.arange(ks)[None, :] < np.asarray(n)[:, None]
    return np.where(used, view.ptrs, np.uint64(0))


def dst_ptrs_of(dst, dc):
    return np.where(dc > 0, dst.ptrs, np.uint64(0))


def run_cell(abi, dests, srcs, ks, layout):
    (ss, sph), (ds, dph) = LAYOUTS[layout]
    rc = row_cols_of(srcs)
    n, dc = chunk_counts(srcs, ks), dst_counts(dests, srcs, ks)
    col0 = first_cols(srcs) if srcs == 1 else None   # NULL = all 0
    view, _ = view_arena(srcs, ks, ss, sph)
    vp = used_view_ptrs(view, n, ks)
    for tbl, exp in expected(dests, srcs, ks, ss, sph):
        dst = Arena(dests, NB, ds, dph, fill=FILL).upload()
        dp = dst_ptrs_of(dst, dc)
        # the flags the host derives: aligned iff the stride and every
        # address in use are
        assert (all(p % 16 == 0 for p in vp.reshape(-1)) and
                ss % 16 == 0) == (sph == 0)
        assert (all(p % 16 == 0 for p in dp.reshape(-1)) and
                ds % 16 == 0) == (dph == 0)
        assert call_view(abi, tbl, srcs, dests, vp, ks, n, rc, col0, dp, dc,
                         ss, ds) == LIZEC_OK
        check_arena(dst, exp, dc,
                    f"{layout} dests={dests} srcs={srcs} ks={ks}")
        assert np.array_equal(view.dev.cpu().numpy(), view.host), \
            "the sources were modified"


@pytest.mark.parametrize("layout", tuple(LAYOUTS))
@pytest.mark.parametrize("ks", KS)
@pytest.mark.parametrize("srcs", SRCS)
@pytest.mark.parametrize("dests", DESTS)
def test_view_cell(abi, dests, srcs, ks, layout):
    run_cell(abi, dests, srcs, ks, layout)


def two_tables(dests, srcs):
    coefs = [coef_matrices(dests, srcs, 11)[0],
             np.random.default_rng(12).integers(1, 256, (dests, srcs),
                                                np.uint8)]
    return [oracle.init_tables(c) for c in coefs]


@pytest.mark.parametrize("dests", (2, 9))
def test_table_per_stripe(abi, dests):
    """Two tables, tbl_index alternating: every stripe is encoded with its
    own table, in the passes with dest_base > 0 too (dests = 9)."""
    srcs, ks = 3, 2
    (ss, sph), (ds, dph) = LAYOUTS["il-il"]
    n, dc = chunk_counts(srcs, ks), dst_counts(dests, srcs, ks)
    view, cut = view_arena(srcs, ks, ss, sph)
    tbls = two_tables(dests, srcs)
    per_table = [oracle_encode(t, cut, dests) for t in tbls]
    index = np.array([0, 1, 0, 1, 0, 1], np.uint32)
    exp = np.stack([per_table[index[s]][s] for s in range(S)])
    dst = Arena(dests, NB, ds, dph, fill=FILL).upload()
    assert call_view(abi, tbls, srcs, dests, used_view_ptrs(view, n, ks), ks,
                     n, srcs, None, dst_ptrs_of(dst, dc), dc, ss, ds,
                     index=index) == LIZEC_OK
    check_arena(dst, exp, dc, f"alternating tables, dests={dests}")
    assert np.array_equal(view.dev.cpu().numpy(), view.host)


def test_null_index_is_table_zero(abi):
    dests, srcs, ks = 2, 3, 2
    (ss, sph), (ds, dph) = LAYOUTS["il-il"]
    n, dc = chunk_counts(srcs, ks), dst_counts(dests, srcs, ks)
    view, cut = view_arena(srcs, ks, ss, sph)
    tbls = two_tables(dests, srcs)
    exp = oracle_encode(tbls[0], cut, dests)
    vp = used_view_ptrs(view, n, ks)
    a = Arena(dests, NB, ds, dph, fill=FILL).upload()
    b = Arena(dests, NB, ds, dph, fill=FILL).upload()
    assert call_view(abi, tbls, srcs, dests, vp, ks, n, srcs, None,
                     dst_ptrs_of(a, dc), dc, ss, ds, index=None) == LIZEC_OK
    assert call_view(abi, tbls, srcs, dests, vp, ks, n, srcs, None,
                     dst_ptrs_of(b, dc), dc, ss, ds,
                     index=np.zeros(S, np.uint32)) == LIZEC_OK
    check_arena(a, exp, dc, "tbl_index = NULL")
    check_arena(b, exp, dc, "tbl_index all zero")
    assert torch.equal(a.dev, b.dev)


@pytest.mark.parametrize("srcs", (1, 3))
def test_one_view_part_equals_ragged_call(abi, srcs):
    """ks = 1 is a fixed stride: the same bytes addressed as
    base + (col0 + j) * 65536 with block stride row_cols * 65536 give
    lizec_ec_encode_batch_ragged the same work.  Byte-identical arenas,
    and both equal the oracle."""
    lib, eng = abi
    dests, ks = 5, 1
    rc = row_cols_of(srcs)
    (ss, sph), (ds, dph) = LAYOUTS["flat-il"]
    assert ss == BLOCK
    n, dc = chunk_counts(srcs, ks), dst_counts(dests, srcs, ks)
    col0 = first_cols(srcs)
    view, cut = view_arena(srcs, ks, ss, sph)
    tbl = oracle.init_tables(coef_matrices(dests, srcs, 500 + srcs)[0])
    exp = oracle_encode(tbl, cut, dests)
    a = Arena(dests, NB, ds, dph, fill=FILL).upload()
    b = Arena(dests, NB, ds, dph, fill=FILL).upload()
    assert call_view(abi, tbl, srcs, dests, view.ptrs, ks, n, rc, col0,
                     dst_ptrs_of(a, dc), dc, ss, ds) == LIZEC_OK
    cols = col0[:, None].astype(np.int64) + np.arange(srcs)[None, :]
    sp = view.ptrs[:, :1] + (cols * BLOCK).astype(np.uint64)
    # source j has the rows r with r*rc + col0 + j < n
    sn = np.maximum(0, -(-(n[:, None].astype(np.int64) - cols) // rc))
    sp = np.ascontiguousarray(sp, np.uint64)
    sn = np.ascontiguousarray(sn, np.uint32)
    dp = np.ascontiguousarray(dst_ptrs_of(b, dc), np.uint64)
    assert lib.lizec_ec_encode_batch_ragged(
        eng, srcs, dests, tbl.ctypes.data_as(u8p), 1, None,
        sp.ctypes.data_as(u64p), sn.ctypes.data_as(u32p),
        dp.ctypes.data_as(u64p), dc.ctypes.data_as(u32p), S, rc * BLOCK, ds,
        stream_arg()) == LIZEC_OK
    check_arena(a, exp, dc, "view call")
    check_arena(b, exp, dc, "ragged call")
    assert torch.equal(a.dev, b.dev)
    assert np.array_equal(view.dev.cpu().numpy(), view.host)


REFUSALS = ("view_parts 0", "view_parts 33", "row_cols 0", "row_cols 33",
            "col0 + srcs > row_cols", "srcs > row_cols with col0 NULL",
            "chunk_blocks 0", "chunk_blocks 1048577", "view address 0",
            "view address 2 mod 4", "src stride 65538", "src stride 65532",
            "dst address 2 mod 4", "dst stride 65538", "dst stride 65532",
            "dst count 32769", "dst count with address 0", "dests 33",
            "srcs 0", "index >= ntables", "ntables 0", "all counts zero")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(abi, what):
    """Each returns LIZEC_EINVAL from the host and leaves the arena as it
    was.  The buffers are those of a valid il-il call, so the same call
    with the offending argument put right succeeds."""
    dests, srcs, ks = 2, 3, 2
    (ss, sph), (ds, dph) = LAYOUTS["il-il"]
    n, dc = chunk_counts(srcs, ks), dst_counts(dests, srcs, ks)
    view, _ = view_arena(srcs, ks, ss, sph)
    dst = Arena(dests, NB, ds, dph, fill=FILL).upload()
    tbl, exp = expected(dests, srcs, ks, ss, sph)[0]
    good = dict(tbls=tbl, srcs=srcs, dests=dests,
                view_ptrs=used_view_ptrs(view, n, ks), ks=ks, chunk_nb=n,
                rc=srcs, col0=np.zeros(S, np.uint32),
                dst_ptrs=dst_ptrs_of(dst, dc), dst_nb=dc, sstride=ss,
                dstride=ds, index=np.zeros(S, np.uint32))
    bad = dict(good)
    if what.startswith(("view_parts", "row_cols")):
        bad["ks" if what.startswith("view") else "rc"] = int(what.split()[-1])
    elif what == "col0 + srcs > row_cols":
        bad["col0"] = np.array([0, 0, 0, 0, 0, 1], np.uint32)
    elif what == "srcs > row_cols with col0 NULL":
        bad["rc"], bad["col0"] = srcs - 1, None
    elif what.startswith("chunk_blocks"):
        c = n.copy()
        c[4] = int(what.split()[-1])
        bad["chunk_nb"] = c
    elif what.startswith("view address"):
        p = bad["view_ptrs"].copy()
        assert n[0] > 1                     # part 1 of stripe 0 is in use
        p[0, 1] = 0 if what.endswith(" 0") else p[0, 1] - 2
        bad["view_ptrs"] = p
    elif "stride" in what:
        bad[what[0] + "stride"] = int(what.split()[-1])
    elif what == "dst address 2 mod 4":
        p = bad["dst_ptrs"].copy()
        p[0, 0] -= 2
        bad["dst_ptrs"] = p
    elif what == "dst count 32769":
        c = dc.copy()
        c[0, 0] = 32769
        bad["dst_nb"] = c
    elif what == "dst count with address 0":
        p = bad["dst_ptrs"].copy()
        assert dc[0, 1] > 0
        p[0, 1] = 0
        bad["dst_ptrs"] = p
    elif what == "dests 33":
        bad["dests"] = 33
    elif what == "srcs 0":
        bad["srcs"] = 0
    elif what == "index >= ntables":
        bad["index"] = np.array([0, 0, 0, 0, 0, 1], np.uint32)
    elif what == "ntables 0":
        bad["ntables"] = 0
    else:
        assert what == "all counts zero"
        bad["dst_nb"] = np.zeros_like(dc)

    def call(kw):
        lib, eng = abi
        arrs = [np.ascontiguousarray(kw[k], t) for k, t in
                (("view_ptrs", np.uint64), ("chunk_nb", np.uint32),
                 ("dst_ptrs", np.uint64), ("dst_nb", np.uint32),
                 ("index", np.uint32))]
        c0 = None
        if kw["col0"] is not None:
            c0 = np.ascontiguousarray(kw["col0"], np.uint32)
            arrs.append(c0)
            c0 = c0.ctypes.data_as(u32p)
        vp, cb, dp, dn, ix = arrs[:5]
        return lib.lizec_ec_encode_batch_view(
            eng, kw["srcs"], kw["dests"], kw["tbls"].ctypes.data_as(u8p),
            kw.get("ntables", 1), ix.ctypes.data_as(u32p),
            vp.ctypes.data_as(u64p), kw["ks"], cb.ctypes.data_as(u32p),
            kw["rc"], c0, dp.ctypes.data_as(u64p), dn.ctypes.data_as(u32p),
            S, kw["sstride"], kw["dstride"], stream_arg())

    assert call(bad) == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert bool((dst.dev == FILL).all()), "a refused call wrote the arena"
    assert call(good) == LIZEC_OK
    check_arena(dst, exp, dc, "the valid call")
    assert np.array_equal(view.dev.cpu().numpy(), view.host)
