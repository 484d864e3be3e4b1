"""lizec_ec_encode_batch_strided through the C ABI: parts stored as 64 KiB
blocks at a stride, at addresses that are only 4-byte aligned (the
INTERLEAVED chunk format), bit-exact against oracle.ec_encode_data.

Every cell has nblocks = 5 and two stripes.  With a block stride of 65540
and a first block at 4 mod 16, the blocks of stripe 0 start at 4, 8, 12, 0, 4
mod 16; stripe 1 of a misaligned side is based at 8 mod 16.  A side given as
aligned keeps every address and its stride at 0 mod 16, so that the host
picks the aligned form of the kernel for that side.

  dests    1..4 (16 KiB tiles), 5..8 (8 KiB tiles): every D the dispatcher
           instantiates; 9, 17 (passes of 8, the later ones with
           dest_base > 0)
  srcs     1, 2, 3, 32: the source loop is unrolled by two
  layouts  (source stride/phase, destination stride/phase), see LAYOUTS

Sources sit in an arena of random bytes, so a read outside a block changes
the result.  Destinations sit in an arena filled with 0xA5, each part
between 256-byte canaries; after a call the whole arena is compared, so
every byte that is not inside a destination block — canaries and the 4-byte
CRC slots between blocks — must still be 0xA5.
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
NBLOCKS = 5
S = 2
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

u8p = ctypes.POINTER(ctypes.c_uint8)
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


_pool = None


def source_pool():
    """Random [S, 32, NBLOCKS * BLOCK] bytes shared (read-only) by all cells."""
    global _pool
    if _pool is None:
        _pool = np.random.default_rng(6554).integers(
            0, 256, (S, 32, NBLOCKS * BLOCK), np.uint8)
        _pool.setflags(write=False)
    return _pool


_expected = {}


def expected(dests, srcs):
    """[(coef, tables, exp [S, dests, NBLOCKS*BLOCK])] for one cell, from the
    oracle; the last cell is kept, the layouts of one cell run in a row."""
    key = (dests, srcs)
    if key not in _expected:
        _expected.clear()
        out = []
        for coef in coef_matrices(dests, srcs, 100 * dests + srcs):
            tbl = oracle.init_tables(coef)
            exp = np.empty((S, dests, NBLOCKS * BLOCK), np.uint8)
            for s in range(S):
                outs = [np.full(NBLOCKS * BLOCK, 0x77, np.uint8)
                        for _ in range(dests)]
                oracle.ec_encode_data(
                    tbl, [np.ascontiguousarray(source_pool()[s, j])
                          for j in range(srcs)], outs)
                exp[s] = np.stack(outs)
            out.append((coef, tbl, exp))
        _expected[key] = out
    return _expected[key]


class Arena:
    """S * nparts parts of NBLOCKS blocks at `stride`, each between GUARD
    bytes; stripe 0 starts `phase` bytes past a 16-byte boundary, stripe 1
    at 8 mod 16 if the side is misaligned."""

    def __init__(self, nparts, stride, phase, fill=None, seed=0):
        self.nparts, self.stride = nparts, stride
        self.span = (NBLOCKS - 1) * stride + BLOCK
        self.slot = (GUARD + 16 + self.span + GUARD + 15) // 16 * 16
        n = S * nparts * self.slot
        if fill is None:
            self.host = np.random.default_rng(seed).integers(0, 256, n,
                                                             np.uint8)
        else:
            self.host = np.full(n, fill, np.uint8)
        phases = (phase, 8 if phase else 0)
        self.offs = np.array([(s * nparts + p) * self.slot + GUARD + phases[s]
                              for s in range(S) for p in range(nparts)],
                             np.int64)

    def place(self, data):
        """data [S, nparts, NBLOCKS*BLOCK] -> the blocks of self.host."""
        flat = data.reshape(S * self.nparts, NBLOCKS, BLOCK)
        for i, off in enumerate(self.offs):
            for b in range(NBLOCKS):
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
    return L.lib(), L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def call_strided(abi, tbl, srcs, dests, src, dst, nblocks=NBLOCKS,
                 src_ptrs=None, dst_ptrs=None, sstride=None, dstride=None):
    lib, eng = abi
    sp = src.ptrs if src_ptrs is None else src_ptrs
    dp = dst.ptrs if dst_ptrs is None else dst_ptrs
    return lib.lizec_ec_encode_batch_strided(
        eng, nblocks, srcs, dests, tbl.ctypes.data_as(u8p),
        sp.ctypes.data_as(u64p), dp.ctypes.data_as(u64p), S,
        src.stride if sstride is None else sstride,
        dst.stride if dstride is None else dstride, stream_arg())


def check_arena(dst, exp, what):
    """The whole destination arena: blocks equal exp, all else FILL."""
    torch.cuda.synchronize()
    got = dst.dev.cpu().numpy()
    want = Arena(dst.nparts, dst.stride, 0, fill=FILL)
    want.offs = dst.offs
    want.place(exp)
    if not np.array_equal(got, want.host):
        bad = np.flatnonzero(got != want.host)
        inside = np.zeros(got.size, bool)
        for off in dst.offs:
            for b in range(NBLOCKS):
                inside[off + b * dst.stride:off + b * dst.stride + BLOCK] = True
        pytest.fail(f"{what}: {bad.size} bytes differ, "
                    f"{int((~inside[bad]).sum())} of them outside every "
                    f"destination block; first offsets {bad[:6].tolist()}")


def run_cell(abi, dests, srcs, layout):
    (ss, sph), (ds, dph) = LAYOUTS[layout]
    src = Arena(srcs, ss, sph, seed=srcs)
    src.place(np.ascontiguousarray(source_pool()[:, :srcs]))
    src.upload()
    # the flags the host derives: aligned iff every address and the stride
    assert (all(p % 16 == 0 for p in src.ptrs) and ss % 16 == 0) == (sph == 0)
    for coef, tbl, exp in expected(dests, srcs):
        dst = Arena(dests, ds, dph, fill=FILL).upload()
        assert (all(p % 16 == 0 for p in dst.ptrs) and
                ds % 16 == 0) == (dph == 0)
        if dph:
            phases = {int(dst.ptrs[0] + b * ds) % 16 for b in range(NBLOCKS)}
            assert phases == {0, 4, 8, 12}
            assert int(dst.ptrs[dests]) % 16 == 8
        assert call_strided(abi, tbl, srcs, dests, src, dst) == LIZEC_OK
        check_arena(dst, exp, f"{layout} dests={dests} srcs={srcs}")
        assert np.array_equal(src.dev.cpu().numpy(), src.host), \
            "the sources were modified"


@pytest.mark.parametrize("layout", tuple(LAYOUTS))
@pytest.mark.parametrize("srcs", SRCS)
@pytest.mark.parametrize("dests", DESTS)
def test_strided_cell(abi, dests, srcs, layout):
    run_cell(abi, dests, srcs, layout)


def test_contiguous_aligned_equals_uniform_batch(abi):
    """Stride 65536 and full alignment: the call is lizec_ec_encode_batch at
    part_len = nblocks * 65536, and both equal the oracle."""
    lib, eng = abi
    dests, srcs = 5, 3
    src = Arena(srcs, BLOCK, 0, seed=1)
    src.place(np.ascontiguousarray(source_pool()[:, :srcs]))
    src.upload()
    coef, tbl, exp = expected(dests, srcs)[0]
    a = Arena(dests, BLOCK, 0, fill=FILL).upload()
    b = Arena(dests, BLOCK, 0, fill=FILL).upload()
    assert call_strided(abi, tbl, srcs, dests, src, a) == LIZEC_OK
    assert lib.lizec_ec_encode_batch(
        eng, NBLOCKS * BLOCK, srcs, dests, tbl.ctypes.data_as(u8p),
        src.ptrs.ctypes.data_as(u64p), b.ptrs.ctypes.data_as(u64p), S,
        stream_arg()) == LIZEC_OK
    check_arena(a, exp, "strided call")
    check_arena(b, exp, "uniform call")
    assert torch.equal(a.dev, b.dev)


REFUSALS = ("src address 2 mod 4", "dst address 2 mod 4", "src stride 65538",
            "dst stride 65538", "src stride 65532", "dst stride 65532",
            "nblocks 0", "src address 0", "dst address 0")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(abi, what):
    """Each returns LIZEC_EINVAL from the host and leaves the arena as it
    was.  The buffers are those of a valid il-il call, so the same call
    with the offending argument put right succeeds."""
    dests, srcs = 2, 3
    src = Arena(srcs, 65540, 4, seed=2)
    src.place(np.ascontiguousarray(source_pool()[:, :srcs]))
    src.upload()
    dst = Arena(dests, 65540, 4, fill=FILL).upload()
    coef, tbl, exp = expected(dests, srcs)[0]
    kw = {}
    side = "src" if what.startswith("src") else "dst"
    ptrs = (src if side == "src" else dst).ptrs.copy()
    if what.endswith("address 2 mod 4"):
        ptrs[-1] -= 2
        kw[side + "_ptrs"] = ptrs
    elif what.endswith("address 0"):
        ptrs[1] = 0
        kw[side + "_ptrs"] = ptrs
    elif "stride" in what:
        kw[side[0] + "stride"] = int(what.split()[-1])
    else:
        kw["nblocks"] = 0
    assert call_strided(abi, tbl, srcs, dests, src, dst, **kw) == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert bool((dst.dev == FILL).all()), "a refused call wrote the arena"
    assert call_strided(abi, tbl, srcs, dests, src, dst) == LIZEC_OK
    check_arena(dst, exp, "the valid call")
