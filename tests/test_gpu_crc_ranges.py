"""lizec_crc32_ranges — CRC32 of byte ranges of any length and alignment —
against zlib.crc32 and oracle.crc32 (which must agree first).

  edge sweep     31 lengths around every boundary of the kernel (head/tail
                 bytes, one unit, one unit per lane, the 8/4/2/1 burst
                 ladder, a full block) x start alignments 0..15, one call
  outside bytes  the same call with the 16 bytes before and behind every
                 range inverted gives the same CRCs
  grid stride    the launch has at most 16384 workgroups x 4 waves = 65536
                 waves (lizec.h, crc.RANGES_GRID_WAVES); 2 x 65536 + 37
                 ranges make every wave take at least two
  sequences      on a stream of its own, whose scratch nothing has grown
                 yet: small call, one that grows the scratch (more than
                 2^16 u64 slots: over 43690 ranges), small again; the same
                 between crc32_blocks calls
  refusals       every LIZEC_EINVAL of lizec.h, device output untouched
"""
import ctypes
import zlib

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_EINVAL = -2
SEEDS = (0, 0xABCD1234)
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65,
           255, 256, 257, 1023, 1024, 1025, 1040,
           4095, 4096, 4097, 16383, 16384,
           65519, 65520, 65535, 65536)
GUARD = 16


@pytest.fixture(scope="module")
def crc_mod():
    from lizardfs_amd import crc
    return crc


def aligned_device(host):
    """Device copy of host whose first byte is 16-byte aligned."""
    raw = torch.empty(host.size + 16, dtype=torch.uint8, device="cuda")
    skew = (-raw.data_ptr()) % 16
    buf = raw[skew:skew + host.size]
    assert buf.data_ptr() % 16 == 0
    buf.copy_(torch.from_numpy(host))
    return buf


def expected(host, offs, lens, seed, oracle_every=1):
    mv = memoryview(host)
    exp = np.array([zlib.crc32(mv[o:o + n], seed)
                    for o, n in zip(offs, lens)], np.uint32)
    for i in range(0, len(offs), oracle_every):
        o, n = int(offs[i]), int(lens[i])
        assert oracle.crc32(host[o:o + n].tobytes(), seed) == exp[i], \
            "the two references disagree"
    return exp


def gpu(crc_mod, buf, offs, lens, seed):
    got = crc_mod.crc32_ranges(buf, offs, lens, seed=seed)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint32)


def mismatch(got, exp, offs, lens):
    bad = np.flatnonzero(got != exp)
    return [(int(offs[i]) % 16, int(lens[i]), hex(got[i]), hex(exp[i]))
            for i in bad[:8]]


@pytest.fixture(scope="module")
def sweep():
    """496 ranges, each with GUARD bytes of its own on both sides, in a
    buffer whose device copy is 16-byte aligned; expected CRCs per seed."""
    offs, lens = [], []
    cursor = 0
    for n in LENGTHS:
        for align in range(16):
            start = (cursor + 15) // 16 * 16 + GUARD + align
            offs.append(start)
            lens.append(n)
            cursor = start + n + GUARD
    rng = np.random.default_rng(77)
    host = rng.integers(0, 256, cursor, np.uint8)
    offs, lens = np.array(offs, np.int64), np.array(lens, np.int64)
    assert len(offs) == 496 and host.size < 6 << 20
    exp = {s: expected(host, offs, lens, s) for s in SEEDS}
    return host, offs, lens, exp


def test_edge_sweep_one_call(crc_mod, sweep):
    host, offs, lens, exp = sweep
    buf = aligned_device(host)
    assert set((buf.data_ptr() + offs) % 16) == set(range(16))
    for seed in SEEDS:
        got = gpu(crc_mod, buf, offs, lens, seed)
        assert np.array_equal(got, exp[seed]), \
            f"seed {seed:#x}: (align, len, got, exp) " \
            f"{mismatch(got, exp[seed], offs, lens)}"


def test_outside_bytes_do_not_count(crc_mod, sweep):
    host, offs, lens, exp = sweep
    flipped = host.copy()
    for o, n in zip(offs, lens):
        flipped[o - GUARD:o] ^= 0xFF
        flipped[o + n:o + n + GUARD] ^= 0xFF
    # the ranges themselves are as before
    assert all(np.array_equal(flipped[o:o + n], host[o:o + n])
               for o, n in zip(offs, lens))
    buf = aligned_device(flipped)
    for seed in SEEDS:
        got = gpu(crc_mod, buf, offs, lens, seed)
        assert np.array_equal(got, exp[seed]), \
            f"seed {seed:#x}: {mismatch(got, exp[seed], offs, lens)}"


def test_known_answers_at_odd_addresses(crc_mod):
    host = np.zeros(8192, np.uint8)
    host[1:2] = np.frombuffer(b"a", np.uint8)
    host[35:44] = np.frombuffer(b"123456789", np.uint8)
    host[4097:4097 + 3001] = 0xFF
    offs = np.array([1, 35, 101, 4097, 4099, 103])
    lens = np.array([1, 9, 3003, 3001, 17, 0])
    buf = aligned_device(host)
    assert all((buf.data_ptr() + o) % 2 == 1 for o in offs)
    got = gpu(crc_mod, buf, offs, lens, 0)
    assert got[0] == 0xE8B7BE43 and got[1] == 0xCBF43926
    assert np.array_equal(got, expected(host, offs, lens, 0))
    assert got[2] == zlib.crc32(bytes(3003))          # all zero
    assert got[3] == zlib.crc32(b"\xff" * 3001)       # all 0xFF
    assert got[5] == 0                                # empty range, seed 0
    got = gpu(crc_mod, buf, offs, lens, 0xABCD1234)
    assert np.array_equal(got, expected(host, offs, lens, 0xABCD1234))
    assert got[5] == 0xABCD1234                       # empty range = seed


def test_overlapping_and_repeated_ranges(crc_mod):
    rng = np.random.default_rng(78)
    host = rng.integers(0, 256, 70000, np.uint8)
    offs, lens = [], []
    for k in range(3):                      # the same range three times
        offs.append(777), lens.append(5000)
    for k in range(20):                     # one byte apart, overlapping
        offs.append(1000 + k), lens.append(3000 + 7 * k)
    for k in range(10):                     # nested around one centre
        offs.append(30000 - 100 * k), lens.append(200 * k + 1)
    offs += [0, 0, 4464, 69999, 70000]      # whole blocks, last byte, empty
    lens += [65536, 65536, 65536, 1, 0]
    offs, lens = np.array(offs), np.array(lens)
    buf = aligned_device(host)
    for seed in SEEDS:
        got = gpu(crc_mod, buf, offs, lens, seed)
        assert np.array_equal(got, expected(host, offs, lens, seed))
    assert got[0] == got[1] == got[2]


def short_ranges(n, seed):
    """n ranges of lengths 0..48 packed back to back (every alignment)."""
    lens = np.arange(n, dtype=np.int64) % 49
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, int(lens.sum()), np.uint8)
    return host, offs, lens


def test_grid_stride(crc_mod):
    waves = crc_mod.RANGES_GRID_WAVES
    assert waves == 16384 * 4
    n = 2 * waves + 37
    host, offs, lens = short_ranges(n, 79)
    buf = aligned_device(host)
    got = gpu(crc_mod, buf, offs, lens, 0)
    exp = expected(host, offs, lens, 0, oracle_every=97)
    assert np.array_equal(got, exp), mismatch(got, exp, offs, lens)


def test_call_sequence_on_one_stream(crc_mod):
    small_h, small_o, small_l = short_ranges(5, 80)
    big_h, big_o, big_l = short_ranges(70000, 81)    # > 43690: scratch grows
    blk_h = np.random.default_rng(82).integers(0, 256, 4 * 65536, np.uint8)
    small, big, blk = (aligned_device(h) for h in (small_h, big_h, blk_h))
    small_e = expected(small_h, small_o, small_l, 0)
    big_e = expected(big_h, big_o, big_l, 0, oracle_every=97)
    blk_e = oracle.crc32_blocks(blk_h, 65536)

    def ranges(buf, o, l):
        return crc_mod.crc32_ranges(buf, o, l)

    # The engine keeps its call scratch per stream, and another test of this
    # process (test_grid_stride) may already have grown the default stream's
    # past what the large call needs.  A stream made here has no scratch
    # yet: the first small call allocates the initial 2^16 slots, and the
    # 70000-range call (105000 slots) really frees and reallocates them
    # while the small call's kernel may still be running.
    torch.cuda.synchronize()                 # the buffers are in place
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    assert big_l.size + (big_l.size + 1) // 2 > 1 << 16
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream
        # no synchronisation between the calls: the stream orders them
        a = ranges(small, small_o, small_l)
        b = ranges(big, big_o, big_l)
        c = ranges(small, small_o, small_l)
        d = crc_mod.crc32_blocks(blk, 65536)
        e = ranges(small, small_o, small_l)
        f = crc_mod.crc32_blocks(blk, 65536)
        g = ranges(big, big_o, big_l)
        h = ranges(small, small_o, small_l)
    side.synchronize()
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)
    for name, t in (("first small", a), ("small after growth", c),
                    ("small after blocks", e), ("last small", h)):
        assert np.array_equal(u(t), small_e), name
    for name, t in (("growing call", b), ("large after blocks", g)):
        assert np.array_equal(u(t), big_e), name
    for name, t in (("blocks after ranges", d), ("blocks again", f)):
        assert np.array_equal(u(t), blk_e), name


def test_out_tensor_and_wrapper_checks(crc_mod):
    host = np.arange(100, dtype=np.uint8)
    buf = aligned_device(host)
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    ret = crc_mod.crc32_ranges(buf, [3, 50], [10, 50], out=out)
    torch.cuda.synchronize()
    assert ret is out
    assert np.array_equal(out.cpu().numpy().view(np.uint32),
                          expected(host, [3, 50], [10, 50], 0))
    # no ranges: an empty tensor, no call into the library
    none = crc_mod.crc32_ranges(buf, np.zeros(0, np.int64),
                                np.zeros(0, np.int64))
    assert none.shape == (0,) and none.dtype == torch.int32 and none.is_cuda
    with pytest.raises(ValueError):
        crc_mod.crc32_ranges(buf, [51], [50])          # one byte past the end
    with pytest.raises(ValueError):
        crc_mod.crc32_ranges(buf, [-1], [5])
    with pytest.raises(ValueError):
        crc_mod.crc32_ranges(buf, [0, 1], [5])
    with pytest.raises(ValueError):
        crc_mod.crc32_ranges(buf.cpu(), [0], [5])


def test_refusals_leave_output_untouched(crc_mod):
    from lizardfs_amd import lib as L
    buf = aligned_device(np.zeros(70000, np.uint8))
    base = buf.data_ptr()
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)

    def call(dptrs, lens, n, outp=None):
        d = None if dptrs is None else \
            np.array(dptrs, np.uint64).ctypes.data_as(u64p)
        l = None if lens is None else \
            np.array(lens, np.uint32).ctypes.data_as(u32p)
        o = ctypes.c_void_p(out.data_ptr()) if outp is None else outp
        r = L.lib().lizec_crc32_ranges(L.engine(0), d, l, n, 0, o, None)
        torch.cuda.synchronize()
        return r

    good = ([base, base + 1, 0, base + 3], [16, 65536, 0, 5])
    assert call(None, good[1], 4) == LIZEC_EINVAL
    assert call(good[0], None, 4) == LIZEC_EINVAL
    assert call(good[0], good[1], 4, ctypes.c_void_p(None)) == LIZEC_EINVAL
    assert call(good[0], good[1], 0) == LIZEC_EINVAL
    assert call(good[0], good[1], (1 << 24) + 1) == LIZEC_EINVAL
    assert call(good[0], [16, 65537, 0, 5], 4) == LIZEC_EINVAL
    assert call([base, base + 1, 0, 0], good[1], 4) == LIZEC_EINVAL
    assert (out.cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all()
    # the unbroken call is accepted; length 0 at address 0 gives the seed
    assert call(*good, 4) == 0
    got = out.cpu().numpy().view(np.uint32)
    assert got[0] == zlib.crc32(bytes(16)) and got[1] == zlib.crc32(bytes(65536))
    assert got[2] == 0 and got[3] == zlib.crc32(bytes(5))
