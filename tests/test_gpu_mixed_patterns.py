"""GPU tests for per-stripe erasure patterns in one recover batch
(ReedSolomon.recover_batch_mixed -> lizec_ec_encode_batch_multi ->
ec_encode_multi_kernel).  Shapes are the smallest at which each kernel path
can still go wrong; every comparison is bit-exact against the CPU oracle.
"""
import ctypes

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_EINVAL = -2


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_stripes(k, m, S, plen, seed):
    """Oracle-encoded stripes: uint8 [S, k+m, plen]."""
    rng = np.random.default_rng(seed)
    parts = np.empty((S, k + m, plen), np.uint8)
    parts[:, :k] = rng.integers(0, 256, (S, k, plen), np.uint8)
    for s in range(S):
        par = oracle.rs_encode(k, m, [np.ascontiguousarray(parts[s, i])
                                      for i in range(k)], plen)
        for j in range(m):
            parts[s, k + j] = par[j]
    return parts


def device_fragments(parts, erased):
    """Strided [S, L] row views of one [S, k+m, L] device tensor; the rows
    of every erased part are overwritten with junk first — they must be
    ignored."""
    junk = parts.copy()
    for s, e in enumerate(erased):
        for i in e:
            junk[s, i] = 0x5A
    full = to_gpu(junk)
    return [full[:, i, :] for i in range(parts.shape[1])]


def oracle_recover(k, m, parts, s, erased, want):
    frags = [None if i in erased else np.ascontiguousarray(parts[s, i])
             for i in range(k + m)]
    mask = 0
    for i in erased:
        mask |= 1 << i
    return oracle.rs_recover(k, m, frags, mask, set(want), parts.shape[2])


def check_against_oracle(k, m, parts, erased, want, got, slots, fill=None):
    S, oc = slots.shape
    for s in range(S):
        exp = oracle_recover(k, m, parts, s, erased[s], want[s])
        assert [p for p in slots[s] if p >= 0] == sorted(want[s])
        for j in range(oc):
            part = int(slots[s, j])
            if part >= 0:
                assert np.array_equal(got[s, j], exp[part]), \
                    f"stripe {s} slot {j} (part {part})"
            elif fill is not None:
                assert (got[s, j] == fill).all(), \
                    f"stripe {s}: unused slot {j} was written"


@pytest.fixture(scope="module")
def rs_mod():
    from lizardfs_amd.ec import ReedSolomon
    return ReedSolomon


def test_pattern_interleave(rs_mod):
    """ec(8,2), D=2/CH=4: one full 16 KiB tile + a ragged tail per stripe,
    adjacent tiles on different tables."""
    k, m, S, plen = 8, 2, 12, 16384 + 32
    pats = [(1, 5), (3, 8), (8, 9), (0, 7), (2, 9)]
    erased = [set(pats[s % len(pats)]) for s in range(S)]
    parts = make_stripes(k, m, S, plen, 11)
    rs = rs_mod(k, m)
    out, slots = rs.recover_batch_mixed(device_fragments(parts, erased),
                                        erased)
    rs.sync()
    assert tuple(out.shape) == (S, m, plen)
    check_against_oracle(k, m, parts, erased, erased, out.cpu().numpy(),
                         slots)


def test_wide_geometry(rs_mod):
    """ec(32,6): D=6 uses 2-chunk (8 KiB) tiles; ragged tail only."""
    k, m, S, plen = 32, 6, 4, 4096 + 16
    erased = [{0, 1, 2, 3, 4, 5}, {7, 13, 31, 32, 35, 37},
              {32, 33, 34, 35, 36, 37}, {5, 10, 15, 20, 25, 30}]
    parts = make_stripes(k, m, S, plen, 12)
    rs = rs_mod(k, m)
    out, slots = rs.recover_batch_mixed(device_fragments(parts, erased),
                                        erased)
    rs.sync()
    assert tuple(out.shape) == (S, 6, plen)
    check_against_oracle(k, m, parts, erased, erased, out.cpu().numpy(),
                         slots)


def test_pass_split(rs_mod):
    """ec(2,9): nine destinations run as passes of 8 + 1, the second with
    dest_base = 8 inside every stripe's own table."""
    k, m, S, plen = 2, 9, 3, 1024
    survivors = [(0, 1), (0, 5), (3, 10)]
    erased = [set(range(k + m)) - set(sv) for sv in survivors]
    parts = make_stripes(k, m, S, plen, 13)
    rs = rs_mod(k, m)
    out, slots = rs.recover_batch_mixed(device_fragments(parts, erased),
                                        erased)
    rs.sync()
    assert tuple(out.shape) == (S, 9, plen)
    check_against_oracle(k, m, parts, erased, erased, out.cpu().numpy(),
                         slots)


def test_skipped_destinations(rs_mod):
    """Want sizes alternate 1 and 2: the unused slot of a 1-part stripe is
    passed as address 0 and must keep its pre-filled bytes."""
    k, m, S, plen = 8, 2, 6, 4096 + 16
    erased = [{0, 3}, {2, 9}, {8, 9}, {4, 6}, {1, 8}, {5, 7}]
    want = [{3}, {2, 9}, {9}, {4, 6}, {1}, {5, 7}]
    parts = make_stripes(k, m, S, plen, 14)
    rs = rs_mod(k, m)
    out = torch.full((S, 2, plen), 0xA5, dtype=torch.uint8, device="cuda")
    got, slots = rs.recover_batch_mixed(device_fragments(parts, erased),
                                        erased, want=want, out=out)
    rs.sync()
    assert got.data_ptr() == out.data_ptr()
    assert (slots[:, 1] < 0).tolist() == [True, False] * 3
    check_against_oracle(k, m, parts, erased, want, out.cpu().numpy(), slots,
                         fill=0xA5)


def test_grid_stride_restage(rs_mod):
    """ec(2,1), one 16-byte tile per stripe, three stripes more than the
    grid cap of 1,048,576 blocks: the only shape at which a block runs a
    second tile, and that tile names a different table than the first.
    ec(2,1) parity is d0 ^ d1, so every part is the XOR of the other two."""
    k, m, plen = 2, 1, 16
    S = 1048576 + 3
    rng = np.random.default_rng(15)
    parts = np.empty((S, 3, plen), np.uint8)
    parts[:, :2] = rng.integers(0, 256, (S, 2, plen), np.uint8)
    parts[:, 2] = parts[:, 0] ^ parts[:, 1]
    gone = (np.arange(S) % 3).astype(np.int64)
    rows = np.arange(S)
    junk = parts.copy()
    junk[rows, gone] = 0x5A
    full = to_gpu(junk)
    rs = rs_mod(k, m)
    out, slots = rs.recover_batch_mixed([full[:, i, :] for i in range(3)],
                                        gone.reshape(S, 1))
    rs.sync()
    got = out.cpu().numpy()
    assert got.shape == (S, 1, plen)
    assert np.array_equal(slots[:, 0], gone)
    a, b = (gone + 1) % 3, (gone + 2) % 3
    exp = parts[rows, a] ^ parts[rows, b]
    bad = np.flatnonzero((got[:, 0] != exp).any(axis=1))
    assert bad.size == 0, f"{bad.size} stripes differ, first {bad[:8]}"
    for s in range(64):
        e = int(gone[s])
        assert np.array_equal(
            got[s, 0], oracle_recover(k, m, parts, s, {e}, {e})[e]), s


def test_grid_stride_restage_distinct_tables(rs_mod):
    """The same over-the-grid-cap shape with ec(2,2).  In ec(2,1) every part
    is the XOR of the other two, so its three tables hold the same bytes and
    a block that kept its first table would still pass; here the three
    patterns have different coefficients.  The stripes are cut from one long
    oracle-encoded stripe (RS coding is bytewise), so the expected bytes are
    the original parts."""
    k, m, plen = 2, 2, 16
    S = 1048576 + 3
    rng = np.random.default_rng(17)
    long_data = [rng.integers(0, 256, S * plen, np.uint8) for _ in range(k)]
    long_parts = long_data + oracle.rs_encode(k, m, long_data, S * plen)
    parts = np.ascontiguousarray(
        np.stack([p.reshape(S, plen) for p in long_parts], axis=1))
    pats = np.array([[0, 1], [0, 2], [1, 3]])
    erased = pats[np.arange(S) % 3]
    rows = np.arange(S)
    junk = parts.copy()
    for j in range(m):
        junk[rows, erased[:, j]] = 0x5A
    full = to_gpu(junk)
    rs = rs_mod(k, m)
    out, slots = rs.recover_batch_mixed(
        [full[:, i, :] for i in range(k + m)], erased)
    rs.sync()
    got = out.cpu().numpy()
    assert got.shape == (S, m, plen)
    assert np.array_equal(slots, erased)
    for j in range(m):
        exp = parts[rows, erased[:, j]]
        bad = np.flatnonzero((got[:, j] != exp).any(axis=1))
        assert bad.size == 0, \
            f"slot {j}: {bad.size} stripes differ, first {bad[:8]}"
    for s in list(range(32)) + list(range(S - 32, S)):
        e = set(erased[s].tolist())
        exp = oracle_recover(k, m, parts, s, e, e)
        for j in range(m):
            assert np.array_equal(got[s, j], exp[int(slots[s, j])]), (s, j)


def test_uniform_equivalence(rs_mod):
    """One pattern, ntables = 1: byte-identical to recover_batch; a plan
    from lizec_ec_plan_create_multi, run twice, matches the batch call."""
    k, m, S, plen = 8, 2, 5, 16384 + 32
    pat = (2, 8)
    erased = [set(pat)] * S
    parts = make_stripes(k, m, S, plen, 16)
    frags = device_fragments(parts, erased)
    rs = rs_mod(k, m)

    ref = rs.recover_batch([None if i in pat else frags[i]
                            for i in range(k + m)], erased=pat)
    batch, slots = rs.recover_batch_mixed(frags, erased)
    rs.sync()
    assert slots.tolist() == [sorted(pat)] * S
    for j, part in enumerate(sorted(pat)):
        assert torch.equal(batch[:, j, :], ref[part]), f"part {part}"
        assert np.array_equal(ref[part].cpu().numpy(), parts[:, part])

    out = torch.zeros((S, m, plen), dtype=torch.uint8, device="cuda")
    nplans = len(rs._plans)
    for run in range(2):
        out.fill_(0xEE)
        rs.recover_batch_mixed(frags, erased, out=out)
        rs.sync()
        assert torch.equal(out, batch), f"plan run {run}"
    assert len(rs._plans) == nplans + 1, "the plan is built once and reused"


def test_argument_checks(rs_mod):
    """An index equal to ntables and ntables = 0 are refused on the host:
    LIZEC_EINVAL, nothing launched, output untouched."""
    from lizardfs_amd import lib as L
    from lizardfs_amd.ec import build_pattern_tables
    k, m, S, plen = 8, 2, 4, 4096
    rs = rs_mod(k, m)
    lib, eng = L.lib(), L.engine(0)
    tables, index, _ = build_pattern_tables(k, m, [{0, 1}, {2, 3}] * 2)
    ntables = tables.shape[0]
    assert ntables == 2
    src_t = torch.zeros((S, k, plen), dtype=torch.uint8, device="cuda")
    out = torch.full((S, m, plen), 0xA5, dtype=torch.uint8, device="cuda")
    src = src_t.data_ptr() + np.arange(S * k, dtype=np.uint64) * np.uint64(plen)
    dst = out.data_ptr() + np.arange(S * m, dtype=np.uint64) * np.uint64(plen)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)

    def call(nt, idx):
        idx = np.ascontiguousarray(idx, np.uint32)
        args = (eng, plen, k, m, tables.ctypes.data_as(u8p), nt,
                idx.ctypes.data_as(u32p), src.ctypes.data_as(u64p),
                dst.ctypes.data_as(u64p), S)
        plan = ctypes.c_void_p()
        rcs = (lib.lizec_ec_encode_batch_multi(*args, stream),
               lib.lizec_ec_plan_create_multi(*args, ctypes.byref(plan)))
        assert not plan.value
        return rcs

    bad = index.copy()
    bad[S - 1] = ntables
    assert call(ntables, bad) == (LIZEC_EINVAL, LIZEC_EINVAL)
    assert call(0, index) == (LIZEC_EINVAL, LIZEC_EINVAL)
    rs.sync()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()), "a refused call wrote to the output"


def test_alignment_checks(rs_mod):
    """A nonzero source or destination address that is not 16-byte aligned
    is refused on the host by the batch, multi-table and both plan entry
    points: LIZEC_EINVAL, no plan returned, output untouched.  The Python
    entry points raise ValueError naming the tensor."""
    from lizardfs_amd import lib as L
    from lizardfs_amd.ec import build_pattern_tables
    k, m, S, plen = 8, 2, 4, 4096
    rs = rs_mod(k, m)
    lib, eng = L.lib(), L.engine(0)
    tables, index, _ = build_pattern_tables(k, m, [{0, 1}, {2, 3}] * 2)
    src_t = torch.zeros((S * k * plen + 64,), dtype=torch.uint8,
                        device="cuda")
    out = torch.full((S * m * plen + 64,), 0xA5, dtype=torch.uint8,
                     device="cuda")
    assert src_t.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    src = src_t.data_ptr() + np.arange(S * k, dtype=np.uint64) * np.uint64(plen)
    dst = out.data_ptr() + np.arange(S * m, dtype=np.uint64) * np.uint64(plen)
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)

    def call(src, dst):
        src = np.ascontiguousarray(src, np.uint64)
        dst = np.ascontiguousarray(dst, np.uint64)
        tail = (src.ctypes.data_as(u64p), dst.ctypes.data_as(u64p), S)
        one = (eng, plen, k, m, tables[0].ctypes.data_as(u8p)) + tail
        multi = (eng, plen, k, m, tables.ctypes.data_as(u8p),
                 tables.shape[0], index.ctypes.data_as(u32p)) + tail
        plan, mplan = ctypes.c_void_p(), ctypes.c_void_p()
        rcs = (lib.lizec_ec_encode_batch(*one, stream),
               lib.lizec_ec_plan_create(*one, ctypes.byref(plan)),
               lib.lizec_ec_encode_batch_multi(*multi, stream),
               lib.lizec_ec_plan_create_multi(*multi, ctypes.byref(mplan)))
        assert not plan.value and not mplan.value
        return rcs

    refused = (LIZEC_EINVAL,) * 4
    for off in (1, 4, 8):
        for at in (0, S * k - 1):          # first and last source
            bad = src.copy()
            bad[at] += np.uint64(off)
            assert call(bad, dst) == refused, ("src", at, off)
        for at in (0, S * m - 1):
            bad = dst.copy()
            bad[at] += np.uint64(off)
            assert call(src, bad) == refused, ("dst", at, off)
    rs.sync()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()), "a refused call wrote to the output"

    # the wrappers name the misaligned tensor
    data = src_t[8:8 + S * k * plen].view(S, k, plen)
    with pytest.raises(ValueError, match="data.*16-byte aligned"):
        rs.encode_batch(data)
    good = src_t[:S * k * plen].view(S, k, plen)
    parity = out[4:4 + S * m * plen].view(S, m, plen)
    with pytest.raises(ValueError, match="parity.*16-byte aligned"):
        rs.encode_batch(good, parity)
    frags = [None, None] + [good[:, i, :] for i in range(2, k)] + \
        [src_t[8:8 + S * plen].view(S, plen), good[:, 0, :]]
    with pytest.raises(ValueError, match="fragment 8.*16-byte aligned"):
        rs.recover_batch(frags, erased=(0, 1))
    mixed = [good[:, i, :] for i in range(k)] + \
        [good[:, 0, :], src_t[8:8 + S * plen].view(S, plen)]
    with pytest.raises(ValueError, match="fragment 9.*16-byte aligned"):
        rs.recover_batch_mixed(mixed, [{0, 1}] * S)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
