"""lizec_read_gate_host — hdd_read over hdd_read_crc_and_block
(hddspacemgr.cc:1525-1608, :1662-1727) over host memory — against the
independent restatement in read_gate_cases.py.  CPU-only.

  world      the full case table (ranges x placements x formats, past-end
             blocks, damage in turn, the sparse rule, overlapping blocks at
             any address), both flag values, the whole arena compared
  refusals   every LIZEC_EINVAL of lizec.h, status and arena left as they were
  packets    read_packets over numpy images in both formats
"""
import ctypes
import zlib

import numpy as np
import pytest

import read_gate_cases as R
from lizardfs_amd import lib as L
from lizardfs_amd import readgate as rg

LIZEC_EINVAL = -2


def test_op_struct_layout():
    assert rg.OP_DTYPE.itemsize == 32
    assert [rg.OP_DTYPE.fields[f][1] for f in
            ("block", "stored", "out", "offset", "size")] == [0, 8, 16, 24, 28]
    assert (rg.OK, rg.BAD_BLOCK, rg.SPARSE) == (R.OK, R.BAD_BLOCK, 1)


def test_layout_restated():
    from lizardfs_amd import scrub
    from lizardfs_amd import slice_traits as st
    for fmt in R.FORMATS:
        assert scrub.image_layout(fmt, st.ec_slice_type(3, 2)) == R.layout(fmt)


def test_world_covers_the_issue():
    """The table holds what it is meant to hold."""
    w = R.world()
    sweep = [r for r in w.reqs if " sweep " in r.name]
    assert {(r.offset, r.size) for r in sweep} == set(R.RANGES)
    assert {r.d for r in sweep} == set(range(16))
    assert {(r.boff + 0) % 16 for r in sweep} == {0, 4, 8, 12}
    for sparse in (False, True):
        status, _ = w.expect(sparse)
        assert set(status.tolist()) == {R.OK, R.BAD_BLOCK}
    plain, sp = w.expect(False)[0], w.expect(True)[0]
    for i in w.select(lambda r: "damage in" in r.name):
        bad = "clean block" not in w.reqs[i].name
        assert plain[i] == sp[i] == (R.BAD_BLOCK if bad else R.OK), \
            w.reqs[i].name
    for i in w.select(lambda r: "sparse:" in r.name):
        name = w.reqs[i].name
        if "stored 0" in name:
            assert (plain[i], sp[i]) == (R.BAD_BLOCK, R.OK), name
        elif "stored its CRC" in name:
            assert (plain[i], sp[i]) == (R.OK, R.OK), name
        else:
            assert (plain[i], sp[i]) == (R.BAD_BLOCK, R.BAD_BLOCK), name


@pytest.mark.parametrize("sparse", (False, True))
def test_world(sparse):
    w = R.world()
    arena = R.aligned(w.arena_size, R.FILL)
    ops = w.ops(rg.OP_DTYPE, [im.ctypes.data for im in w.images],
                arena.ctypes.data)
    status = rg.gate_host(ops, sparse=sparse)
    want_status, want_arena = w.expect(sparse)
    for i in np.flatnonzero(status != want_status)[:1]:
        pytest.fail(f"{w.reqs[i].name} (sparse={sparse}): status {status[i]},"
                    f" expected {want_status[i]}")
    bad = R.first_mismatch(arena, want_arena, w.starts, w.reqs)
    assert bad is None, f"sparse={sparse}: {bad}"


def test_refusals_leave_outputs_untouched():
    w = R.world()
    arena = R.aligned(w.arena_size, R.FILL)
    good = w.ops(rg.OP_DTYPE, [im.ctypes.data for im in w.images],
                 arena.ctypes.data)[:6].copy()
    n = good.size
    status = np.full(n, -77, np.int32)

    def broken(**fields):
        ops = good.copy()
        for k, v in fields.items():
            ops[-1][k] = v
        return ops

    def call(ops, cnt, flags, st=status):
        o = ctypes.c_void_p(ops.ctypes.data) if ops is not None else None
        s = ctypes.c_void_p(st.ctypes.data) if st is not None else None
        return L.lib().lizec_read_gate_host(o, cnt, flags, s)

    refused = [
        ("ops NULL", None, n, 0),
        ("n == 0", good, 0, 0),
        ("n > 2^24", good, (1 << 24) + 1, 0),
        ("size == 0", broken(size=0), n, 0),
        ("offset + size > 65536", broken(offset=65535, size=2), n, 0),
        ("size > 65536", broken(offset=0, size=65537), n, 0),
        ("offset >= 65536", broken(offset=65536, size=1), n, 0),
        ("offset wraps", broken(offset=0xFFFFFFFF, size=2), n, 0),
        ("out == 0", broken(out=0), n, 0),
        ("block without stored", broken(stored=0), n, 0),
        ("unknown flag bit", good, n, 2),
    ]
    assert good[-1]["block"] != 0
    for what, ops, cnt, flags in refused:
        assert call(ops, cnt, flags) == LIZEC_EINVAL, what
    assert call(good, n, 0, st=None) == LIZEC_EINVAL
    assert (status == -77).all()
    assert (arena == R.FILL).all()
    # stored is ignored for a past-end block, and a valid call still works
    assert call(broken(block=0, stored=0), n, 0) == 0
    assert call(good, n, 0) == 0
    want_status, want_arena = w.expect(False)
    assert (status == want_status[:n]).all()
    end = int(w.starts[n - 1]) + 4 + w.reqs[n - 1].size
    assert np.array_equal(arena[:end], want_arena[:end])
    assert (arena[end:] == R.FILL).all()
    with pytest.raises(L.LizecError):
        rg.gate_host(broken(size=0))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_read_packets_host(fmt):
    from lizardfs_amd import slice_traits as st
    w = R.world()
    img = w.images[w.fmts.index(fmt)]
    data_off, _, bstride, _ = R.layout(fmt)
    requests = [(0, 0, 65536), (1, 100, 3001), (2, 65535, 1), (3, 0, 65536),
                (5, 17, 40), (1, 0, 1)]
    packets, starts, status = rg.read_packets(img, fmt, st.ec_slice_type(3, 2),
                                              requests)
    assert packets.size == sum(4 + r[2] for r in requests)
    assert (status == R.OK).all()
    for (b, off, size), at in zip(requests, starts):
        body = packets[at + 4:at + 4 + size]
        if b < R.NBLOCKS:
            src = data_off + b * bstride + off
            assert np.array_equal(body, img[src:src + size])
        else:
            assert not body.any()
        assert int.from_bytes(bytes(packets[at:at + 4]), "big") == \
            zlib.crc32(body.tobytes())
