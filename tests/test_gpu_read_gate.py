"""lizec_read_gate_batch — the batched hdd_read gate on the GPU — against the
independent restatement of hddspacemgr.cc:1525-1608 / :1662-1727 in
read_gate_cases.py and against lizec_read_gate_host.

The case table (read_gate_cases.world) is one call per flag value: 3-block
ec(3,2) part images of both formats (MooseFS blocks at 0 mod 16, INTERLEAVED
ones at 4, 8 and 12), every range of the issue at every placement 0..15 of
the packet against its source, past-end blocks, damage in turn, the sparse
rule, and overlapping blocks at odd addresses.  Packets lie in an arena of
0xA5 and the WHOLE arena is compared, so a byte written in front of or
behind a packet fails as surely as a wrong byte inside one.
"""
import ctypes
import zlib

import numpy as np
import pytest

import read_gate_cases as R

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

WAVES = 16384 * 4                    # the launch cap of lizec.h, in waves


def to_device(a):
    t = torch.from_numpy(np.array(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


@pytest.fixture(scope="module")
def dev():
    """The world's images on the device, its op table over them and the
    results of one call per flag value."""
    from lizardfs_amd import readgate as rg
    w = R.world()
    d_images = [to_device(im) for im in w.images]
    results = {}
    for sparse in (False, True):
        arena = torch.full((w.arena_size,), R.FILL, dtype=torch.uint8,
                           device="cuda")
        assert arena.data_ptr() % 16 == 0
        ops = w.ops(rg.OP_DTYPE, [t.data_ptr() for t in d_images],
                    arena.data_ptr())
        status = rg.gate_batch(ops, sparse=sparse)
        torch.cuda.synchronize()
        results[sparse] = (status.cpu().numpy(), arena.cpu().numpy(), ops)
    return dict(world=w, d_images=d_images, results=results)


def test_every_store_form_is_reached(dev):
    w = dev["world"]
    ops = dev["results"][False][2]
    sweep = w.select(lambda r: " sweep " in r.name)
    delta = {(int(o["out"]) + 4 - int(o["block"]) - int(o["offset"])) % 16
             for o in ops[sweep]}
    assert delta == set(range(16))
    assert {int(o["block"]) % 16 for o in ops[sweep]} == {0, 4, 8, 12}
    past = w.select(lambda r: r.boff is None)
    assert {(int(o["out"]) + 4 - int(o["offset"])) % 16 for o in ops[past]} >= \
        {0, 4, 8, 5, 11}


@pytest.mark.parametrize("sparse", (False, True))
def test_world_matches_restatement(dev, sparse):
    w = dev["world"]
    status, arena, _ = dev["results"][sparse]
    want_status, want_arena = w.expect(sparse)
    for i in np.flatnonzero(status != want_status)[:1]:
        pytest.fail(f"{w.reqs[i].name} (sparse={sparse}): status {status[i]},"
                    f" expected {want_status[i]}")
    bad = R.first_mismatch(arena, want_arena, w.starts, w.reqs)
    assert bad is None, f"sparse={sparse}: {bad}"


@pytest.mark.parametrize("sparse", (False, True))
def test_host_equals_device(dev, sparse):
    from lizardfs_amd import readgate as rg
    w = dev["world"]
    arena = R.aligned(w.arena_size, R.FILL)
    ops = w.ops(rg.OP_DTYPE, [im.ctypes.data for im in w.images],
                arena.ctypes.data)
    h_status = rg.gate_host(ops, sparse=sparse)
    d_status, d_arena, _ = dev["results"][sparse]
    assert np.array_equal(h_status, d_status)
    assert np.array_equal(arena, d_arena)


def test_more_ops_than_waves(dev):
    """n a few above the launch's wave count: seven waves take a second op,
    whose table entry they loaded while hashing the first."""
    from lizardfs_amd import readgate as rg
    w = dev["world"]
    n = WAVES + 7
    i = np.arange(n, dtype=np.int64)
    size = 1 + i % 32
    offset = (i * 40503) % (R.BLOCK - 32)
    which = i % 6                              # 3 blocks of either format
    starts = np.cumsum(4 + size + 1 + i % 3) - (4 + size)
    total = int(starts[-1] + 4 + size[-1] + 16)
    arena = torch.full((total,), R.FILL, dtype=torch.uint8, device="cuda")
    ops = np.zeros(n, rg.OP_DTYPE)
    boff = np.zeros(n, np.int64)
    for k in range(6):
        img = w.fmts.index(R.FORMATS[k // 3])
        data_off, crc_off, bstride, cstride = R.layout(R.FORMATS[k // 3])
        base = dev["d_images"][img].data_ptr()
        sel = which == k
        ops["block"][sel] = base + data_off + (k % 3) * bstride
        ops["stored"][sel] = base + crc_off + (k % 3) * cstride
        boff[sel] = data_off + (k % 3) * bstride
    ops["out"] = arena.data_ptr() + starts
    ops["offset"], ops["size"] = offset, size
    status = rg.gate_batch(ops)
    torch.cuda.synchronize()
    want = np.full(total, R.FILL, np.uint8)
    imgs = [w.images[w.fmts.index(f)] for f in R.FORMATS]
    for j in range(n):
        src = imgs[which[j] // 3]
        at = boff[j] + offset[j]
        body = src[at:at + size[j]]
        want[starts[j]:starts[j] + 4] = R.be32(zlib.crc32(body.tobytes()))
        want[starts[j] + 4:starts[j] + 4 + size[j]] = body
    assert (status.cpu().numpy() == R.OK).all()
    got = arena.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, \
        f"first wrong arena byte {bad[0]} (op " \
        f"{np.searchsorted(starts, bad[0], side='right') - 1} of {n})"


def test_refusals_leave_outputs_untouched(dev):
    from lizardfs_amd import lib as L
    from lizardfs_amd import readgate as rg
    w = dev["world"]
    arena = torch.full((w.arena_size,), R.FILL, dtype=torch.uint8,
                       device="cuda")
    good = w.ops(rg.OP_DTYPE, [t.data_ptr() for t in dev["d_images"]],
                 arena.data_ptr())[:6].copy()
    n = good.size
    status = torch.full((n,), -77, dtype=torch.int32, device="cuda")

    def broken(**fields):
        ops = good.copy()
        for k, v in fields.items():
            ops[-1][k] = v
        return ops

    def call(ops, cnt, flags, st=status, engine=True):
        o = ctypes.c_void_p(ops.ctypes.data) if ops is not None else None
        s = ctypes.c_void_p(st.data_ptr()) if st is not None else None
        r = L.lib().lizec_read_gate_batch(L.engine(0) if engine else None, o,
                                          cnt, flags, s, None)
        torch.cuda.synchronize()
        return r

    refused = [
        ("ops NULL", None, n, 0),
        ("n == 0", good, 0, 0),
        ("n > 2^24", good, (1 << 24) + 1, 0),
        ("size == 0", broken(size=0), n, 0),
        ("offset + size > 65536", broken(offset=65535, size=2), n, 0),
        ("size > 65536", broken(offset=0, size=65537), n, 0),
        ("offset >= 65536", broken(offset=65536, size=1), n, 0),
        ("out == 0", broken(out=0), n, 0),
        ("block without stored", broken(stored=0), n, 0),
        ("unknown flag bit", good, n, 2),
    ]
    assert good[-1]["block"] != 0
    for what, ops, cnt, flags in refused:
        assert call(ops, cnt, flags) == -2, what
    assert call(good, n, 0, st=None) == -2
    assert call(good, n, 0, engine=False) == -2
    assert (status.cpu().numpy() == -77).all()
    assert (arena.cpu().numpy() == R.FILL).all()
    with pytest.raises(L.LizecError):
        rg.gate_batch(broken(size=0))
    # a valid call afterwards is still right
    assert call(good, n, 0) == 0
    want_status, want_arena = w.expect(False)
    assert np.array_equal(status.cpu().numpy(), want_status[:n])
    end = int(w.starts[n - 1]) + 4 + w.reqs[n - 1].size
    got = arena.cpu().numpy()
    assert np.array_equal(got[:end], want_arena[:end])
    assert (got[end:] == R.FILL).all()


def test_call_sequences_share_the_stream_scratch(dev):
    """A large n then a small one, and a read gate right behind a write gate
    and a ranges call: all on one stream, whose scratch holds each call's
    tables in turn.  Nothing is synchronised in between."""
    from lizardfs_amd import crc as lcrc
    from lizardfs_amd import readgate as rg
    from lizardfs_amd import slice_traits as st
    from lizardfs_amd import writegate as wg
    w = dev["world"]
    slice_type = st.ec_slice_type(3, 2)
    want_status, want_arena = w.expect(False)
    addrs = [t.data_ptr() for t in dev["d_images"]]
    nreq = len(w.reqs)

    def read_call(sel):
        arena = torch.full((w.arena_size,), R.FILL, dtype=torch.uint8,
                           device="cuda")
        ops = w.ops(rg.OP_DTYPE, addrs, arena.data_ptr())[sel]
        return sel, arena, rg.gate_batch(ops)

    def check(call):
        sel, arena, status = call
        assert np.array_equal(status.cpu().numpy(), want_status[sel])
        want = np.full(w.arena_size, R.FILL, np.uint8)
        for i in sel:
            a, b = int(w.starts[i]), int(w.starts[i]) + 4 + w.reqs[i].size
            want[a:b] = want_arena[a:b]
        assert np.array_equal(arena.cpu().numpy(), want)

    big = read_call(list(range(nreq)))
    small = read_call([nreq - 1, 3])
    # a partial write into a clean block, then CRCs of two odd ranges
    fmt = "interleaved"
    k = w.fmts.index(fmt)
    img = dev["d_images"][k]
    data_off, _, bstride, _ = R.layout(fmt)
    payload = np.arange(4096, dtype=np.uint32).astype(np.uint8)
    d_payload = to_device(payload)
    wop = wg.make_op(img, fmt, slice_type, 1, 4096, d_payload, 0, 4096,
                     zlib.crc32(payload.tobytes()))
    wstatus, wnewcrc = wg.gate_batch([wop], sparse=True)
    crcs = lcrc.crc32_ranges(img, [5, 70001], [333, 65536])
    after = read_call([0, 17, nreq - 2])
    torch.cuda.synchronize()
    check(big)
    check(small)
    check(after)
    blk = w.images[k][data_off + bstride:data_off + bstride + R.BLOCK].copy()
    blk[4096:8192] = payload
    assert int(wstatus[0]) == 0
    assert int(wnewcrc.cpu().numpy().view(np.uint32)[0]) == \
        zlib.crc32(blk.tobytes())
    host = w.images[k]
    assert crcs.cpu().numpy().view(np.uint32).tolist() == \
        [zlib.crc32(host[5:338].tobytes()),
         zlib.crc32(host[70001:70001 + 65536].tobytes())]


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_read_packets(dev, fmt):
    from lizardfs_amd import readgate as rg
    from lizardfs_amd import slice_traits as st
    w = dev["world"]
    k = w.fmts.index(fmt)
    img, host = dev["d_images"][k], w.images[k]
    data_off, _, bstride, _ = R.layout(fmt)
    requests = [(0, 0, 65536), (1, 100, 3001), (2, 65535, 1), (3, 0, 65536),
                (5, 17, 40), (1, 0, 1), (2, 4096, 4096)]
    packets, starts, status = rg.read_packets(img, fmt, st.ec_slice_type(3, 2),
                                              requests)
    torch.cuda.synchronize()
    packets = packets.cpu().numpy()
    assert packets.size == sum(4 + r[2] for r in requests)
    assert (status.cpu().numpy() == R.OK).all()
    for (b, off, size), at in zip(requests, starts):
        body = packets[at + 4:at + 4 + size]
        if b < R.NBLOCKS:
            src = data_off + b * bstride + off
            assert np.array_equal(body, host[src:src + size])
        else:
            assert not body.any()
        assert int.from_bytes(bytes(packets[at:at + 4]), "big") == \
            zlib.crc32(body.tobytes())
