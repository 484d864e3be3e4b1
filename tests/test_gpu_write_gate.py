"""lizec_write_gate_batch — the batched hdd_write gate on the GPU — over
device images of both on-disk formats, against the Python restatement of
hddspacemgr.cc:1918-2001 on the oracle (gate_cases.restate), zlib's CRC of
the written block, the scrub, and lizec_write_gate_host.

Every case that names a block gets a 3-block image of its own: an ec(3,2)
MooseFS part (blocks 16-byte aligned, CRC array at 1024) and an INTERLEAVED
part (block b at 4 + 65540 b: 4, 8 and 12 mod 16; CRCs inline).  The case's
block sits at index i % 3, the other two are clean, so the scrub names
exactly the block the gate names.  Data lies at alignments 0..15.
"""
import zlib

import numpy as np
import pytest

import gate_cases as G

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FORMATS = ("moosefs", "interleaved")
NBLOCKS = 3


class Placed:
    """One case placed in an image of one format."""

    def __init__(self, case, fmt, image, bindex, data_off):
        self.case, self.fmt = case, fmt
        self.image, self.bindex, self.data_off = image, bindex, data_off


@pytest.fixture(scope="module")
def world():
    """Host images, the data buffer and the placed cases; the device copies;
    the device results for both flag values."""
    from lizardfs_amd import scrub, writegate as wg
    from lizardfs_amd import slice_traits as st
    slice_type = st.ec_slice_type(3, 2)
    rng = np.random.default_rng(4242)
    cases = G.sweep_cases() + G.sparse_cases()
    images, placed, data_parts = [], [], []
    cursor = 0
    for fmt in FORMATS:
        layout = scrub.image_layout(fmt, slice_type)
        clean = len(images)          # a clean image for the "no block" ops
        images.append(scrub.build_chunk_image(
            7, 1, slice_type, 0,
            [rng.integers(0, 256, G.BLOCK, np.uint8) for _ in range(NBLOCKS)],
            crc32_fn=zlib.crc32, fmt=fmt))
        for i, c in enumerate(cases):
            # data at alignment i % 16 of a 16-byte aligned buffer
            start = (cursor + 15) // 16 * 16 + i % 16
            data_parts.append((start, c.data))
            cursor = start + c.size
            if c.block is None:
                placed.append(Placed(c, fmt, clean, NBLOCKS, start))
                continue
            b = i % NBLOCKS
            blocks = [rng.integers(0, 256, G.BLOCK, np.uint8)
                      for _ in range(NBLOCKS)]
            blocks[b] = c.orig
            img = scrub.build_chunk_image(7, 1, slice_type, 0, blocks,
                                          crc32_fn=zlib.crc32, fmt=fmt)
            data_off, crc_off, bstride, cstride = layout
            at = data_off + b * bstride
            img[at:at + G.BLOCK] = c.block          # the flipped byte, if any
            if c.stored is not None:
                img[crc_off + b * cstride:crc_off + b * cstride + 4] = c.stored
            placed.append(Placed(c, fmt, len(images), b, start))
            images.append(img)
    data = np.zeros(cursor + 1, np.uint8)
    for start, d in data_parts:
        data[start:start + d.size] = d

    d_images = [torch.from_numpy(img).cuda() for img in images]
    d_data = torch.from_numpy(data).cuda()
    assert d_data.data_ptr() % 16 == 0
    assert all(t.data_ptr() % 16 == 0 for t in d_images)

    def ops_over(imgs, dat):
        return wg.ops_array([
            wg.make_op(imgs[p.image], p.fmt, slice_type, p.bindex,
                       p.case.offset, dat, p.data_off, p.case.size,
                       p.case.claimed) for p in placed])

    d_ops = ops_over(d_images, d_data)
    assert set(int(a) % 16 for a in d_ops["data"][d_ops["size"] > 0]) == \
        set(range(16))
    assert {int(a) % 16 for a in d_ops["block"] if a} == {0, 4, 8, 12}
    results = {}
    for sparse in (False, True):          # ONE call for the whole matrix
        status, newcrc = wg.gate_batch(d_ops, sparse=sparse)
        torch.cuda.synchronize()
        results[sparse] = (status.cpu().numpy(),
                           newcrc.cpu().numpy().view(np.uint32))
    return dict(slice_type=slice_type, images=images, data=data,
                placed=placed, d_images=d_images, d_data=d_data,
                ops_over=ops_over, results=results)


@pytest.mark.parametrize("sparse", (False, True))
def test_mixed_call_matches_restatement(world, sparse):
    status, newcrc = world["results"][sparse]
    seen = set()
    for i, p in enumerate(world["placed"]):
        c = p.case
        exp = c.expect(sparse)
        what = f"{p.fmt}: {c.name} (sparse={sparse})"
        assert (int(status[i]), int(newcrc[i])) == exp, \
            f"{what}: got status {status[i]} newcrc {int(newcrc[i]):#010x}, " \
            f"expected {exp[0]} {exp[1]:#010x}"
        if exp[0] == G.OK:
            assert int(newcrc[i]) == G.spliced_crc(c.offset, c.size, c.data,
                                                   c.block), what
        seen.add(exp[0])
    assert seen == {G.OK, G.BAD_DATA, G.BAD_BLOCK}


def test_apply_and_scrub(world):
    from lizardfs_amd import scrub
    slice_type = world["slice_type"]
    status, newcrc = world["results"][False]
    imgs = [t.clone() for t in world["d_images"]]
    d_data = world["d_data"]
    want = {}                  # image -> what the scrub must report
    for i, p in enumerate(world["placed"]):
        c = p.case
        if c.block is None:
            continue           # past the end of the image: nothing to touch
        if status[i] == G.OK:
            data_off, crc_off, bstride, cstride = \
                scrub.image_layout(p.fmt, slice_type)
            at = data_off + p.bindex * bstride + c.offset
            imgs[p.image][at:at + c.size] = \
                d_data[p.data_off:p.data_off + c.size]
            be = np.frombuffer(int(newcrc[i]).to_bytes(4, "big"), np.uint8)
            at = crc_off + p.bindex * cstride
            imgs[p.image][at:at + 4] = torch.from_numpy(be.copy()).cuda()
            want[p.image] = None
        elif status[i] == G.BAD_BLOCK:
            want[p.image] = p.bindex
        else:
            assert status[i] == G.BAD_DATA
            want[p.image] = None             # untouched and clean
    fmt_of = {p.image: p.fmt for p in world["placed"]}
    order = sorted(want)
    got = scrub.scrub_batch([(imgs[k], slice_type, fmt_of[k]) for k in order])
    for k, g in zip(order, got):
        assert g == want[k], \
            f"image {k} ({fmt_of[k]}): scrub says {g}, the gate {want[k]}"
    assert sum(w is not None for w in want.values()) >= 20
    assert sum(w is None for w in want.values()) >= 20


@pytest.mark.parametrize("sparse", (False, True))
def test_host_equals_device(world, sparse):
    from lizardfs_amd import writegate as wg
    h_ops = world["ops_over"](world["images"], world["data"])
    h_status, h_newcrc = wg.gate_host(h_ops, sparse=sparse)
    d_status, d_newcrc = world["results"][sparse]
    assert np.array_equal(h_status, d_status)
    assert np.array_equal(h_newcrc, d_newcrc)


def test_refusals_leave_outputs_untouched(world):
    import ctypes
    from lizardfs_amd import lib as L
    from lizardfs_amd import writegate as wg
    good = world["ops_over"](world["d_images"], world["d_data"])[:6].copy()
    n = good.size
    status = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    newcrc = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    one = int(world["d_data"].data_ptr())
    blk = int(world["d_images"][0].data_ptr())

    def broken(**fields):
        ops = good.copy()
        last = ops[-1]
        last["data"], last["block"], last["stored"] = one, 0, 0
        last["offset"], last["size"], last["reserved"] = 0, 1, 0
        for k, v in fields.items():
            last[k] = v
        return ops

    def call(ops, cnt, flags, st=status, nc=newcrc):
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        o = ctypes.c_void_p(ops.ctypes.data) if ops is not None else None
        r = L.lib().lizec_write_gate_batch(L.engine(0), o, cnt, flags, p(st),
                                           p(nc), None)
        torch.cuda.synchronize()
        return r

    refused = [
        ("ops NULL", None, n, 0),
        ("n == 0", good, 0, 0),
        ("n > 2^24", good, (1 << 24) + 1, 0),
        ("size > 65536", broken(size=65537), n, 0),
        ("offset >= 65536", broken(offset=65536, size=0), n, 0),
        ("offset + size > 65536", broken(offset=65535, size=2), n, 0),
        ("reserved != 0", broken(reserved=1), n, 0),
        ("size > 0 with data == 0", broken(data=0), n, 0),
        ("partial op, block without stored", broken(block=blk, stored=0), n,
         0),
        ("unknown flag bit", good, n, 2),
    ]
    for what, ops, cnt, flags in refused:
        assert call(ops, cnt, flags) == -2, what
    assert call(good, n, 0, st=None) == -2
    assert call(good, n, 0, nc=None) == -2
    assert (status.cpu().numpy() == -77).all()
    assert (newcrc.cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all()
    assert call(broken(), n, 0) == 0
    assert (status.cpu().numpy() != -77).all()
    with pytest.raises(L.LizecError):
        wg.gate_batch(broken(reserved=1))
