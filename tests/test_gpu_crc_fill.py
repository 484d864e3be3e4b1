"""lizec_crc_fill_batch_strided: the store counterpart of the scrub.  For
both on-disk layouts, three images of 1, 2 and 5 blocks get every block's
CRC written where scrub.build_chunk_image (with the oracle's crc32) puts it,
no other byte changes, and scrub_batch then reports the images clean."""
import ctypes

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
BLOCK_COUNTS = (1, 2, 5)

u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def reference_images(fmt, slice_type):
    from lizardfs_amd import scrub
    rng = np.random.default_rng(4242)
    imgs = []
    for i, n in enumerate(BLOCK_COUNTS):
        blocks = [rng.integers(0, 256, 65536, np.uint8) for _ in range(n)]
        img = scrub.build_chunk_image(77 + i, 3, slice_type, 1, blocks,
                                      crc32_fn=oracle.crc32, fmt=fmt)
        if fmt == "moosefs":
            # the unused tail of the CRC array must survive too
            img[scrub.SIGNATURE_BLOCK + 4 * n:
                scrub.header_size(slice_type)] = 0x5A
        imgs.append(img)
    return imgs


def fill(lib, eng, dev_imgs, layout, counts):
    doff, coff, bstride, cstride = layout
    n = len(dev_imgs)
    dptrs = np.array([t.data_ptr() for t in dev_imgs], np.uint64)
    doffs = np.full(n, doff, np.uint32)
    coffs = np.full(n, coff, np.uint32)
    cnt = np.array(counts, np.uint32)
    return lib.lizec_crc_fill_batch_strided(
        eng, dptrs.ctypes.data_as(u64p), doffs.ctypes.data_as(u32p),
        coffs.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p), n, bstride,
        cstride, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_crc_fill(fmt):
    from lizardfs_amd import lib as L
    from lizardfs_amd import scrub
    from lizardfs_amd import slice_traits as st
    lib, eng = L.lib(), L.engine(0)
    slice_type = st.ec_slice_type(8, 2)
    layout = scrub.image_layout(fmt, slice_type)
    doff, coff, bstride, cstride = layout
    ref = reference_images(fmt, slice_type)

    # the same images with 0xA5 in every CRC slot, packed back to back in
    # one buffer: INTERLEAVED images then start at 0, 4 and 12 mod 16
    blank = [r.copy() for r in ref]
    for img, n in zip(blank, BLOCK_COUNTS):
        for b in range(n):
            assert not np.all(img[coff + b * cstride:][:4] == 0xA5)
            img[coff + b * cstride:coff + b * cstride + 4] = 0xA5
    packed = torch.from_numpy(np.concatenate(blank)).cuda()
    starts = np.concatenate([[0], np.cumsum([r.size for r in ref])])
    dev = [packed[starts[i]:starts[i + 1]] for i in range(len(ref))]
    if fmt == "interleaved":
        assert [t.data_ptr() % 16 for t in dev] == [0, 4, 12]

    assert fill(lib, eng, dev, layout, BLOCK_COUNTS) == LIZEC_OK
    torch.cuda.synchronize()
    got = packed.cpu().numpy()
    for i, r in enumerate(ref):
        g = got[starts[i]:starts[i + 1]]
        for b in range(BLOCK_COUNTS[i]):
            stored = int.from_bytes(
                g[coff + b * cstride:coff + b * cstride + 4].tobytes(), "big")
            blk = r[doff + b * bstride:doff + b * bstride + 65536]
            assert stored == oracle.crc32(blk.tobytes()), (fmt, i, b)
        assert np.array_equal(g, r), f"{fmt} image {i}: other bytes changed"

    assert scrub.scrub_batch([(t, slice_type, fmt) for t in dev]) == \
        [None] * len(dev)


def test_crc_fill_refusals():
    """Host-side LIZEC_EINVAL, image untouched: block data at 2 mod 4, a
    block stride below 65536 or not a multiple of 4, no blocks, address 0."""
    from lizardfs_amd import lib as L
    lib, eng = L.lib(), L.engine(0)
    buf = torch.full((4 * 65540 + 16,), 0xA5, dtype=torch.uint8,
                     device="cuda")
    ok = (4, 0, 65540, 65540)
    cases = [
        ([buf[2:]], ok, [2]),
        ([buf], (4, 0, 65532, 65540), [2]),
        ([buf], (4, 0, 65538, 65540), [2]),
        ([buf], ok, [0]),
    ]
    for imgs, layout, counts in cases:
        assert fill(lib, eng, imgs, layout, counts) == LIZEC_EINVAL
    zero = np.zeros(1, np.uint64)
    one = np.array([1], np.uint32)
    assert lib.lizec_crc_fill_batch_strided(
        eng, zero.ctypes.data_as(u64p), one.ctypes.data_as(u32p),
        one.ctypes.data_as(u32p), one.ctypes.data_as(u32p), 1, 65540, 65540,
        None) == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
