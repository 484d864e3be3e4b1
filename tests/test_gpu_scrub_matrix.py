"""lizec_scrub_batch_strided through the C ABI: scrub_chunks_kernel<false> at
16-byte alignment (MooseFS images) and at dword alignment (INTERLEAVED
images packed back to back, starting at 0, 4 and 12 mod 16), and the host
checks it shares with lizec_crc_fill_batch_strided.

Images come from scrub.build_chunk_image with the oracle's crc32; damage is
one flipped bit at a chosen byte.  The expected status is the first damaged
block, INT32_MAX for a clean image or one of no blocks.

Not covered: the kernel's grid-stride loop, which starts above 524,288
blocks of 64 KiB (131,072 workgroups of four waves), 32 GiB of images.
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
CLEAN = 0x7FFFFFFF
UNTOUCHED = 0x5A5A5A5A
FORMATS = ("moosefs", "interleaved")

u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def scrub_call(dptrs, doffs, coffs, counts, n, bstride, cstride, status):
    from lizardfs_amd import lib as L
    return L.lib().lizec_scrub_batch_strided(
        L.engine(0), p(dptrs, u64p), p(doffs, u32p), p(coffs, u32p),
        p(counts, u32p), n, bstride, cstride,
        ctypes.c_void_p(status.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))


def layout_of(fmt):
    from lizardfs_amd import scrub
    from lizardfs_amd import slice_traits as st
    return scrub.image_layout(fmt, st.ec_slice_type(8, 2))


def make_image(fmt, nblocks, rng, damage=()):
    """damage: (kind, block, byte) with kind "data" or "crc"."""
    from lizardfs_amd import scrub
    from lizardfs_amd import slice_traits as st
    doff, coff, bstride, cstride = layout_of(fmt)
    blocks = [rng.integers(0, 256, BLOCK, np.uint8) for _ in range(nblocks)]
    img = scrub.build_chunk_image(5, 1, st.ec_slice_type(8, 2), 0, blocks,
                                  crc32_fn=oracle.crc32, fmt=fmt)
    for kind, b, byte in damage:
        at = (doff + b * bstride if kind == "data" else coff + b * cstride)
        img[at + byte] ^= 0x04
    return img


def run_packed(fmt, images, counts=None, empty_after=None):
    """Scrub `images` packed back to back in one device buffer; with
    empty_after = i, an image of no blocks (at the next image's address) is
    passed after image i.  Returns the status list."""
    doff, coff, bstride, cstride = layout_of(fmt)
    packed = torch.from_numpy(np.concatenate(images)).cuda()
    starts = np.concatenate([[0], np.cumsum([i.size for i in images])])
    addrs = [packed.data_ptr() + int(s) for s in starts[:-1]]
    cnts = [(i.size - (doff if fmt == "moosefs" else 0)) //
            (BLOCK if fmt == "moosefs" else bstride) for i in images] \
        if counts is None else list(counts)
    if empty_after is not None:
        addrs.insert(empty_after + 1, addrs[empty_after + 1])
        cnts.insert(empty_after + 1, 0)
    n = len(addrs)
    status = torch.full((n + 2,), UNTOUCHED, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = scrub_call(np.array(addrs, np.uint64), np.full(n, doff, np.uint32),
                    np.full(n, coff, np.uint32), np.array(cnts, np.uint32),
                    n, bstride, cstride, status[1:])
    assert rc == LIZEC_OK
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st[0] == UNTOUCHED and st[-1] == UNTOUCHED
    assert np.array_equal(packed.cpu().numpy(), np.concatenate(images)), \
        "the scrub wrote to an image"
    return [a % 16 for a in addrs], st[1:-1].tolist()


@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_images_and_an_empty_one(fmt):
    """Images of 1, 2, 5, 6 and 3 blocks back to back (INTERLEAVED ones
    start at 0, 4, 12, 0 and 8 mod 16), an image of no blocks between the
    second and the third.  Damage: none; block 1 in its first byte only;
    block 4 in its last byte only; none; the stored CRC of block 2."""
    rng = np.random.default_rng(2024)
    images = [
        make_image(fmt, 1, rng),
        make_image(fmt, 2, rng, [("data", 1, 0)]),
        make_image(fmt, 5, rng, [("data", 4, BLOCK - 1)]),
        make_image(fmt, 6, rng),
        make_image(fmt, 3, rng, [("crc", 2, 3)]),
    ]
    phases, status = run_packed(fmt, images, empty_after=1)
    if fmt == "interleaved":
        assert phases == [0, 4, 12, 12, 0, 8]
    else:
        assert phases == [0] * 6
    assert status == [CLEAN, 1, CLEAN, 4, CLEAN, 2]


@pytest.mark.parametrize("fmt", FORMATS)
def test_first_and_last_byte_of_every_block(fmt):
    """One image per damaged byte: byte 0 and byte 65535 of blocks 0 and 2
    of a three-block image; each must be seen at its block."""
    rng = np.random.default_rng(2025)
    cases = [(0, 0), (0, BLOCK - 1), (2, 0), (2, BLOCK - 1)]
    images = [make_image(fmt, 3, rng, [("data", b, byte)])
              for b, byte in cases]
    _, status = run_packed(fmt, images)
    assert status == [b for b, _ in cases]


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_damaged_blocks_in_different_workgroups(fmt):
    """Blocks 0 and 5 of a six-block image: a workgroup holds four waves, so
    block 5 is checked by the second one; the first damaged block wins."""
    rng = np.random.default_rng(2026)
    img = make_image(fmt, 6, rng, [("data", 0, 1000), ("data", 5, 77)])
    only5 = make_image(fmt, 6, rng, [("data", 5, 77)])
    assert run_packed(fmt, [img])[1] == [0]
    assert run_packed(fmt, [only5])[1] == [5]


REFUSALS = ("NULL chunk_dptrs", "NULL data_offs", "NULL crc_offs",
            "NULL block_counts", "block data at 2 mod 4",
            "block stride 65532", "block stride 65538", "address 0",
            "address 0 of an image without blocks", "no blocks at all",
            "max_blocks * block_stride = 2^32 + 262144",
            "max_blocks * crc_stride = 2^32")


@pytest.mark.parametrize("what", REFUSALS)
def test_scrub_refusals(what):
    """Host-side LIZEC_EINVAL with nothing enqueued: the status array keeps
    its 0x5A5A5A5A.  No refused call reaches the kernel, so the counts and
    strides of the overflow cases are never used as addresses."""
    buf = torch.zeros(4 * 65540 + 16, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), UNTOUCHED, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a = buf.data_ptr()
    dptrs = np.array([a, a], np.uint64)
    doffs = np.array([4, 4], np.uint32)
    coffs = np.array([0, 0], np.uint32)
    counts = np.array([2, 1], np.uint32)
    bstride = cstride = 65540
    assert scrub_call(dptrs, doffs, coffs, counts, 2, bstride, cstride,
                      status) == LIZEC_OK      # the unchanged call is fine
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist()[:2] != [UNTOUCHED, UNTOUCHED]
    status.fill_(UNTOUCHED)
    torch.cuda.synchronize()
    if what == "NULL chunk_dptrs":
        dptrs = None
    elif what == "NULL data_offs":
        doffs = None
    elif what == "NULL crc_offs":
        coffs = None
    elif what == "NULL block_counts":
        counts = None
    elif what == "block data at 2 mod 4":
        dptrs[1] = a + 2
    elif what == "block stride 65532":
        bstride = 65532
    elif what == "block stride 65538":
        bstride = 65538
    elif what == "address 0":
        dptrs[1] = 0
    elif what == "address 0 of an image without blocks":
        dptrs[1], counts[1] = 0, 0
    elif what == "no blocks at all":
        counts[:] = 0
    elif what == "max_blocks * block_stride = 2^32 + 262144":
        counts[1] = 65536
    elif what == "max_blocks * crc_stride = 2^32":
        bstride, cstride = 65536, 0x80000000
        doffs[:] = 8
    else:
        raise AssertionError(what)
    assert scrub_call(dptrs, doffs, coffs, counts, 2, bstride, cstride,
                      status) == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [UNTOUCHED] * 4


def test_scrub_batch_keeps_empty_images_out_of_the_call():
    """scrub.scrub_batch: an empty INTERLEAVED image (a tensor of no bytes
    has address 0, which the call refuses) is clean and does not disturb
    the images around it."""
    from lizardfs_amd import scrub
    from lizardfs_amd import slice_traits as st
    t = st.ec_slice_type(8, 2)
    rng = np.random.default_rng(2027)
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    bad = torch.from_numpy(
        make_image("interleaved", 2, rng, [("data", 1, 9)])).cuda()
    good = torch.from_numpy(make_image("interleaved", 1, rng)).cuda()
    assert scrub.scrub_batch([(bad, t, "interleaved"),
                              (empty, t, "interleaved"),
                              (good, t, "interleaved")]) == [1, None, None]
    assert scrub.scrub_batch([(empty, t, "interleaved")]) == [None]
