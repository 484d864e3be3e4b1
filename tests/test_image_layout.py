"""scrub.image_layout, and the refusal of an unknown chunk format before
anything touches a GPU (these run without one)."""
import numpy as np
import pytest

from lizardfs_amd import scrub
from lizardfs_amd import slice_traits as st


@pytest.mark.parametrize("k,m", ((2, 1), (8, 2), (16, 4), (32, 32)))
def test_image_layout_values(k, m):
    t = st.ec_slice_type(k, m)
    assert scrub.image_layout("moosefs", t) == (
        scrub.header_size(t), scrub.SIGNATURE_BLOCK, st.BLOCK_SIZE, 4)
    assert scrub.image_layout("interleaved", t) == (
        4, 0, scrub.HDD_BLOCK, scrub.HDD_BLOCK)
    assert scrub.HDD_BLOCK == 65540


def test_image_layout_describes_build_chunk_image():
    """Block b's data and CRC are where image_layout says, in both formats."""
    from lizardfs_amd import crc as lcrc
    t = st.ec_slice_type(8, 2)
    rng = np.random.default_rng(5)
    blocks = [rng.integers(0, 256, st.BLOCK_SIZE, np.uint8) for _ in range(3)]
    for fmt in scrub.FORMATS:
        img = scrub.build_chunk_image(9, 1, t, 0, blocks, fmt=fmt)
        doff, coff, bstride, cstride = scrub.image_layout(fmt, t)
        assert img.size == doff + 2 * bstride + st.BLOCK_SIZE
        for b, blk in enumerate(blocks):
            at = doff + b * bstride
            assert np.array_equal(img[at:at + st.BLOCK_SIZE], blk)
            stored = int.from_bytes(
                img[coff + b * cstride:coff + b * cstride + 4].tobytes(),
                "big")
            assert stored == lcrc.crc32(blk.tobytes())


def test_unknown_format_is_refused_before_any_gpu_use():
    from lizardfs_amd.replicate import rebuild_part_images, replicate_stream
    t = st.ec_slice_type(8, 2)
    with pytest.raises(ValueError):
        scrub.image_layout("moosefs2", t)
    with pytest.raises(ValueError):
        scrub.image_layout(None, t)
    parts = [np.zeros((1, st.BLOCK_SIZE), np.uint8) for _ in range(10)]
    with pytest.raises(ValueError, match="format"):
        rebuild_part_images(8, 2, parts, (8, 9), (8, 9), [1], 1,
                            fmt="lizardfs")
    with pytest.raises(ValueError, match="format"):
        replicate_stream(8, 2, parts, (8, 9), (8, 9), [1], 1, fmt="lizardfs")
