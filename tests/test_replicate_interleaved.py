"""INTERLEAVED-format rebuild: ec(8,2), 5 chunks, 3 blocks per part,
sub_batch 2 (two full pipeline stages and a short one).  The streamed and
the device-resident images are byte-identical to
scrub.build_chunk_image(fmt="interleaved") of the original data (CRCs by the
oracle), pass the scrub, and a flipped byte is reported at its block; and
survivors are read straight out of INTERLEAVED images."""
import numpy as np
import pytest

import oracle

from lizardfs_amd import slice_traits as st

pytestmark = pytest.mark.gpu

K, M, S, NBLOCKS = 8, 2, 5, 3
PLEN = NBLOCKS * st.BLOCK_SIZE
ERASED = (1, 9)        # a data part and a parity part


@pytest.fixture(scope="module")
def stripes():
    """(data [S, K, PLEN], parity [S, M, PLEN]) from the oracle, and the
    reference images of every part: ref[p][s]."""
    from lizardfs_amd import scrub
    rng = np.random.default_rng(1905)
    data = rng.integers(0, 256, (S, K, PLEN), np.uint8)
    parity = np.stack([np.stack(oracle.rs_encode(K, M, list(data[s]), PLEN))
                       for s in range(S)])
    parts = np.concatenate([data, parity], axis=1)      # [S, K+M, PLEN]
    t = st.ec_slice_type(K, M)
    ref = {p: [scrub.build_chunk_image(
        0, 0, t, p, [parts[s, p, b * st.BLOCK_SIZE:(b + 1) * st.BLOCK_SIZE]
                     for b in range(NBLOCKS)],
        crc32_fn=oracle.crc32, fmt="interleaved") for s in range(S)]
        for p in range(K + M)}
    for v in (data, parity, parts):
        v.setflags(write=False)
    return parts, ref


def test_replicate_stream_interleaved(stripes):
    import torch
    from lizardfs_amd import scrub
    from lizardfs_amd.replicate import replicate_stream
    parts, ref = stripes
    host_parts = [None if i in ERASED else np.ascontiguousarray(parts[:, i])
                  for i in range(K + M)]
    out = replicate_stream(K, M, host_parts, ERASED, ERASED,
                           list(range(S)), version=1, sub_batch=2,
                           fmt="interleaved")
    assert sorted(out) == sorted(ERASED)
    for p in ERASED:
        assert out[p].shape == (S, NBLOCKS * scrub.HDD_BLOCK)
        for s in range(S):
            assert np.array_equal(out[p][s], ref[p][s]), (p, s)
    t = st.ec_slice_type(K, M)
    batch = [(torch.from_numpy(np.ascontiguousarray(out[p][s])).cuda(), t,
              "interleaved") for p in ERASED for s in range(S)]
    assert scrub.scrub_batch(batch) == [None] * len(batch)


def test_rebuild_part_images_interleaved(stripes):
    import torch
    from lizardfs_amd import scrub
    from lizardfs_amd.replicate import rebuild_part_images
    parts, ref = stripes
    frags = [None if i in ERASED else
             torch.from_numpy(np.ascontiguousarray(parts[:, i])).cuda()
             for i in range(K + M)]
    images = rebuild_part_images(K, M, frags, ERASED, set(ERASED),
                                 list(range(S)), version=1,
                                 fmt="interleaved")
    assert sorted(images) == sorted((s, p) for p in ERASED for s in range(S))
    for (s, p), img in images.items():
        assert np.array_equal(img.cpu().numpy(), ref[p][s]), (s, p)

    t = st.ec_slice_type(K, M)
    keys = sorted(images)
    batch = [(images[key].contiguous(), t, "interleaved") for key in keys]
    assert scrub.scrub_batch(batch) == [None] * len(batch)
    # one flipped data byte, in block 2 of one image, is found there
    victim = batch[3][0]
    victim[2 * scrub.HDD_BLOCK + 4 + 100] ^= 0x01
    want = [None] * len(batch)
    want[3] = 2
    assert scrub.scrub_batch(batch) == want


def test_recover_batch_blocks_reads_interleaved_images(stripes):
    """Survivors read from INTERLEAVED images (img[:, 4:], stride 65540)
    into plain aligned tensors: the same bytes as recover_batch on the
    de-interleaved data, and as the original parts."""
    import torch
    from lizardfs_amd import scrub
    from lizardfs_amd.ec import ReedSolomon
    parts, ref = stripes
    rs = ReedSolomon(K, M)
    imgs = {p: torch.from_numpy(np.stack(ref[p])).cuda()
            for p in range(K + M) if p not in ERASED}
    frags_il = [None if p in ERASED else imgs[p][:, 4:]
                for p in range(K + M)]
    got = rs.recover_batch_blocks(frags_il, ERASED, nblocks=NBLOCKS,
                                  src_stride=scrub.HDD_BLOCK)
    frags = [None if p in ERASED else
             torch.from_numpy(np.ascontiguousarray(parts[:, p])).cuda()
             for p in range(K + M)]
    exp = rs.recover_batch(frags, ERASED)
    rs.sync()
    torch.cuda.synchronize()
    assert sorted(got) == sorted(exp) == sorted(ERASED)
    for p in ERASED:
        assert got[p].shape == (S, PLEN) and got[p].data_ptr() % 16 == 0
        assert torch.equal(got[p], exp[p]), p
        assert np.array_equal(got[p].cpu().numpy(), parts[:, p]), p
    for p, img in imgs.items():
        assert np.array_equal(img.cpu().numpy(), np.stack(ref[p])), \
            "the source images were modified"


def test_recover_batch_blocks_argument_checks(stripes):
    import torch
    from lizardfs_amd import scrub
    from lizardfs_amd.ec import ReedSolomon
    parts, ref = stripes
    rs = ReedSolomon(K, M)
    img = torch.zeros((S, NBLOCKS * scrub.HDD_BLOCK), dtype=torch.uint8,
                      device="cuda")
    frags = [None if p in ERASED else img[:, 4:] for p in range(K + M)]
    kw = dict(nblocks=NBLOCKS, src_stride=scrub.HDD_BLOCK)
    with pytest.raises(ValueError):     # out needed for a strided output
        rs.recover_batch_blocks(frags, ERASED, dst_stride=scrub.HDD_BLOCK,
                                **kw)
    with pytest.raises(ValueError):     # rows too short for the blocks
        rs.recover_batch_blocks(frags, ERASED, nblocks=NBLOCKS + 1,
                                src_stride=scrub.HDD_BLOCK)
    with pytest.raises(ValueError):     # rows at 2 mod 4
        rs.recover_batch_blocks(
            [None if f is None else img[:, 2:] for f in frags], ERASED, **kw)
    with pytest.raises(ValueError):     # stride not a multiple of 4
        rs.recover_batch_blocks(frags, ERASED, nblocks=NBLOCKS,
                                src_stride=65538)
    with pytest.raises(ValueError):     # recover_batch's own checks
        rs.recover_batch_blocks(frags, (1,), **kw)
    with pytest.raises(ValueError):
        rs.recover_batch_blocks(frags, ERASED, want=(2,), **kw)
