"""Chunks of different lengths in one batch, through the Python layer:
ReedSolomon.recover_batch_ragged and rebuild_part_images(chunk_blocks=...).

ec(3,2), six chunks of 1, 2, 3, 4, 5 and 7 blocks.  Block b of a chunk is
block b // 3 of data part b % 3 (slice_traits.h:311-316), so the parts have
0..3 blocks and the last stripe row of most chunks is short.  The expected
bytes come from the oracle over the zero-padded stripes; fragment rows
beyond a chunk's own length hold 0xFF, so reading them changes the result.
"""
import struct

import numpy as np
import pytest

import oracle

from lizardfs_amd import slice_traits as st

pytestmark = pytest.mark.gpu

K, M = 3, 2
CHUNK_BLOCKS = (1, 2, 3, 4, 5, 7)
S = len(CHUNK_BLOCKS)
BLOCK = st.BLOCK_SIZE
LMAX = 3 * BLOCK
T = st.ec_slice_type(K, M)
FILL = 0xA5
VERSION = 7
CHUNK_IDS = [0x1000 + s for s in range(S)]


@pytest.fixture(scope="module")
def chunks():
    """(parts [S, K+M, LMAX] zero-padded, from the oracle; part_blocks
    [S, K+M]), read-only."""
    rng = np.random.default_rng(311)
    pb = np.array([[st.number_of_blocks(T, p, n) for p in range(K + M)]
                   for n in CHUNK_BLOCKS], np.int64)
    assert pb.min() == 0 and pb.max() == 3
    parts = np.zeros((S, K + M, LMAX), np.uint8)
    for s, n in enumerate(CHUNK_BLOCKS):
        chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
        for b in range(n):
            parts[s, b % K, (b // K) * BLOCK:(b // K + 1) * BLOCK] = chunk[b]
        par = oracle.rs_encode(K, M, [np.ascontiguousarray(parts[s, p])
                                      for p in range(K)], LMAX)
        for l in range(M):
            parts[s, K + l] = par[l]
            # parity is as long as part 0; beyond that everything is zero
            assert not parts[s, K + l, pb[s, K + l] * BLOCK:].any()
    parts.setflags(write=False)
    pb.setflags(write=False)
    return parts, pb


def fragment(parts, pb, p):
    """Part p of every chunk as a [S, LMAX] CUDA tensor, 0xFF from the end
    of each chunk's own part on."""
    import torch
    a = np.array(parts[:, p])
    for s in range(S):
        a[s, int(pb[s, p]) * BLOCK:] = 0xFF
    return torch.from_numpy(a).cuda()


def check_out(out, slots, parts, pb, what):
    """out[s, j]: the blocks of part slots[s, j] below its count equal the
    oracle's, every other byte is still FILL."""
    import torch
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s in range(S):
        for j in range(slots.shape[1]):
            p = int(slots[s, j])
            n = int(pb[s, p]) * BLOCK if p >= 0 else 0
            if p >= 0:
                assert np.array_equal(got[s, j, :n], parts[s, p, :n]), \
                    (what, s, p)
            assert (got[s, j, n:] == FILL).all(), (what, s, p, "overrun")


def test_encode(chunks):
    import torch
    from lizardfs_amd.ec import ReedSolomon
    parts, pb = chunks
    rs = ReedSolomon(K, M)
    frags = [fragment(parts, pb, p) for p in range(K)] + [None] * M
    keep = [f.clone() for f in frags[:K]]
    out = torch.full((S, M, LMAX), FILL, dtype=torch.uint8, device="cuda")
    got, slots = rs.recover_batch_ragged(frags, (3, 4), out=out,
                                         part_blocks=pb)
    assert got is out
    assert slots.tolist() == [[3, 4]] * S
    check_out(out, slots, parts, pb, "encode")
    for f, k in zip(frags[:K], keep):
        assert torch.equal(f, k), "the sources were modified"
    # allocated output: rows sized for the longest wanted part
    got, slots = rs.recover_batch_ragged(frags, (3, 4), want=(4,),
                                         part_blocks=pb)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (S, 1, LMAX) and slots.tolist() == [[4]] * S
    for s in range(S):
        n = int(pb[s, 4]) * BLOCK
        assert np.array_equal(got[s, 0, :n].cpu().numpy(), parts[s, 4, :n])


def test_recover_one_pattern(chunks):
    import torch
    from lizardfs_amd.ec import ReedSolomon
    parts, pb = chunks
    rs = ReedSolomon(K, M)
    erased = (0, 3)
    frags = [None if p in erased else fragment(parts, pb, p)
             for p in range(K + M)]
    out = torch.full((S, 2, LMAX), FILL, dtype=torch.uint8, device="cuda")
    _, slots = rs.recover_batch_ragged(frags, erased, out=out,
                                       part_blocks=pb)
    assert slots.tolist() == [[0, 3]] * S
    check_out(out, slots, parts, pb, "erased (0, 3)")


def test_recover_pattern_per_stripe(chunks):
    import torch
    from lizardfs_amd.ec import ReedSolomon
    parts, pb = chunks
    rs = ReedSolomon(K, M)
    erased = [(0, 1), (1, 4), (2, 3), (0, 4), (3, 4), (1, 2)]
    want = [(0, 1), (4,), (2, 3), (0,), (3, 4), (2,)]
    frags = [fragment(parts, pb, p) for p in range(K + M)]
    # rows of a part erased in a stripe are ignored
    for s, e in enumerate(erased):
        for p in e:
            frags[p][s] = 0xEE
    out = torch.full((S, 2, LMAX), FILL, dtype=torch.uint8, device="cuda")
    _, slots = rs.recover_batch_ragged(frags, erased, want, out=out,
                                       part_blocks=pb)
    assert slots.tolist() == [[0, 1], [4, -1], [2, 3], [0, -1], [3, 4],
                              [2, -1]]
    check_out(out, slots, parts, pb, "per-stripe patterns")
    # a strided destination: INTERLEAVED block slots inside a wider row
    span = 4 + 3 * 65540
    out = torch.full((S, 2, span), FILL, dtype=torch.uint8, device="cuda")
    rs.recover_batch_ragged(frags, erased, want, out=out[:, :, 4:],
                            part_blocks=pb, dst_stride=65540)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exp = np.full((S, 2, span), FILL, np.uint8)
    for s in range(S):
        for j in range(2):
            p = slots[s, j]
            for b in range(int(pb[s, p]) if p >= 0 else 0):
                exp[s, j, 4 + b * 65540:4 + b * 65540 + BLOCK] = \
                    parts[s, p, b * BLOCK:(b + 1) * BLOCK]
    assert np.array_equal(got, exp)


def ref_image(parts, pb, s, p, fmt):
    """The image of part p of chunk s, CRCs by the oracle.  MooseFS through
    scrub.build_chunk_image; INTERLEAVED assembled here: every block behind
    its own big-endian CRC, nothing else."""
    from lizardfs_amd import scrub
    blocks = [parts[s, p, b * BLOCK:(b + 1) * BLOCK]
              for b in range(int(pb[s, p]))]
    if fmt == "moosefs":
        return scrub.build_chunk_image(CHUNK_IDS[s], VERSION, T, p, blocks,
                                       crc32_fn=oracle.crc32)
    out = bytearray()
    for blk in blocks:
        out += struct.pack(">I", oracle.crc32(blk.tobytes())) + blk.tobytes()
    return np.frombuffer(bytes(out), np.uint8)


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_rebuild_part_images(chunks, fmt):
    from lizardfs_amd import scrub
    from lizardfs_amd.replicate import rebuild_part_images
    parts, pb = chunks
    erased = (1, 3)
    frags = [None if p in erased else fragment(parts, pb, p)
             for p in range(K + M)]
    images = rebuild_part_images(K, M, frags, erased, set(erased), CHUNK_IDS,
                                 VERSION, fmt=fmt, chunk_blocks=CHUNK_BLOCKS)
    assert sorted(images) == sorted((s, p) for s in range(S) for p in erased)
    hdr = scrub.header_size(T)
    sizes = set()
    for (s, p), img in images.items():
        nb = int(pb[s, p])
        size = hdr + nb * BLOCK if fmt == "moosefs" else nb * scrub.HDD_BLOCK
        assert img.numel() == size, (s, p)
        sizes.add(size)
        assert np.array_equal(img.cpu().numpy(),
                              ref_image(parts, pb, s, p, fmt)), (s, p)
    assert len(sizes) == 4      # parts of 0, 1, 2 and 3 blocks
    keys = sorted(images)
    batch = [(images[key], T, fmt) for key in keys]
    assert scrub.scrub_batch(batch) == [None] * len(batch)


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_rebuild_pattern_per_chunk(chunks, fmt):
    from lizardfs_amd.replicate import rebuild_part_images
    parts, pb = chunks
    erased = [(0, 1), (1, 4), (2, 3), (0, 4), (3, 4), (1, 2)]
    want = [(0, 1), (4,), (2, 3), (0,), (3, 4), (2,)]
    frags = [fragment(parts, pb, p) for p in range(K + M)]
    images = rebuild_part_images(K, M, frags, erased, want, CHUNK_IDS,
                                 VERSION, fmt=fmt, chunk_blocks=CHUNK_BLOCKS)
    assert sorted(images) == sorted((s, p) for s in range(S)
                                    for p in want[s])
    for (s, p), img in images.items():
        assert np.array_equal(img.cpu().numpy(),
                              ref_image(parts, pb, s, p, fmt)), (s, p)


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_without_chunk_blocks_nothing_changes(chunks, fmt):
    """Full-length parts, no chunk_blocks: the images of the uniform path,
    equal to the reference images and to a ragged rebuild of chunks that
    all have 9 blocks."""
    import torch
    from lizardfs_amd import scrub
    from lizardfs_amd.replicate import rebuild_part_images
    parts, _ = chunks
    rng = np.random.default_rng(312)
    full = np.array(parts)
    full[:, :K] = rng.integers(0, 256, (S, K, LMAX), np.uint8)
    for s in range(S):
        par = oracle.rs_encode(K, M, [np.ascontiguousarray(full[s, p])
                                      for p in range(K)], LMAX)
        full[s, K:] = np.stack(par)
    pb9 = np.full((S, K + M), 3, np.int64)
    erased = (1, 3)
    frags = [None if p in erased else
             torch.from_numpy(np.ascontiguousarray(full[:, p])).cuda()
             for p in range(K + M)]
    plain = rebuild_part_images(K, M, frags, erased, set(erased), CHUNK_IDS,
                                VERSION, fmt=fmt)
    ragged = rebuild_part_images(K, M, frags, erased, set(erased), CHUNK_IDS,
                                 VERSION, fmt=fmt, chunk_blocks=[9] * S)
    assert sorted(plain) == sorted(ragged)
    hdr = scrub.header_size(T)
    for key, img in plain.items():
        s, p = key
        assert img.numel() == (hdr + LMAX if fmt == "moosefs"
                               else 3 * scrub.HDD_BLOCK)
        assert np.array_equal(img.cpu().numpy(),
                              ref_image(full, pb9, s, p, fmt)), key
        assert torch.equal(img, ragged[key]), key


def test_argument_errors(chunks, monkeypatch):
    """ValueError, and before any call into the library."""
    import torch
    from lizardfs_amd.ec import ReedSolomon
    from lizardfs_amd.replicate import rebuild_part_images
    parts, pb = chunks
    rs = ReedSolomon(K, M)

    def no_call(*a, **kw):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ReedSolomon, "_ragged_call", no_call)
    erased = (0, 3)
    frags = [None if p in erased else fragment(parts, pb, p)
             for p in range(K + M)]
    ok = dict(part_blocks=pb)

    def refused(*a, **kw):
        with pytest.raises(ValueError):
            rs.recover_batch_ragged(*a, **kw)

    refused(frags[:-1], erased, **ok)                   # k+m slots
    refused(frags, erased, part_blocks=pb[:, :-1])      # [S, k+m]
    refused(frags, erased, part_blocks=pb[0])
    refused(frags, erased, part_blocks=pb.astype(np.float64))
    big = np.array(pb)
    big[0, 1] = 32769
    refused(frags, erased, part_blocks=big)
    big[0, 1] = -1
    refused(frags, erased, part_blocks=big)
    refused(frags, (0,), **ok)                          # exactly m erased
    refused(frags, erased, want=(1,), **ok)             # want within erased
    refused(frags, [erased] * (S - 1), **ok)            # one set per stripe
    refused(frags, erased, want=[(0,)] * (S + 1), **ok)
    # None where the part survives in some stripe
    refused(frags, [erased] * (S - 1) + [(1, 3)], **ok)
    refused([None] * (K + M), erased, **ok)
    # rows that cannot hold the largest count of the part
    short = list(frags)
    assert pb[:, 1].max() == 2
    short[1] = frags[1][:, :2 * BLOCK - 16]
    refused(short, erased, **ok)
    odd = list(frags)                                   # rows at 2 mod 4
    odd[2] = torch.zeros((S, LMAX + 16), dtype=torch.uint8,
                         device="cuda")[:, 2:]
    refused(odd, erased, **ok)
    refused(frags, erased, src_stride=65538, **ok)
    refused(frags, erased, src_stride=65532, **ok)
    refused(frags, erased, dst_stride=65538, **ok)
    refused(frags, erased, dst_stride=65540, **ok)      # needs out
    out = torch.zeros((S, 2, LMAX), dtype=torch.uint8, device="cuda")
    refused(frags, erased, out=out[:, :1], **ok)        # [S, oc, span]
    refused(frags, erased, out=out[:, :, :LMAX - 16], **ok)
    refused(frags, erased, out=out[:, :, 2:], **ok)
    refused(frags, erased, out=out, dst_stride=65540, **ok)   # too short
    # nothing to rebuild: part 2 of the one-block chunk is empty
    one = [None if f is None else f[:1] for f in frags]
    one[0] = fragment(parts, pb, 0)[:1]
    one[2] = None
    refused(one, (2, 3), want=(2,), part_blocks=pb[:1])

    for bad in ([0] + list(CHUNK_BLOCKS[1:]), [1025] + list(CHUNK_BLOCKS[1:]),
                CHUNK_BLOCKS[:-1], [CHUNK_BLOCKS]):
        with pytest.raises(ValueError):
            rebuild_part_images(K, M, frags, erased, set(erased), CHUNK_IDS,
                                VERSION, chunk_blocks=bad)
    with pytest.raises(ValueError):
        rebuild_part_images(K, M, frags, erased, set(erased), CHUNK_IDS[:-1],
                            VERSION, chunk_blocks=CHUNK_BLOCKS)
