"""The ragged streaming rebuild on the CPU (no GPU):
replicate_stream_ragged_host over lizec_replicate_ragged_host, against images
built from the oracle's parts (replicate_ragged_cases.py)."""
import ctypes

import numpy as np
import pytest

import replicate_ragged_cases as C

from lizardfs_amd import lib as L
from lizardfs_amd import replicate
from lizardfs_amd import scrub


@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("case", sorted(C.IMAGE_CASES))
def test_images(case, fmt):
    popf, erased, want = C.IMAGE_CASES[case]
    pop = popf()
    res, bufs = C.run(replicate.replicate_stream_ragged_host, pop, erased,
                      want, fmt)
    assert res.corrupt == {}
    C.check_images(res, bufs, pop, erased, want, fmt)


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_header_only_and_empty_sizes(fmt):
    """Parts 1 and 2 of the 1-block chunk have no block: a header and nothing
    else in MooseFS format, nothing at all in INTERLEAVED format."""
    pop = C.base()
    res, _ = C.run(replicate.replicate_stream_ragged_host, pop, (1, 2), None,
                   fmt)
    hdr = scrub.header_size(pop.T) if fmt == "moosefs" else 0
    assert res.images[(0, 1)].size == hdr and res.images[(0, 2)].size == hdr
    if hdr:
        assert not res.images[(0, 1)][22:].any()


def test_allocated_images():
    """Without `out` the images are views of one arena, each of its own
    size."""
    pop = C.base()
    res = replicate.replicate_stream_ragged_host(
        pop.k, pop.m, pop.sources(), pop.chunk_blocks, C.PER_CHUNK, None,
        pop.chunk_ids, C.VERSION)
    C.check_images(res, {}, pop, C.PER_CHUNK, None, "moosefs")
    assert len({id(a.base) for a in res.images.values()}) == 1


@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("what", C.VERIFY_CASES)
def test_verification(what, fmt):
    pop = C.base()
    parts, crcs, bad = C.verify_inputs(pop, what)
    res, bufs = C.run(replicate.replicate_stream_ragged_host, pop, C.V_ERASED,
                      None, fmt, crcs=crcs, parts=parts)
    assert res.corrupt == bad
    skip = set(bad)
    if what == "unverified_slot":
        # nobody looked: the chunk rebuilt from the corrupt source is wrong
        skip = {C.V_CHUNK}
        res.images.pop((C.V_CHUNK, 0))
        res.images.pop((C.V_CHUNK, 1))
    C.check_images(res, bufs, pop, C.V_ERASED, None, fmt, skip=skip)


def test_crc_array_as_big_endian_words():
    """crcs as [S, nmax] '>u4' arrays give the same as [S, nmax, 4] bytes."""
    pop = C.base()
    parts, crcs, bad = C.verify_inputs(pop, "data_byte")
    crcs = [np.ascontiguousarray(c).view(">u4").reshape(pop.S, pop.nmax)
            for c in crcs]
    res, _ = C.run(replicate.replicate_stream_ragged_host, pop, C.V_ERASED,
                   None, "moosefs", crcs=crcs, parts=parts)
    assert res.corrupt == bad


def test_c_entry_bad_out_bits():
    """The C entry itself: the mask of (chunk 3, slot 1) is 1 << 1 and every
    other mask 0; the images are emitted either way."""
    pop = C.base()
    parts, crcs, _ = C.verify_inputs(pop, "data_byte")
    p = replicate._stream_ragged_prepare(
        pop.k, pop.m, parts, pop.chunk_blocks, C.V_ERASED, None,
        pop.chunk_ids, C.VERSION, crcs, None, "moosefs")
    sizes = p["sizes"]
    arena = np.full(int(sizes.sum()), C.FILL, np.uint8)
    offs = np.concatenate([[0], np.cumsum(sizes.ravel())[:-1]]).reshape(
        sizes.shape)
    dst = (arena.ctypes.data + offs).astype(np.uint64)
    bad = np.full(pop.S, 0xFFFFFFFF, np.uint32)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    src_crc = np.ascontiguousarray(p["src_crc"])
    L.check(L.lib().lizec_replicate_ragged_host(
        pop.k, p["oc"], p["tables"].ctypes.data_as(u8p),
        p["tables"].shape[0], p["index"].ctypes.data_as(u32p),
        p["src"].ctypes.data_as(u64p), p["src_nb"].ctypes.data_as(u32p),
        src_crc.ctypes.data_as(u64p), p["sigs"].ctypes.data_as(u8p), 22,
        p["head"], p["coff"], dst.ctypes.data_as(u64p),
        p["dst_nb"].ctypes.data_as(u32p), pop.S, 0, bad.ctypes.data_as(u32p)))
    exp = [0] * pop.S
    exp[C.V_CHUNK] = 1 << C.V_SLOT
    assert bad.tolist() == exp
    assert not (arena == C.FILL).all()
    # chunk 0 is untouched by the corruption: its images are the expected ones
    for j, part in enumerate(C.PER_CHUNK[0]):
        n = int(sizes[0, j])
        assert np.array_equal(arena[int(offs[0, j]):int(offs[0, j]) + n],
                              pop.expected(0, part, "moosefs"))
