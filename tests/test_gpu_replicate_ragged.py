"""The ragged streaming rebuild on the GPU: replicate_stream_ragged over
lizec_replicate_run_ragged, against images built from the oracle's parts and
against the host twin (replicate_ragged_cases.py)."""
import ctypes

import numpy as np
import pytest

import replicate_ragged_cases as C

from lizardfs_amd import lib as L
from lizardfs_amd import replicate
from lizardfs_amd import scrub
from lizardfs_amd import slice_traits as st

pytestmark = pytest.mark.gpu

GPU = replicate.replicate_stream_ragged
HOST = replicate.replicate_stream_ragged_host


def same_as_host(res, pop, erased, want, fmt, crcs=None, parts=None):
    ref, _ = C.run(HOST, pop, erased, want, fmt, crcs=crcs, parts=parts)
    assert res.corrupt == ref.corrupt
    assert set(res.images) == set(ref.images)
    for key, img in ref.images.items():
        assert np.array_equal(res.images[key], img), (fmt, key)


@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("case", sorted(C.IMAGE_CASES))
def test_images(case, fmt):
    popf, erased, want = C.IMAGE_CASES[case]
    pop = popf()
    res, bufs = C.run(GPU, pop, erased, want, fmt)
    assert res.corrupt == {}
    C.check_images(res, bufs, pop, erased, want, fmt)
    same_as_host(res, pop, erased, want, fmt)


def footprints(pop, erased, fmt):
    """Per chunk: source bytes plus image bytes, each image rounded to 16."""
    p = replicate._stream_ragged_prepare(
        pop.k, pop.m, pop.sources(), pop.chunk_blocks, erased, None,
        pop.chunk_ids, C.VERSION, None, None, fmt)
    foot = p["src_nb"].astype(np.int64).sum(axis=1) * C.BLOCK + \
        ((p["sizes"] + 15) & ~15).sum(axis=1)
    return p, foot


def stage_cut(p, fmt, stage_bytes):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    S, oc = p["dst_nb"].shape
    first = np.zeros(S + 1, np.uint32)
    dst = np.ones((S, oc), np.uint64)       # every slot wanted
    n = L.lib().lizec_replicate_ragged_stages(
        p["src_nb"].shape[1], oc, p["src_nb"].ctypes.data_as(u32p),
        dst.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        p["dst_nb"].ctypes.data_as(u32p), S, p["head"], p["flags"],
        stage_bytes, first.ctypes.data_as(u32p), S + 1)
    assert n >= 1
    return first[:n + 1].tolist()


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_stage_settings(fmt):
    """The same run cut into one stage, one chunk per stage (each slot used
    three times), with room for two of the largest chunks, and with the
    largest chunk oversized: identical output."""
    pop = C.base()
    p, foot = footprints(pop, C.PER_CHUNK, fmt)
    pair = int(max(foot[0] + foot[1], foot[2] + foot[3], foot[4] + foot[5]))
    settings = {0: [0, 6], 1: [0, 1, 2, 3, 4, 5, 6],
                int(foot[5]) - 1: None, pair: None}
    cuts = {sb: stage_cut(p, fmt, sb) for sb in settings}
    assert cuts[0] == [0, 6] and cuts[1] == [0, 1, 2, 3, 4, 5, 6]
    assert cuts[int(foot[5]) - 1] == [0, 3, 4, 5, 6]  # chunk 5 oversized
    assert cuts[pair] == [0, 4, 6]       # room for the two largest chunks
    for sb in settings:
        res, bufs = C.run(GPU, pop, C.PER_CHUNK, None, fmt, stage_bytes=sb)
        C.check_images(res, bufs, pop, C.PER_CHUNK, None, fmt)


def test_pinned_and_pageable_sources():
    pop = C.base()
    parts = pop.sources()
    pinned = L.pinned_empty(parts[2].shape)
    pinned[:] = parts[2]
    parts[2] = pinned
    res, bufs = C.run(GPU, pop, C.PER_CHUNK, None, "moosefs", parts=parts)
    C.check_images(res, bufs, pop, C.PER_CHUNK, None, "moosefs")


def test_allocated_pinned_arena():
    pop = C.base()
    res = GPU(pop.k, pop.m, pop.sources(), pop.chunk_blocks, C.PER_CHUNK,
              None, pop.chunk_ids, C.VERSION, fmt="interleaved")
    C.check_images(res, {}, pop, C.PER_CHUNK, None, "interleaved")


@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("what", C.VERIFY_CASES)
def test_verification(what, fmt):
    pop = C.base()
    parts, crcs, bad = C.verify_inputs(pop, what)
    res, bufs = C.run(GPU, pop, C.V_ERASED, None, fmt, crcs=crcs, parts=parts)
    assert res.corrupt == bad
    same_as_host(res, pop, C.V_ERASED, None, fmt, crcs=crcs, parts=parts)
    skip = set(bad)
    if what == "unverified_slot":
        skip = {C.V_CHUNK}
        res.images.pop((C.V_CHUNK, 0))
        res.images.pop((C.V_CHUNK, 1))
    # the images of the uncorrupted chunks are unchanged by the corruption
    C.check_images(res, bufs, pop, C.V_ERASED, None, fmt, skip=skip)


def test_verification_per_stage_masks():
    """One chunk per stage: the masks come home from the right stage."""
    pop = C.base()
    parts, crcs, bad = C.verify_inputs(pop, "data_byte")
    res, _ = C.run(GPU, pop, C.V_ERASED, None, "moosefs", crcs=crcs,
                   parts=parts, stage_bytes=1)
    assert res.corrupt == bad


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_equals_device_resident_rebuild_and_scrubs_clean(fmt):
    import torch
    pop = C.base()
    erased = (0, 3)
    res, _ = C.run(GPU, pop, erased, None, fmt)
    frags = [None if p in erased else torch.from_numpy(a).cuda()
             for p, a in enumerate(pop.sources())]
    dev = replicate.rebuild_part_images(
        pop.k, pop.m, frags, erased, None, pop.chunk_ids, C.VERSION, fmt=fmt,
        chunk_blocks=pop.chunk_blocks)
    torch.cuda.synchronize()
    assert set(dev) == set(res.images)
    for key, img in dev.items():
        assert np.array_equal(img.cpu().numpy(), res.images[key]), (fmt, key)
    up = [(torch.from_numpy(np.array(img)).cuda(), pop.T, fmt)
          for _, img in sorted(res.images.items())]
    assert scrub.scrub_batch(up) == [None] * len(up)


def test_call_sequence():
    """Three ragged streams in one process with a device-resident ragged
    recover on the default stream between them, then the uniform stream:
    every result is right, so no call leaves scratch behind that the next
    one trips over."""
    import torch
    from lizardfs_amd.ec import ReedSolomon
    pop = C.base()
    rs = ReedSolomon(pop.k, pop.m)
    erased = (0, 3)
    frags = [None if p in erased else torch.from_numpy(a).cuda()
             for p, a in enumerate(pop.sources())]
    lmax = pop.nmax * C.BLOCK
    for i, (e, fmt, sb) in enumerate([(C.PER_CHUNK, "moosefs", 0),
                                      ((0, 3), "interleaved", 1),
                                      (C.PER_CHUNK, "moosefs", 1)]):
        res, bufs = C.run(GPU, pop, e, None, fmt, stage_bytes=sb)
        C.check_images(res, bufs, pop, e, None, fmt)
        out = torch.full((pop.S, 2, lmax), C.FILL, dtype=torch.uint8,
                         device="cuda")
        _, slots = rs.recover_batch_ragged(frags, erased, out=out,
                                           part_blocks=pop.pb)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for s in range(pop.S):
            for j, p in enumerate(erased):
                n = int(pop.pb[s, p]) * C.BLOCK
                assert np.array_equal(got[s, j, :n], pop.parts[s, p, :n]), \
                    (i, s, p)
                assert (got[s, j, n:] == C.FILL).all()
    # the uniform pipeline, on full-length (zero-padded) parts
    parts = [None if p in erased else np.array(pop.parts[:, p])
             for p in range(pop.nparts)]
    uni = replicate.replicate_stream(pop.k, pop.m, parts, erased, erased,
                                     pop.chunk_ids, C.VERSION)
    for p in erased:
        for s in range(pop.S):
            blocks = [pop.parts[s, p, b * C.BLOCK:(b + 1) * C.BLOCK]
                      for b in range(pop.nmax)]
            exp = scrub.build_chunk_image(pop.chunk_ids[s], C.VERSION, pop.T,
                                          p, blocks)
            assert np.array_equal(uni[p][s], exp), (s, p)


def test_ec82_product_shape():
    """ec(8,2), chunks of 1, 8, 9 and 17 blocks, one lost data part per chunk
    at a different index, MooseFS, two stages."""
    pop = C.Population(8, 2, (1, 8, 9, 17), 313)
    erased = [(0, 9), (3, 9), (5, 9), (7, 9)]
    want = [(0,), (3,), (5,), (7,)]
    p = replicate._stream_ragged_prepare(
        pop.k, pop.m, pop.sources(), pop.chunk_blocks, erased, want,
        pop.chunk_ids, C.VERSION, None, None, "moosefs")
    foot = p["src_nb"].astype(np.int64).sum(axis=1) * C.BLOCK + \
        ((p["sizes"] + 15) & ~15).sum(axis=1)
    sb = int(foot[0] + foot[1] + foot[2])
    assert stage_cut(p, "moosefs", sb) == [0, 3, 4]
    res, bufs = C.run(GPU, pop, erased, want, "moosefs", stage_bytes=sb,
                      crcs=pop.source_crcs())
    assert res.corrupt == {}
    C.check_images(res, bufs, pop, erased, want, "moosefs")
    same_as_host(res, pop, erased, want, "moosefs")
