"""Shared by the ragged streaming-rebuild tests (host twin and GPU): the
population, the expected images and the checks.

ec(3,2), six chunks of 1, 2, 3, 4, 5 and 7 blocks — the population of
test_gpu_ragged_rebuild.py: parts of 0..3 blocks, most last rows short.  The
expected images are scrub.build_chunk_image over parts made with
oracle.rs_encode and CRCs from oracle.crc32, never from the code under test.
Host sources hold 0xFF from the end of each part's own count on; destination
buffers are OVER bytes longer than the image and prefilled with 0xA5.
"""
import functools

import numpy as np

import oracle

from lizardfs_amd import scrub
from lizardfs_amd import slice_traits as st

K, M = 3, 2
CHUNK_BLOCKS = (1, 2, 3, 4, 5, 7)
BLOCK = st.BLOCK_SIZE
FILL = 0xA5
OVER = 48
VERSION = 7
FORMATS = ("moosefs", "interleaved")
PER_CHUNK = [(0, 3), (1, 4), (3, 4), (0, 1), (2, 4), (1, 2)]


class Population:
    """Chunks of `chunk_blocks` blocks in ec(k, m): oracle parts, their CRCs
    and the expected images; everything read-only."""

    def __init__(self, k, m, chunk_blocks, seed):
        self.k, self.m = k, m
        self.nparts = k + m
        self.chunk_blocks = tuple(chunk_blocks)
        self.S = len(chunk_blocks)
        self.T = st.ec_slice_type(k, m)
        self.chunk_ids = [0x1000 + s for s in range(self.S)]
        rng = np.random.default_rng(seed)
        self.pb = np.array(
            [[st.number_of_blocks(self.T, p, n) for p in range(self.nparts)]
             for n in chunk_blocks], np.int64)
        self.nmax = int(self.pb.max())
        lmax = self.nmax * BLOCK
        self.parts = np.zeros((self.S, self.nparts, lmax), np.uint8)
        for s, n in enumerate(chunk_blocks):
            chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
            for b in range(n):
                self.parts[s, b % k, (b // k) * BLOCK:(b // k + 1) * BLOCK] = \
                    chunk[b]
            par = oracle.rs_encode(
                k, m, [np.ascontiguousarray(self.parts[s, p])
                       for p in range(k)], lmax)
            for l in range(m):
                self.parts[s, k + l] = par[l]
        # big-endian CRC of every block of every part; 0xFF past the count
        self.crcs = np.full((self.S, self.nparts, self.nmax, 4), 0xFF,
                            np.uint8)
        for s in range(self.S):
            for p in range(self.nparts):
                for b in range(int(self.pb[s, p])):
                    c = oracle.crc32(self.parts[s, p, b * BLOCK:(b + 1) * BLOCK])
                    self.crcs[s, p, b] = np.frombuffer(
                        int(c).to_bytes(4, "big"), np.uint8)
        for a in (self.parts, self.pb, self.crcs):
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def expected(self, s, p, fmt):
        n = int(self.pb[s, p])
        blocks = [self.parts[s, p, b * BLOCK:(b + 1) * BLOCK]
                  for b in range(n)]
        img = scrub.build_chunk_image(self.chunk_ids[s], VERSION, self.T, p,
                                      blocks, crc32_fn=oracle.crc32, fmt=fmt)
        img.setflags(write=False)
        return img

    def sources(self):
        """host_parts: every part [S, Lmax], 0xFF from the end of each
        chunk's own count on."""
        out = []
        for p in range(self.nparts):
            a = np.array(self.parts[:, p])
            for s in range(self.S):
                a[s, int(self.pb[s, p]) * BLOCK:] = 0xFF
            out.append(a)
        return out

    def source_crcs(self):
        """crcs: every part [S, nmax, 4] uint8."""
        return [np.array(self.crcs[:, p]) for p in range(self.nparts)]

    def image_size(self, s, p, fmt):
        return self.expected(s, p, fmt).size


@functools.lru_cache(maxsize=None)
def base():
    return Population(K, M, CHUNK_BLOCKS, 311)


@functools.lru_cache(maxsize=None)
def ones():
    """Every chunk has one block: parts 1 and 2 have none."""
    return Population(K, M, (1,) * 4, 312)


def per_chunk(sets, S):
    sets = list(sets)
    if sets and all(isinstance(i, int) for i in sets):
        return [tuple(sets)] * S
    return [tuple(x) for x in sets]


def run(fn, pop, erased, want, fmt, crcs=None, parts=None, **kw):
    """Call `fn` (replicate_stream_ragged or its host twin) with destination
    buffers OVER bytes too long and prefilled; returns (result, buffers)."""
    parts = pop.sources() if parts is None else parts
    keep = [a.copy() for a in parts]
    wants = per_chunk(erased if want is None else want, pop.S)
    bufs, out = {}, {}
    for s, w in enumerate(wants):
        for p in w:
            n = pop.image_size(s, p, fmt)
            bufs[(s, p)] = np.full(n + OVER, FILL, np.uint8)
            out[(s, p)] = bufs[(s, p)][:n]
    res = fn(pop.k, pop.m, parts, pop.chunk_blocks, erased, want,
             pop.chunk_ids, VERSION, crcs=crcs, out=out, fmt=fmt, **kw)
    for a, b in zip(parts, keep):
        assert np.array_equal(a, b), "the sources were modified"
    return res, bufs


def check_images(res, bufs, pop, erased, want, fmt, skip=()):
    """Every wanted image equals the expected one byte for byte and the
    bytes behind it are untouched; chunks in `skip` are expected to be
    missing from the result."""
    wants = per_chunk(erased if want is None else want, pop.S)
    keys = {(s, p) for s, w in enumerate(wants) for p in w if s not in skip}
    assert set(res.images) == keys
    for (s, p) in sorted(keys):
        exp = pop.expected(s, p, fmt)
        got = res.images[(s, p)]
        assert got.shape == exp.shape, (s, p)
        assert np.array_equal(got, exp), (fmt, s, p)
    for (s, p), b in bufs.items():
        n = pop.image_size(s, p, fmt)
        if s not in skip:
            assert np.array_equal(b[:n], pop.expected(s, p, fmt)), (s, p)
        assert (b[n:] == FILL).all(), (fmt, s, p, "overrun")


# the image cases: (population, erased, want)
IMAGE_CASES = {
    "one_pattern": (base, (0, 3), None),
    "per_chunk": (base, PER_CHUNK, None),
    "want_one_and_two": (base, PER_CHUNK,
                         [(0, 3), (4,), (3, 4), (0,), (2, 4), (2,)]),
    "header_only": (base, (1, 2), None),
    "no_blocks_anywhere": (ones, (2, 4), (2,)),
}

# the verification cases: corruption of (chunk 3, slot 1, block 1) under the
# per-chunk patterns, where chunk 3 (4 blocks) has lost parts 0 and 1, so its
# slot 1 is part 3 (survivors 2, 3, 4), which has two blocks
V_ERASED = PER_CHUNK
V_CHUNK, V_SLOT, V_PART, V_BLOCK = 3, 1, 3, 1


def verify_inputs(pop, what):
    """(parts, crcs, expected bad masks) for one verification case."""
    parts, crcs = pop.sources(), pop.source_crcs()
    bad = {}
    assert pop.pb[V_CHUNK, V_PART] > V_BLOCK
    if what == "clean":
        pass
    elif what == "data_byte":
        parts[V_PART][V_CHUNK, V_BLOCK * BLOCK + 777] ^= 0x10
        bad = {V_CHUNK: {V_PART}}
    elif what == "crc_byte":
        crcs[V_PART][V_CHUNK, V_BLOCK, 2] ^= 0x01
        bad = {V_CHUNK: {V_PART}}
    elif what == "past_count":
        # chunk 2 (3 blocks, survivors 0, 1, 2): part 1 has one block; flip
        # the byte behind it and the CRC slot behind its only CRC
        assert pop.pb[2, 1] == 1
        parts[1][2, BLOCK] ^= 0xFF
        crcs[1][2, 1, 0] ^= 0xFF
    elif what == "unverified_slot":
        parts[V_PART][V_CHUNK, V_BLOCK * BLOCK + 777] ^= 0x10
        crcs[V_PART] = None
    else:
        raise AssertionError(what)
    return parts, crcs, bad


VERIFY_CASES = ("clean", "data_byte", "crc_byte", "past_count",
                "unverified_slot")
