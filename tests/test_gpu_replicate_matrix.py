"""The streaming rebuild pipeline (lizec_replicate_run and
lizec_replicate_run_interleaved, replicate_run_impl in csrc/lizec_gpu.hip)
over its stage loop, its shapes, both image formats and its refusals.
tests/KERNEL_COVERAGE_REPLICATE.md says which cell reaches which branch.

Every comparison is bit-exact and every expected byte comes from the oracle:
parities from oracle.rs_encode, images from scrub.build_chunk_image with
oracle.crc32 over the ORIGINAL part bytes.  Chunk s has id 7000 + 13*s and
the version is 9, so a signature taken from another chunk or stage shows.

Every call gets row-strided arrays: a surviving part is a view into an array
of 0xA5 whose rows lie plen + 512 bytes apart, the part 256 bytes in; an
output is a view into such a buffer with 256 guard bytes on either side of
every image.  After the call the WHOLE output buffers are compared (images
equal to the reference, every guard byte still 0xA5), the whole source
arrays are compared with a copy taken before, and every emitted image goes
through scrub.scrub_batch in its own format."""
import ctypes
import functools

import numpy as np
import pytest

import oracle

from lizardfs_amd import slice_traits as st

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
GUARD = 256
FILL = 0xA5
VERSION = 9
FORMATS = ("moosefs", "interleaved")

u8p = ctypes.POINTER(ctypes.c_uint8)
u64p = ctypes.POINTER(ctypes.c_uint64)


def chunk_ids(S):
    return [7000 + 13 * s for s in range(S)]


@functools.lru_cache(maxsize=None)
def stripes(k, m, nblocks, S):
    """parts [S, k+m, plen]: random data, distinct per chunk and part, and
    the oracle's parities; read-only, shared by the cells of one shape."""
    plen = nblocks * st.BLOCK_SIZE
    rng = np.random.default_rng([k, m, nblocks, S, 20251])
    data = rng.integers(0, 256, (S, k, plen), np.uint8)
    parity = np.stack([np.stack(oracle.rs_encode(k, m, list(data[s]), plen))
                       for s in range(S)])
    parts = np.concatenate([data, parity], axis=1)
    parts.setflags(write=False)
    return parts


@functools.lru_cache(maxsize=None)
def reference_images(fmt, k, m, nblocks, S, want):
    """ref[p][s], from the original bytes of part p of chunk s."""
    from lizardfs_amd import scrub
    parts = stripes(k, m, nblocks, S)
    t = st.ec_slice_type(k, m)
    ids = chunk_ids(S)
    ref = {}
    for p in want:
        ref[p] = []
        for s in range(S):
            img = scrub.build_chunk_image(
                ids[s], VERSION, t, p,
                [parts[s, p, b * st.BLOCK_SIZE:(b + 1) * st.BLOCK_SIZE]
                 for b in range(nblocks)],
                crc32_fn=oracle.crc32, fmt=fmt)
            img.setflags(write=False)
            ref[p].append(img)
    return ref


def image_bytes(fmt, k, m, nblocks):
    from lizardfs_amd import scrub
    if fmt == "interleaved":
        return nblocks * scrub.HDD_BLOCK
    return scrub.header_size(st.ec_slice_type(k, m)) + \
        nblocks * st.BLOCK_SIZE


def guarded(rows, width, pinned=False):
    """(whole buffer [rows, width + 2*GUARD] of 0xA5, the view [rows, width]
    GUARD bytes into every row)."""
    from lizardfs_amd import lib as L
    shape = (rows, width + 2 * GUARD)
    whole = L.pinned_empty(shape) if pinned else np.empty(shape, np.uint8)
    whole[:] = FILL
    view = whole[:, GUARD:GUARD + width]
    assert view.strides == (width + 2 * GUARD, 1)
    return whole, view


def first_difference(got, exp):
    bad = np.argwhere(got != exp)
    if bad.size == 0:
        return None
    r, c = (int(x) for x in bad[0])
    return (f"{len(bad)} bytes differ, first in row {r} at {c - GUARD} "
            f"from the image's start: {int(got[r, c]):#x}, "
            f"expected {int(exp[r, c]):#x}")


def check_recover_reference(k, m, nblocks, S, erased, want):
    """oracle.rs_recover over the survivors gives the original bytes: the
    reference recovery itself, not only the round trip."""
    parts = stripes(k, m, nblocks, S)
    plen = nblocks * st.BLOCK_SIZE
    mask = sum(1 << i for i in erased)
    for s in range(S):
        frags = [None if i in erased else np.ascontiguousarray(parts[s, i])
                 for i in range(k + m)]
        rec = oracle.rs_recover(k, m, frags, mask, set(want), plen)
        for p in want:
            assert np.array_equal(rec[p], parts[s, p]), (s, p)


def run_cell(fmt, k, m, nblocks, S, erased, want, sub_batch, pinned=()):
    """One replicate_stream call, shaped and checked as the module docstring
    says.  pinned: the wanted parts whose output buffer is pinned."""
    import torch
    from lizardfs_amd import scrub
    from lizardfs_amd.replicate import replicate_stream
    plen = nblocks * st.BLOCK_SIZE
    parts = stripes(k, m, nblocks, S)
    ref = reference_images(fmt, k, m, nblocks, S, tuple(want))
    img = image_bytes(fmt, k, m, nblocks)

    src_whole, host_parts = {}, []
    for i in range(k + m):
        if i in erased:
            host_parts.append(None)
            continue
        whole, view = guarded(S, plen)
        view[:] = parts[:, i]
        src_whole[i] = whole
        host_parts.append(view)
    src_before = {i: a.copy() for i, a in src_whole.items()}
    dst_whole, out = {}, {}
    for p in want:
        dst_whole[p], out[p] = guarded(S, img, pinned=p in pinned)

    got = replicate_stream(k, m, host_parts, erased, want, chunk_ids(S),
                           version=VERSION, out=out, sub_batch=sub_batch,
                           fmt=fmt)
    assert sorted(got) == sorted(want)

    for p in want:
        assert got[p] is out[p]
        exp = np.full_like(dst_whole[p], FILL)
        exp[:, GUARD:GUARD + img] = np.stack(ref[p])
        assert first_difference(dst_whole[p], exp) is None, \
            f"part {p}: {first_difference(dst_whole[p], exp)}"
    for i, a in src_whole.items():
        assert np.array_equal(a, src_before[i]), \
            f"surviving part {i} or its surroundings were written"

    t = st.ec_slice_type(k, m)
    batch = [(torch.from_numpy(np.ascontiguousarray(out[p][s])).cuda(), t,
              fmt) for p in want for s in range(S)]
    assert scrub.scrub_batch(batch) == [None] * len(batch)


# (nchunks, sub_batch): auto with one stage and slot 1 never used; every slot
# reused; two full stages and a short one; exact fit; clamped to nchunks; an
# exact multiple with each slot used once; a single chunk.
STAGES = [(5, 0), (5, 1), (5, 2), (5, 5), (5, 7), (4, 2), (1, 0)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nchunks,sub_batch", STAGES)
def test_stage_cell(nchunks, sub_batch, fmt):
    """ec(3,2), a data part and a parity part erased, parts of 2 blocks;
    part 1's images go to a pinned buffer, part 3's to pageable numpy."""
    k, m, nblocks, erased = 3, 2, 2, (1, 3)
    if (nchunks, sub_batch) == (5, 2):
        check_recover_reference(k, m, nblocks, nchunks, erased, erased)
    run_cell(fmt, k, m, nblocks, nchunks, erased, erased, sub_batch,
             pinned=(1,))


# (k, m, erased, want, blocks): the smallest legal shape; oc = 1 < m, a parity
# alone from a pattern that also lost data; encode through the recover path;
# Cauchy matrix with oc = 9, a second EC pass with dest_base 8; ic = 32.
SHAPES = [
    (2, 1, (0,), (0,), 1),
    (3, 2, (0, 4), (4,), 1),
    (8, 2, (8, 9), (8, 9), 2),
    (4, 9, (0, 2, 4, 5, 6, 7, 8, 9, 10), (0, 2, 4, 5, 6, 7, 8, 9, 10), 1),
    (32, 2, (5, 33), (5, 33), 1),
]
SHAPE_IDS = ["ec2_1", "ec3_2-parity-alone", "ec8_2-encode", "ec4_9-cauchy",
             "ec32_2"]
SHAPE_CHUNKS = 3


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k,m,erased,want,nblocks", SHAPES, ids=SHAPE_IDS)
def test_shape_cell(k, m, erased, want, nblocks, fmt):
    """sub_batch 2 over 3 chunks (a full stage and a short one), every
    buffer pageable."""
    if (k, m) == (4, 9):
        assert st.is_ec2(st.ec_slice_type(k, m))
        check_recover_reference(k, m, nblocks, SHAPE_CHUNKS, erased, want)
    run_cell(fmt, k, m, nblocks, SHAPE_CHUNKS, erased, want, sub_batch=2)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k,m,erased,want,nblocks", SHAPES, ids=SHAPE_IDS)
def test_device_resident_path(k, m, erased, want, nblocks, fmt):
    """rebuild_part_images, survivors as CUDA tensors, builds the same
    images as the reference."""
    import torch
    from lizardfs_amd.replicate import rebuild_part_images
    S = SHAPE_CHUNKS
    parts = stripes(k, m, nblocks, S)
    ref = reference_images(fmt, k, m, nblocks, S, tuple(want))
    frags = [None if i in erased else
             torch.from_numpy(np.ascontiguousarray(parts[:, i])).cuda()
             for i in range(k + m)]
    images = rebuild_part_images(k, m, frags, erased, set(want),
                                 chunk_ids(S), VERSION, fmt=fmt)
    torch.cuda.synchronize()
    assert sorted(images) == sorted((s, p) for p in want for s in range(S))
    for (s, p), img in images.items():
        assert np.array_equal(img.cpu().numpy(), ref[p][s]), (s, p)
    for i, f in enumerate(frags):
        if f is not None:
            assert np.array_equal(f.cpu().numpy(), parts[:, i]), \
                f"surviving part {i} was modified"


# ---------------------------------------------------------------------------
# Refusals, through the C ABI
# ---------------------------------------------------------------------------

class AbiCall:
    """A valid small call of either entry point — ec(3,2), erased (1, 3),
    parts of one block, 2 chunks — whose arguments a case changes one at a
    time.  Destinations are images inside guarded buffers of 0xA5 that have
    room for the few extra bytes of the header_size cases."""
    K, M, NBLOCKS, S = 3, 2, 1, 2
    ERASED = (1, 3)

    def __init__(self, entry):
        from lizardfs_amd import lib as L
        from lizardfs_amd import scrub
        self.entry = entry
        self.fmt = "moosefs" if entry == "run" else "interleaved"
        k, m, S = self.K, self.M, self.S
        self.lib, self.eng = L.lib(), L.engine(0)
        parts = stripes(k, m, self.NBLOCKS, S)
        surv = [i for i in range(k + m) if i not in self.ERASED]
        present = sum(1 << i for i in surv)
        needed = sum(1 << i for i in self.ERASED)
        self.tbl = np.zeros(32 * 32 * 32, np.uint8)
        ic, oc = ctypes.c_int(), ctypes.c_int()
        assert self.lib.lizec_rs_tables(
            k, m, present, present, needed, self.tbl.ctypes.data_as(u8p),
            ctypes.byref(ic), ctypes.byref(oc)) == LIZEC_OK
        assert (ic.value, oc.value) == (len(surv), len(self.ERASED))
        self.srcs = [np.ascontiguousarray(parts[:, i]) for i in surv]
        self.img = image_bytes(self.fmt, k, m, self.NBLOCKS)
        self.dst_whole, self.dst = zip(*(guarded(S, self.img)
                                         for _ in self.ERASED))
        self.src_ptrs = np.array(
            [[a[s].ctypes.data for a in self.srcs] for s in range(S)],
            np.uint64)
        self.dst_ptrs = np.array(
            [[a[s].ctypes.data for a in self.dst] for s in range(S)],
            np.uint64)
        self.hdr = scrub.header_size(st.ec_slice_type(k, m))
        # room for sig_len = header_size + 1
        self.sigs = np.zeros((S, oc.value, self.hdr + 1), np.uint8)
        self.args = dict(
            e=self.eng, part_len=self.NBLOCKS * st.BLOCK_SIZE, ic=ic.value,
            oc=oc.value, gftbls=self.tbl.ctypes.data_as(u8p),
            host_src=self.src_ptrs.ctypes.data_as(u64p), sigs=None,
            sig_len=0, header_size=self.hdr, crc_off=scrub.SIGNATURE_BLOCK,
            host_dst=self.dst_ptrs.ctypes.data_as(u64p), nchunks=S,
            sub_batch=1)

    def call(self, **changed):
        a = dict(self.args, **changed)
        if self.entry == "run":
            return self.lib.lizec_replicate_run(
                a["e"], a["part_len"], a["ic"], a["oc"], a["gftbls"],
                a["host_src"], a["sigs"], a["sig_len"], a["header_size"],
                a["crc_off"], a["host_dst"], a["nchunks"], a["sub_batch"])
        return self.lib.lizec_replicate_run_interleaved(
            a["e"], a["part_len"], a["ic"], a["oc"], a["gftbls"],
            a["host_src"], a["host_dst"], a["nchunks"], a["sub_batch"])

    def untouched(self):
        return all((w == FILL).all() for w in self.dst_whole)


SHARED_REFUSALS = [
    ("engine-null", dict(e=None)),
    ("gftbls-null", dict(gftbls=None)),
    ("host_src-null", dict(host_src=None)),
    ("host_dst-null", dict(host_dst=None)),
    ("nchunks-0", dict(nchunks=0)),
    ("ic-0", dict(ic=0)),
    ("ic-33", dict(ic=33)),
    ("oc-0", dict(oc=0)),
    ("oc-33", dict(oc=33)),
    ("part_len-0", dict(part_len=0)),
    ("part_len-65552", dict(part_len=65536 + 16)),
    ("part_len-2g+64k", dict(part_len=2 ** 31 + 65536)),
]


@pytest.mark.parametrize("entry", ("run", "interleaved"))
@pytest.mark.parametrize("changed", [c for _, c in SHARED_REFUSALS],
                         ids=[n for n, _ in SHARED_REFUSALS])
def test_refusal(changed, entry):
    """check_replicate_args: LIZEC_EINVAL from the host, destinations
    untouched."""
    c = AbiCall(entry)
    assert c.call(**changed) == LIZEC_EINVAL
    assert c.untouched()


MOOSEFS_REFUSALS = [
    ("sig_len-header+1", lambda c: dict(
        sigs=c.sigs.ctypes.data_as(u8p), sig_len=c.hdr + 1)),
    ("crc-array-past-header", lambda c: dict(
        crc_off=c.hdr + 4 - 4 * c.NBLOCKS)),
    ("header_size-4100", lambda c: dict(header_size=4100)),
    ("header_size-4104", lambda c: dict(header_size=4104)),
]


@pytest.mark.parametrize("change", [c for _, c in MOOSEFS_REFUSALS],
                         ids=[n for n, _ in MOOSEFS_REFUSALS])
def test_refusal_moosefs_header(change):
    """lizec_replicate_run's own conditions: the signature and the CRC array
    fit in the header, and header_size is a multiple of 16 (4100 and 4104
    hold both and are 4 and 8 mod 16)."""
    c = AbiCall("run")
    changed = change(c)
    if "header_size" in changed:
        assert changed["header_size"] >= c.hdr    # the other rules hold
    assert c.call(**changed) == LIZEC_EINVAL
    assert c.untouched()


@pytest.mark.parametrize("entry", ("run", "interleaved"))
def test_refusal_base_call_succeeds(entry):
    """The positive control: the call that every refusal cell spoils is
    itself accepted and right.  For lizec_replicate_run it has sigs = NULL
    and sig_len = 0: the images' first 1024 bytes are zero and the rest
    equals the reference."""
    from lizardfs_amd import scrub
    c = AbiCall(entry)
    assert c.call() == LIZEC_OK
    ref = reference_images(c.fmt, c.K, c.M, c.NBLOCKS, c.S, c.ERASED)
    for j, p in enumerate(c.ERASED):
        exp = np.full_like(c.dst_whole[j], FILL)
        exp[:, GUARD:GUARD + c.img] = np.stack(ref[p])
        if entry == "run":
            assert exp[:, GUARD:GUARD + 22].any()
            exp[:, GUARD:GUARD + scrub.SIGNATURE_BLOCK] = 0
        assert first_difference(c.dst_whole[j], exp) is None, \
            f"part {p}: {first_difference(c.dst_whole[j], exp)}"
    for a, i in zip(c.srcs, (0, 2, 4)):
        assert np.array_equal(a, stripes(c.K, c.M, c.NBLOCKS, c.S)[:, i])
