"""Goal change through the Python layer: convert.convert_parts and
replicate.convert_part_images build the parts of one slice type from chunks
held in another (lizec_ec_encode_batch_view).

Seven chunks of 1, 2, 3, 4, 5, 7 and 17 blocks.  The expected bytes are
built without the code under test, with the numpy model of
test_convert_host.py: the chunk is split into the source slice's data parts,
which become the fragments; for the target the chunk is zero-padded to whole
rows, a data part is a column of the rows (a plain copy) and a parity part is
oracle.ec_encode_data over the row's columns with oracle.rs_make_tables
tables (XOR of the columns for a xor target).  Fragment rows beyond a part's
own length hold 0xFF, so reading them changes the result; outputs are
prefilled with 0xA5 and compared whole.
"""
import struct

import numpy as np
import pytest

import oracle

from lizardfs_amd import slice_traits as st
from test_convert_host import split_chunk, target_rows

pytestmark = pytest.mark.gpu

CHUNK_BLOCKS = (1, 2, 3, 4, 5, 7, 17)
S = len(CHUNK_BLOCKS)
BLOCK = st.BLOCK_SIZE
FILL = 0xA5
VERSION = 9
CHUNK_IDS = [0x2000 + s for s in range(S)]
STD = st.K_STANDARD
XOR2, XOR3 = st.K_XOR2, st.K_XOR2 + 1
EC32, EC82 = st.ec_slice_type(3, 2), st.ec_slice_type(8, 2)
EC51, EC21 = st.ec_slice_type(5, 1), st.ec_slice_type(2, 1)
CONVERSIONS = {"std-ec32": (STD, EC32), "xor3-ec32": (XOR3, EC32),
               "ec32-ec82": (EC32, EC82), "ec51-ec21": (EC51, EC21),
               "ec32-xor2": (EC32, XOR2)}


def total_parts(t):
    return st.data_parts(t) + st.parity_parts(t)


def data_index(t, part):
    if st.is_xor(t):
        return part - 1 if part >= 1 else None
    return part if part < st.data_parts(t) else None


_chunks = None


def chunks():
    """The S chunks, [n, BLOCK] each, read-only."""
    global _chunks
    if _chunks is None:
        rng = np.random.default_rng(411)
        _chunks = [rng.integers(0, 256, (n, BLOCK), np.uint8)
                   for n in CHUNK_BLOCKS]
        for c in _chunks:
            c.setflags(write=False)
    return _chunks


_parts = {}


def slice_parts(t):
    """Every part of every chunk stored as slice type t, from the model and
    the oracle: list over chunks of list over parts of [blocks, BLOCK]."""
    if t in _parts:
        return _parts[t]
    k, m = st.data_parts(t), st.parity_parts(t)
    out = []
    for chunk in chunks():
        data = split_chunk(chunk, k)
        rows = target_rows(chunk, k)
        cols = [np.ascontiguousarray(rows[:, j]).reshape(-1)
                for j in range(k)]
        par = []
        if st.is_xor(t):
            par = [np.bitwise_xor.reduce(np.stack(cols), axis=0)]
        elif st.is_ec(t):
            dmask = (1 << k) - 1
            for l in range(m):
                tbl, ic, oc = oracle.rs_make_tables(k, m, dmask, dmask,
                                                    1 << (k + l))
                assert (ic, oc) == (k, 1)
                o = np.full(cols[0].size, 0x77, np.uint8)
                oracle.ec_encode_data(tbl, cols, [o])
                par.append(o)
        par = [p.reshape(-1, BLOCK) for p in par]
        parts = (par + data) if st.is_xor(t) else (data + par)
        assert len(parts) == total_parts(t)
        out.append(parts)
    _parts[t] = out
    return out


def fragments(t, only_data=True, lmax_blocks=None):
    """The parts of slice type t as [S, Lmax] CUDA tensors, 0xFF from the
    end of each chunk's own part on; parity parts None if only_data."""
    import torch
    parts = slice_parts(t)
    nb = lmax_blocks or max(p.shape[0] for c in parts for p in c)
    out = []
    for p in range(total_parts(t)):
        if only_data and data_index(t, p) is None:
            out.append(None)
            continue
        a = np.full((S, nb * BLOCK), 0xFF, np.uint8)
        for s in range(S):
            b = parts[s][p].reshape(-1)
            a[s, :b.size] = b
        out.append(torch.from_numpy(a).cuda())
    return out


def check_out(out, slots, want, target, what):
    """out[s, j] holds part slots[s, j]: its own blocks equal the model's,
    every other byte is still FILL; slots are the want sets, ascending."""
    import torch
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exp = slice_parts(target)
    for s in range(S):
        w = sorted(want[s])
        assert [p for p in slots[s] if p >= 0] == w, (what, s)
        for j in range(slots.shape[1]):
            p = int(slots[s, j])
            n = 0
            if p >= 0:
                e = exp[s][p].reshape(-1)
                n = e.size
                assert n == BLOCK * st.number_of_blocks(
                    target, st.data_parts(target)
                    if data_index(target, p) is None
                    else data_index(target, p), CHUNK_BLOCKS[s])
                assert np.array_equal(got[s, j, :n], e), (what, s, p)
            assert (got[s, j, n:] == FILL).all(), (what, s, p, "overrun")


def want_sets(target, kind):
    P, k = total_parts(target), st.data_parts(target)
    parity0 = 0 if st.is_xor(target) else k
    data1 = 2 if st.is_xor(target) else 1
    if kind == "data":
        return [{data1}] * S
    if kind == "parity":
        return [{parity0}] * S
    if kind == "all":
        return [set(range(P))] * S
    sets = [{s % P} | ({(3 * s + 1) % P, parity0} if s % 2 else set())
            for s in range(S)]
    assert len({frozenset(w) for w in sets}) > 3
    return sets


@pytest.mark.parametrize("kind", ("data", "parity", "all", "per-chunk"))
@pytest.mark.parametrize("conv", tuple(CONVERSIONS))
def test_convert_parts(conv, kind):
    import torch
    from lizardfs_amd.convert import convert_parts
    src, target = CONVERSIONS[conv]
    frags = fragments(src)
    keep = [None if f is None else f.clone() for f in frags]
    want = want_sets(target, kind)
    oc = max(len(w) for w in want)
    span = max(p.size for c in slice_parts(target) for p in c)
    out = torch.full((S, oc, span), FILL, dtype=torch.uint8, device="cuda")
    arg = want[0] if kind != "per-chunk" else want
    got, slots = convert_parts(src, frags, CHUNK_BLOCKS, target, arg, out=out)
    assert got is out
    check_out(out, slots, want, target, f"{conv} {kind}")
    for f, k in zip(frags, keep):
        assert f is None or torch.equal(f, k), "the sources were modified"


def test_allocated_and_strided_out():
    """out=None allocates rows for the longest wanted part; a given out may
    keep its blocks at a stride (INTERLEAVED block slots)."""
    import torch
    from lizardfs_amd.convert import convert_parts
    frags = fragments(EC32)
    want = [{0, 8}] * S
    got, slots = convert_parts(EC32, frags, CHUNK_BLOCKS, EC82, {0, 8})
    exp = slice_parts(EC82)
    assert tuple(got.shape) == (S, 2, 3 * BLOCK)
    assert slots.tolist() == [[0, 8]] * S
    torch.cuda.synchronize()
    for s in range(S):
        for j, p in enumerate((0, 8)):
            e = exp[s][p].reshape(-1)
            assert np.array_equal(got[s, j, :e.size].cpu().numpy(), e)
    span = 4 + 3 * 65540
    out = torch.full((S, 2, span), FILL, dtype=torch.uint8, device="cuda")
    convert_parts(EC32, frags, CHUNK_BLOCKS, EC82, want, out=out[:, :, 4:],
                  dst_stride=65540)
    torch.cuda.synchronize()
    want_bytes = np.full((S, 2, span), FILL, np.uint8)
    for s in range(S):
        for j, p in enumerate((0, 8)):
            for b, blk in enumerate(exp[s][p]):
                want_bytes[s, j, 4 + b * 65540:4 + b * 65540 + BLOCK] = blk
    assert np.array_equal(out.cpu().numpy(), want_bytes)


@pytest.mark.parametrize("erased", ((1,), (0, 3)), ids=("data", "data+parity"))
def test_degraded_ec_source(erased):
    """Missing parts of an ec(3,2) source: the data part among them is
    rebuilt first, and the result is that of the undamaged source."""
    import torch
    from lizardfs_amd.convert import convert_parts
    whole = fragments(EC32, only_data=False)
    want = [set(range(10))] * S
    span = 3 * BLOCK
    a = torch.full((S, 10, span), FILL, dtype=torch.uint8, device="cuda")
    b = torch.full((S, 10, span), FILL, dtype=torch.uint8, device="cuda")
    _, slots = convert_parts(EC32, whole, CHUNK_BLOCKS, EC82, want[0], out=a)
    check_out(a, slots, want, EC82, "undamaged")
    damaged = [None if p in erased else f for p, f in enumerate(whole)]
    _, slots = convert_parts(EC32, damaged, CHUNK_BLOCKS, EC82, want[0],
                             out=b, src_erased=set(erased))
    check_out(b, slots, want, EC82, f"erased {erased}")
    assert torch.equal(a, b)


def test_equals_encode_of_the_chunk_stored_as_target():
    """ec(3,2) -> ec(8,2) parity equals recover_batch_ragged's encode over
    the same chunks stored directly as ec(8,2)."""
    import torch
    from lizardfs_amd.convert import convert_parts
    from lizardfs_amd.ec import ReedSolomon
    span = 3 * BLOCK
    a = torch.full((S, 2, span), FILL, dtype=torch.uint8, device="cuda")
    b = torch.full((S, 2, span), FILL, dtype=torch.uint8, device="cuda")
    _, slots = convert_parts(EC32, fragments(EC32), CHUNK_BLOCKS, EC82,
                             {8, 9}, out=a)
    pb = np.array([[st.number_of_blocks(EC82, p, n) for p in range(10)]
                   for n in CHUNK_BLOCKS], np.int64)
    direct = fragments(EC82, lmax_blocks=3)
    _, rslots = ReedSolomon(8, 2).recover_batch_ragged(
        direct, (8, 9), out=b, part_blocks=pb)
    torch.cuda.synchronize()
    assert slots.tolist() == rslots.tolist() == [[8, 9]] * S
    assert torch.equal(a, b)
    check_out(a, slots, [{8, 9}] * S, EC82, "parity of ec(8,2)")


def ref_image(target, s, p, fmt):
    """The image of part p of chunk s, CRCs by the oracle (as in
    test_gpu_ragged_rebuild.py)."""
    from lizardfs_amd import scrub
    blocks = list(slice_parts(target)[s][p])
    if fmt == "moosefs":
        return scrub.build_chunk_image(CHUNK_IDS[s], VERSION, target, p,
                                       blocks, crc32_fn=oracle.crc32)
    out = bytearray()
    for blk in blocks:
        out += struct.pack(">I", oracle.crc32(blk.tobytes())) + blk.tobytes()
    return np.frombuffer(bytes(out), np.uint8)


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_convert_part_images(fmt):
    from lizardfs_amd import scrub
    from lizardfs_amd.replicate import convert_part_images
    want = {1, 7, 8, 9}
    images = convert_part_images(EC32, fragments(EC32), CHUNK_BLOCKS, EC82,
                                 want, CHUNK_IDS, VERSION, fmt=fmt)
    assert sorted(images) == sorted((s, p) for s in range(S) for p in want)
    hdr = scrub.header_size(EC82)
    for (s, p), img in images.items():
        nb = slice_parts(EC82)[s][p].shape[0]
        assert img.numel() == (hdr + nb * BLOCK if fmt == "moosefs"
                               else nb * scrub.HDD_BLOCK), (s, p)
        assert np.array_equal(img.cpu().numpy(),
                              ref_image(EC82, s, p, fmt)), (s, p)
    keys = sorted(images)
    batch = [(images[key], EC82, fmt) for key in keys]
    assert scrub.scrub_batch(batch) == [None] * len(batch)
    # one flipped byte in the last block of the longest image
    at = keys.index((S - 1, 8))
    img = images[(S - 1, 8)]
    assert slice_parts(EC82)[S - 1][8].shape[0] == 3
    img[img.numel() - 100] ^= 0x10
    res = scrub.scrub_batch(batch)
    assert res[at] == 2
    assert [r for i, r in enumerate(res) if i != at] == [None] * (len(batch) - 1)


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_convert_part_images_per_chunk_from_a_copy(fmt):
    """2 copies -> ec(3,2), a want set per chunk."""
    from lizardfs_amd.replicate import convert_part_images
    want = want_sets(EC32, "per-chunk")
    images = convert_part_images(STD, fragments(STD), CHUNK_BLOCKS, EC32,
                                 want, CHUNK_IDS, VERSION, fmt=fmt)
    assert sorted(images) == sorted((s, p) for s in range(S)
                                    for p in want[s])
    for (s, p), img in images.items():
        assert np.array_equal(img.cpu().numpy(),
                              ref_image(EC32, s, p, fmt)), (s, p)
