"""lizardfs_amd.convert without a GPU: the choice of a recovery method, the
view columns, the argument checks of convert_parts, and the numpy addressing
model that the GPU tests build their expected bytes with.

The recovery_method cases are derived by hand from
SliceRecoveryPlanner::prepare (slice_recovery_planner.h:85-117), whose
branches are, in order: the part's own slice can give the part
(SliceReadPlanner: the part itself, or enough parts to recover it); the part
is a data part and some slice can give the chunk blocks it consists of; the
part is a parity part and some slice can give the rows under it.
"""
import numpy as np
import pytest

from lizardfs_amd import convert
from lizardfs_amd import slice_traits as st

BLOCK = st.BLOCK_SIZE
STD = st.K_STANDARD
XOR2, XOR3 = st.K_XOR2, st.K_XOR2 + 1
EC32, EC82 = st.ec_slice_type(3, 2), st.ec_slice_type(8, 2)


# ---- the addressing model (also imported by test_gpu_convert.py) ----------

def view_address(c, ks):
    """Chunk block c of a chunk held over ks data parts: (view column,
    block in that part) — chunk_read_planner.h:44-45."""
    return c % ks, c // ks


def data_part_blocks(kt, d, n):
    """The chunk blocks that data part d of a slice of kt data parts holds,
    in order, for a chunk of n blocks (slice_recovery_planner.h:46-54)."""
    return list(range(d, n, kt))


def split_chunk(chunk, k):
    """chunk [n, BLOCK] -> its k data parts, part d as [blocks, BLOCK]."""
    n = chunk.shape[0]
    return [chunk[data_part_blocks(k, d, n)] for d in range(k)]


def assemble_chunk(parts, n):
    """The inverse of split_chunk, block by block through view_address."""
    ks = len(parts)
    chunk = np.empty((n, BLOCK), np.uint8)
    for c in range(n):
        p, b = view_address(c, ks)
        chunk[c] = parts[p][b]
    return chunk


def target_rows(chunk, kt):
    """chunk [n, BLOCK] zero-padded to whole rows: [rows, kt, BLOCK]."""
    n = chunk.shape[0]
    rows = -(-n // kt)
    padded = np.zeros((rows * kt, BLOCK), np.uint8)
    padded[:n] = chunk
    return padded.reshape(rows, kt, BLOCK)


def test_addressing_model_covers_every_block_once():
    for ks in range(1, 7):
        for kt in range(1, 7):
            for n in range(1, 41):
                # where the chunk lies in the source slice
                held = [view_address(c, ks) for c in range(n)]
                assert len(set(held)) == n
                for p in range(ks):
                    blocks = sorted(b for q, b in held if q == p)
                    assert blocks == list(range(len(blocks)))
                    assert len(blocks) == st.number_of_blocks(
                        st.ec_slice_type(max(ks, 2), 1), p, n) or ks == 1
                # what the target's data parts take from it
                taken = [c for d in range(kt)
                         for c in data_part_blocks(kt, d, n)]
                assert sorted(taken) == list(range(n))
                # the kernel's form of the same: row b, column d
                for d in range(kt):
                    cs = data_part_blocks(kt, d, n)
                    assert cs == [b * kt + d for b in range(len(cs))]
                    assert len(cs) == (n + kt - d - 1) // kt


def test_model_round_trip():
    rng = np.random.default_rng(5)
    chunk = rng.integers(0, 256, (7, BLOCK), np.uint8)
    for k in (1, 2, 3, 5):
        assert np.array_equal(assemble_chunk(split_chunk(chunk, k), 7), chunk)
    rows = target_rows(chunk, 3)
    assert rows.shape == (3, 3, BLOCK) and not rows[2, 1:].any()
    assert np.array_equal(rows[2, 0], chunk[6])


# ---- recovery_method -------------------------------------------------------

def test_read_from_the_same_slice_is_preferred():
    # the part itself is there
    assert convert.recovery_method(EC32, 1, [(STD, 0), (EC32, 1)]) == "read"
    # k = 3 other parts of the slice are: SliceReadPlanner recovers it
    avail = [(STD, 0), (EC32, 0), (EC32, 2), (EC32, 4)]
    assert convert.recovery_method(EC32, 1, avail) == "read"
    assert convert.recovery_method(EC32, 3, avail) == "read"
    # xor2: the parity (part 0) from both data parts
    assert convert.recovery_method(XOR2, 0, [(XOR2, 1), (XOR2, 2)]) == "read"


def test_data_target_from_a_standard_copy():
    assert convert.recovery_method(EC32, 1, [(STD, 0)]) == "data"
    assert convert.recovery_method(EC82, 7, [(EC82, 0), (STD, 0)]) == "data"
    # xor data parts are 1..N
    assert convert.recovery_method(XOR3, 2, [(STD, 0)]) == "data"
    # two of the three parts of the slice do not recover it, the ec(8,2)
    # slice is incomplete, the xor2 one is whole
    avail = [(EC32, 0), (EC32, 4), (EC82, 1), (XOR2, 1), (XOR2, 2)]
    assert convert.recovery_method(EC32, 1, avail) == "data"


def test_parity_target_from_a_xor_slice():
    assert convert.recovery_method(EC32, 3, [(XOR2, 1), (XOR2, 2)]) == "parity"
    # the xor slice is degraded but recoverable (2 of its 3 parts)
    assert convert.recovery_method(EC82, 9, [(XOR2, 0), (XOR2, 2)]) == "parity"
    assert convert.recovery_method(XOR3, 0, [(STD, 0)]) == "parity"
    assert convert.recovery_method(EC82, 8, [(EC32, 1), (EC32, 3),
                                             (EC32, 4)]) == "parity"


def test_nothing_readable():
    assert convert.recovery_method(EC32, 0, []) is None
    assert convert.recovery_method(EC32, 0, [(XOR3, 1), (XOR3, 2),
                                             (EC82, 0), (EC32, 4)]) is None
    assert convert.recovery_method(EC32, 4, [(XOR2, 1), (EC32, 0)]) is None
    with pytest.raises(ValueError):
        convert.recovery_method(EC32, 5, [(STD, 0)])
    with pytest.raises(ValueError):
        convert.recovery_method(st.K_TAPE, 0, [(STD, 0)])


def test_chunk_block_ranges():
    """slice_recovery_planner.h:99-115."""
    assert convert.chunk_block_range(EC82, 2, 3, 4) == (2 + 3 * 8, 1 + 3 * 8)
    assert convert.chunk_block_range(EC82, 8, 3, 4) == (3 * 8, 4 * 8)
    assert convert.chunk_block_range(XOR3, 2, 1, 2) == (1 + 3, 1 + 3)
    assert convert.chunk_block_range(XOR3, 0, 1, 2) == (3, 6)
    # one block of data part 0 of ec(3,2) is chunk block 0, which xor3 keeps
    # in its part 1 (chunk_read_planner.h:182-206); two blocks span a row
    assert convert.recovery_method(EC32, 0, [(XOR3, 1)], 0, 1) == "data"
    assert convert.recovery_method(EC32, 0, [(XOR3, 1)], 0, 2) is None
    assert convert.recovery_method(EC32, 1, [(XOR3, 1)], 0, 1) is None
    assert convert.recovery_method(EC32, 1, [(XOR3, 2)], 0, 1) == "data"


def test_view_columns():
    assert convert.view_columns(STD) == [0]
    assert convert.view_columns(XOR2) == [1, 2]
    assert convert.view_columns(st.K_XOR9) == list(range(1, 10))
    assert convert.view_columns(EC32) == [0, 1, 2]
    assert convert.view_columns(EC82) == list(range(8))
    with pytest.raises(ValueError):
        convert.view_columns(st.K_TAPE)


# ---- convert_parts refuses its arguments before it needs a GPU -------------

def test_argument_errors_need_no_gpu(monkeypatch):
    import torch
    from lizardfs_amd import lib as L

    def no_call(*a, **kw):
        raise AssertionError("the library was used")
    monkeypatch.setattr(L, "lib", no_call)
    monkeypatch.setattr(L, "engine", no_call)
    S = 3
    cb = [1, 4, 7]
    frag = torch.zeros((S, 3 * BLOCK), dtype=torch.uint8)     # not on a GPU
    f5 = [frag] * 5

    def refused(*a, **kw):
        with pytest.raises(ValueError):
            convert.convert_parts(*a, **kw)

    refused(st.K_TAPE, [frag], cb, EC82, {8})
    refused(EC32, f5, cb, st.K_TAPE, {0})
    refused(EC32, f5, [0, 4, 7], EC82, {8})
    refused(EC32, f5, [1, 4, 1025], EC82, {8})
    refused(EC32, f5, [cb], EC82, {8})
    refused(EC32, f5, [1.0, 4.0, 7.0], EC82, {8})
    refused(EC32, f5, [], EC82, {8})
    refused(EC32, f5[:4], cb, EC82, {8})                # k+m fragment slots
    refused(XOR2, [frag] * 2, cb, EC82, {8})            # N+1 of them
    refused(EC32, f5, cb, EC82, {10})                   # want within the slice
    refused(EC32, f5, cb, EC82, {-1})
    refused(EC32, f5, cb, EC82, set())
    refused(EC32, f5, cb, EC82, [set(), set(), set()])
    refused(EC32, f5, cb, EC82, [{8}, {9}])             # one set per chunk
    refused(EC32, f5, cb, EC82, {8}, src_stride=65538)
    refused(EC32, f5, cb, EC82, {8}, src_stride=65532)
    refused(EC32, f5, cb, EC82, {8}, dst_stride=65538)
    refused(EC32, f5, cb, EC82, {8}, dst_stride=65532)
    refused(EC32, f5, cb, EC82, {8}, dst_stride=65540)  # needs out
    # a degraded source: only an ec one is rebuilt first
    refused(XOR2, [frag] * 3, cb, EC82, {8}, src_erased={1})
    refused(STD, [frag], cb, EC82, {8}, src_erased={0})
    refused(XOR2, [frag, None, frag], cb, EC82, {8})
    refused(EC32, [frag, None, frag, frag, frag], cb, EC82, {8})
    refused(EC32, f5, cb, EC82, {8}, src_erased={0, 1, 2})      # > m
    refused(EC32, f5, cb, EC82, {8}, src_erased={5})
    refused(EC32, f5, cb, EC82, {8}, src_erased=[{0}, {1}])
    # erased {0}: padded with part 4, so part 3 must be there
    refused(EC32, [None, frag, frag, None, frag], cb, EC82, {8},
            src_erased={0})
    refused(EC32, [None] * 5, cb, EC82, {8}, src_erased={0})
    # and last of all the tensors themselves
    refused(EC32, f5, cb, EC82, {8})                    # not CUDA tensors
    refused(EC32, [np.zeros((S, BLOCK), np.uint8)] * 5, cb, EC82, {8})
