"""Host side of ragged EC batches (no GPU): lizec_ragged_block_map, and the
part geometry a ragged rebuild feeds it (slice_traits.number_of_blocks).

The block map has one (stripe, block) entry per 64 KiB block row of a batch:
stripe s contributes blocks 0 .. max_l dst_nblocks[s][l] - 1, stripe-major.
"""
import ctypes

import numpy as np
import pytest

from lizardfs_amd import lib as L
from lizardfs_amd import slice_traits as st

LIZEC_EINVAL = -2
u32p = ctypes.POINTER(ctypes.c_uint32)


def block_map(counts, cap=None, count_only=False):
    """counts [S, dests] -> (return value, map [cap, 2])."""
    counts = np.ascontiguousarray(counts, np.uint32)
    S, dests = counts.shape
    if count_only:
        return L.lib().lizec_ragged_block_map(
            counts.ctypes.data_as(u32p), dests, S, None, 0), None
    m = np.full((cap, 2), 0xDEADBEEF, np.uint32)
    r = L.lib().lizec_ragged_block_map(
        counts.ctypes.data_as(u32p), dests, S, m.ctypes.data_as(u32p), cap)
    return r, m


# a stripe with all-zero counts in the middle (2), and one whose destinations
# differ in length (4)
HAND = [[3, 3], [1, 1], [0, 0], [2, 2], [2, 3]]
HAND_MAP = [(0, 0), (0, 1), (0, 2), (1, 0), (3, 0), (3, 1),
            (4, 0), (4, 1), (4, 2)]


def test_hand_written_case():
    r, m = block_map(HAND, cap=12)
    assert r == len(HAND_MAP)
    assert [tuple(int(x) for x in e) for e in m[:r]] == HAND_MAP
    assert (m[r:] == 0xDEADBEEF).all(), "wrote past the entries"


def test_exact_capacity():
    r, m = block_map(HAND, cap=len(HAND_MAP))
    assert r == len(HAND_MAP)
    assert [tuple(int(x) for x in e) for e in m] == HAND_MAP


def test_null_map_counts_only():
    r, _ = block_map(HAND, count_only=True)
    assert r == len(HAND_MAP)
    r, _ = block_map([[0, 0, 0]], count_only=True)
    assert r == 0


def test_capacity_too_small():
    r, m = block_map(HAND, cap=len(HAND_MAP) - 1)
    assert r == LIZEC_EINVAL
    assert (m == 0xDEADBEEF).all(), "a refused call wrote the map"


def test_single_destination_and_many():
    r, m = block_map([[2], [0], [1]], cap=3)
    assert r == 3
    assert m.tolist() == [[0, 0], [0, 1], [2, 0]]
    counts = np.zeros((2, 32), np.uint32)
    counts[1, 31] = 2
    r, m = block_map(counts, cap=2)
    assert r == 2 and m.tolist() == [[1, 0], [1, 1]]


def test_bad_arguments():
    lib = L.lib()
    one = np.ones(4, np.uint32)
    p = one.ctypes.data_as(u32p)
    assert lib.lizec_ragged_block_map(None, 1, 1, None, 0) == LIZEC_EINVAL
    assert lib.lizec_ragged_block_map(p, 0, 1, None, 0) == LIZEC_EINVAL
    assert lib.lizec_ragged_block_map(p, 33, 1, None, 0) == LIZEC_EINVAL
    assert lib.lizec_ragged_block_map(p, 1, 0, None, 0) == LIZEC_EINVAL
    r, _ = block_map([[32768]], count_only=True)
    assert r == 32768
    r, _ = block_map([[32769]], count_only=True)
    assert r == LIZEC_EINVAL


def test_tile_overflow_refused():
    """8192 stripes of 32768 blocks are 2^28 block rows: counted in 8 KiB
    tiles, one workgroup each, that is 2^31 > 2^31 - 1.  One block less
    fits."""
    counts = np.full((8192, 1), 32768, np.uint32)
    r, _ = block_map(counts, count_only=True)
    assert r == LIZEC_EINVAL
    counts[-1, 0] -= 1
    r, _ = block_map(counts, count_only=True)
    assert r == 8192 * 32768 - 1


@pytest.mark.parametrize("chunk_blocks", list(range(1, 14)) + [1023, 1024])
def test_number_of_blocks_ec32(chunk_blocks):
    """ec(3,2): the data parts share out the chunk's blocks round-robin
    (slice_traits.h:311-316) and every parity part is as long as part 0."""
    t = st.ec_slice_type(3, 2)
    data = [st.number_of_blocks(t, p, chunk_blocks) for p in range(3)]
    assert sum(data) == chunk_blocks
    assert data == sorted(data, reverse=True)
    assert data[0] - data[2] <= 1
    for p in (3, 4):
        assert st.number_of_blocks(t, p, chunk_blocks) == data[0]
    # block b of the chunk is block b // 3 of part b % 3
    assert data == [len(range(p, chunk_blocks, 3)) for p in range(3)]
