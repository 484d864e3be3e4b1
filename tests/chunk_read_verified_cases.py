"""Shared by test_chunk_read_verified_host.py and
test_gpu_chunk_read_verified.py: the CRC side of a verified chunk read, on
top of chunk_read_cases.py (Slice, PartStore, Reads, chunk_blocks).

The CRCs come from oracle.crc32_blocks, big-endian, in one of two layouts:

  array   block data at stride 65536 (or any other), the CRCs of a part as an
          array at stride 4 in a second buffer of random bytes, with room for
          one CRC more than the store gives any part blocks; `odd` puts every
          array at an odd address
  inline  [4-byte CRC][block] at stride 65540, the CRC at data - 4: the body
          of an INTERLEAVED image, or a stream of whole-block READ_DATA
          packets

Whatever lies past a part's count, data and CRC alike, is random bytes: a
check of such a block would fail.

loads() is the rule that says which source blocks a read consumes, written
over chunk blocks rather than over the kernel's [lo, hi) columns.
"""
import numpy as np

import chunk_read_cases as C
import oracle

BLOCK = C.BLOCK
INLINE = BLOCK + 4


def crc_bytes(part):
    """part [count, BLOCK] -> uint8 [4 * count], the CRC of block b,
    big-endian, at 4 * b."""
    if part.shape[0] == 0:
        return np.zeros(0, np.uint8)
    crcs = oracle.crc32_blocks(np.ascontiguousarray(part).reshape(-1), BLOCK)
    return np.asarray(crcs).astype(">u4").view(np.uint8).copy()


class VerifiedStore:
    """A PartStore and the CRCs of its parts.  put() -> (data offset in
    .data, CRC offset in .crc); with the inline layout .crc is .data."""

    def __init__(self, nslots, room, layout="array", stride=None, phase=None,
                 seed=0, odd=False):
        assert layout in ("array", "inline")
        self.inline = layout == "inline"
        self.stride = stride or (INLINE if self.inline else BLOCK)
        assert self.stride >= (INLINE if self.inline else BLOCK)
        self.crc_stride = self.stride if self.inline else 4
        self.parts = C.PartStore(nslots, room, self.stride, phase, seed)
        self.data = self.parts.host
        self.room = room
        if self.inline:
            self.crc = self.data
        else:
            self.per = (4 * room + 4 + 15) // 16 * 16
            self.crc = np.random.default_rng(seed + 1000).integers(
                0, 256, 16 + nslots * self.per, np.uint8)
        self.odd, self.used = odd, 0

    def put(self, part):
        off = self.parts.put(part)
        crc = crc_bytes(part)
        if self.inline:
            at = off - 4
            for b in range(part.shape[0]):
                self.data[at + b * self.stride:at + b * self.stride + 4] = \
                    crc[4 * b:4 * b + 4]
        else:
            at = 16 + self.used * self.per + (1 if self.odd else 0)
            self.crc[at:at + crc.size] = crc
        self.used += 1
        return off, at


class VReads(C.Reads):
    """Reads plus, per slot, where its CRCs lie (None = not verified)."""

    def __init__(self, slice_, rows):
        super().__init__(slice_, rows)
        self.crc = []

    def add(self, src_offs, src_nb, col_map, first, count, expect, index=0,
            crc_offs=None):
        super().add(src_offs, src_nb, col_map, first, count, expect, index)
        self.crc.append(crc_offs or [None] * len(src_offs))
        assert len(self.crc[-1]) == len(src_offs)

    def crc_ptrs(self, crc_base):
        return np.array([[0 if o is None else crc_base + o for o in row]
                         for row in self.crc], np.uint64)


def loads(ks, col_map, src_nb, first, count, j, b):
    """Does a read of chunk blocks [first, first + count) load block b of
    source slot j?  It has to exist; row b has to hold a requested block;
    and either a lost column is requested there (every present slot is then
    read) or the column that slot j backs is."""
    if b >= src_nb[j]:
        return False
    cols = [c for c in range(ks) if first <= b * ks + c < first + count]
    if any(C.LOST <= col_map[c] < C.UNMAPPED for c in cols):
        return True
    return any(col_map[c] == j for c in cols)


def expected_mask(ks, col_map, src_nb, first, count, crc_offs, bad_blocks):
    """bad_blocks: (slot, block) pairs whose data or CRC is corrupt."""
    mask = 0
    for j, b in bad_blocks:
        if crc_offs[j] is not None and \
                loads(ks, col_map, src_nb, first, count, j, b):
            mask |= 1 << j
    return mask
