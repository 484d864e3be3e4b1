"""The write-gate test matrix and a Python restatement of hdd_write's checks
(hddspacemgr.cc:1918-2001) on the oracle — shared by test_write_gate_host.py
and test_gpu_write_gate.py.  Nothing here calls liblizec."""
import zlib

import numpy as np

import oracle

BLOCK = 65536
OK, BAD_DATA, BAD_BLOCK = 0, 1, 2

# (offset, size): whole block, empty writes, single bytes at both ends,
# ranges that start or end the block, aligned and odd middles
PAIRS = ((0, 65536), (0, 0), (0, 1), (0, 65535),
         (1, 65535), (1, 1), (33, 0), (65535, 0), (65535, 1),
         (4096, 4096), (12345, 6789), (65520, 16))


def crc(data):
    """CRC of bytes by both references, which must agree."""
    b = bytes(data)
    c = oracle.crc32(b)
    assert c == zlib.crc32(b), "the two references disagree"
    return c


def zeroblock(n):
    """mycrc32_zeroblock(0, n), crc.h:27."""
    return oracle.crc32_combine(0 ^ 0xFFFFFFFF, 0xFFFFFFFF, n)


EMPTY_BLOCK_CRC = zeroblock(BLOCK)


def splice(pre, offset, c, size, post):
    """hddspacemgr.cc:1954-1962 / :1992-1999."""
    rest = BLOCK - (offset + size)
    if offset == 0:
        return oracle.crc32_combine(c, post, rest)
    comb = oracle.crc32_combine(pre, c, size)
    if offset + size < BLOCK:
        comb = oracle.crc32_combine(comb, post, rest)
    return comb


def restate(offset, size, claimed, data, block, stored, sparse):
    """(status, newcrc) as hdd_write decides them.  data: the bytes to
    write; block: the block's current 65536 bytes or None (past the end of
    the chunk); stored: its 4 stored CRC bytes."""
    if claimed != crc(data):                                   # :1918
        return BAD_DATA, 0
    if offset == 0 and size == BLOCK:                          # :1922
        return OK, claimed
    end = offset + size
    if block is None:                                          # :1989-1990
        pre, post = zeroblock(offset), zeroblock(BLOCK - end)
    else:                                                      # :1951-1953
        pre = crc(block[:offset])
        post = crc(block[end:])
        have = splice(pre, offset, crc(block[offset:end]), size, post)
        st = int.from_bytes(bytes(stored), "big")
        if sparse and st == 0 and not np.any(block):           # crc.cc:235
            st = EMPTY_BLOCK_CRC
        if st != have:                                         # :1965
            return BAD_BLOCK, 0
    return OK, splice(pre, offset, claimed, size, post)


def spliced_crc(offset, size, data, block):
    """zlib's CRC of the block with the data written into it — the end
    state, computed without any combine algebra."""
    b = np.zeros(BLOCK, np.uint8) if block is None else np.array(block)
    b[offset:offset + size] = data
    return zlib.crc32(b.tobytes())


class Case:
    """One op of the matrix.  orig is the block the stored CRC was taken
    from (None: no block); block is what the block holds now (orig with at
    most one byte flipped); stored is None for "CRC of orig"."""

    def __init__(self, name, offset, size, data, claimed, orig, block,
                 stored=None):
        self.name, self.offset, self.size = name, offset, size
        self.data, self.claimed = data, claimed
        self.orig, self.block, self.stored = orig, block, stored
        self._expect = {}

    def stored_bytes(self):
        if self.stored is not None:
            return self.stored
        c = zlib.crc32(self.orig.tobytes()) if self.orig is not None else 0
        return np.frombuffer(c.to_bytes(4, "big"), np.uint8).copy()

    def expect(self, sparse):
        """restate() for this case, computed once per flag value."""
        if sparse not in self._expect:
            self._expect[sparse] = restate(
                self.offset, self.size, self.claimed, self.data, self.block,
                self.stored_bytes(), sparse)
        return self._expect[sparse]


def sweep_cases(seed=20240):
    """For every (offset, size): good data, a wrong claimed CRC, no block,
    and a flipped byte in each non-empty region of the block."""
    rng = np.random.default_rng(seed)
    cases = []
    for offset, size in PAIRS:
        tag = f"({offset},{size})"
        end = offset + size
        data = rng.integers(0, 256, size, np.uint8)
        good = crc(data)
        orig = rng.integers(0, 256, BLOCK, np.uint8)
        cases.append(Case(tag + " good", offset, size, data, good, orig, orig))
        cases.append(Case(tag + " wrong data crc", offset, size, data,
                          good ^ 0x00010000, orig, orig))
        cases.append(Case(tag + " no block", offset, size, data, good, None,
                          None))
        for region, lo, hi in (("pre", 0, offset), ("changed", offset, end),
                               ("post", end, BLOCK)):
            if lo == hi:
                continue
            # first, last or a middle byte of the region, by turns
            at = (lo, hi - 1, (lo + hi) // 2)[len(cases) % 3]
            bad = orig.copy()
            bad[at] ^= 0x40
            cases.append(Case(f"{tag} flipped byte {at} in {region}", offset,
                              size, data, good, orig, bad))
    return cases


def sparse_cases(seed=20241):
    """Zero or non-zero block x stored 0 or the empty-block CRC; the flag
    is the call's.  "Non-zero" is a single set byte, once in each region of
    the op, so an OR that misses a region lets the rule fire wrongly."""
    rng = np.random.default_rng(seed)
    offset, size = 4096, 4096
    data = rng.integers(0, 256, size, np.uint8)
    good = crc(data)
    zero4 = np.zeros(4, np.uint8)
    empty4 = np.frombuffer(EMPTY_BLOCK_CRC.to_bytes(4, "big"), np.uint8).copy()
    blocks = [("zero block", np.zeros(BLOCK, np.uint8))]
    for region, at in (("pre", 5), ("changed", 4096 + 7), ("post", 65535)):
        b = np.zeros(BLOCK, np.uint8)
        b[at] = 1
        blocks.append((f"block with byte {at} set ({region})", b))
    cases = []
    for bname, b in blocks:
        for sname, stored in (("stored 0", zero4), ("stored empty-block crc",
                                                    empty4)):
            cases.append(Case(f"sparse: {bname}, {sname}", offset, size, data,
                              good, b, b, stored))
    return cases
