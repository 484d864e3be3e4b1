"""The read-gate test matrix and an independent restatement of hdd_read over
hdd_read_crc_and_block (hddspacemgr.cc:1525-1608, :1662-1727) — shared by
test_read_gate_host.py and test_gpu_read_gate.py.  Plain numpy and
zlib.crc32 (which is mycrc32); nothing here calls or imports the library.

A World is a set of part-file images, a list of requests over them and the
layout of their packets in one arena filled with 0xA5.  The layout depends
only on addresses mod 16, and images and arena are 16-byte aligned wherever
they live, so ONE expected arena per flag value serves the host twin and the
device call alike.
"""
import functools
import zlib

import numpy as np

BLOCK = 65536
HDD_BLOCK = BLOCK + 4                 # chunk.h:40 kHddBlockSize
OK, BAD_BLOCK = 0, 2
FILL = 0xA5
NBLOCKS = 3
FORMATS = ("moosefs", "interleaved")
EMPTY_BLOCK_CRC = zlib.crc32(bytes(BLOCK))            # emptyblockcrc

# (offset, size): whole block; single bytes at both ends; all but the last /
# first byte / both; no and one aligned 16-byte unit; one unit per lane, one
# less and one more; aligned KiB-sized reads
RANGES = ((0, 65536), (0, 1), (65535, 1), (0, 65535), (1, 65535), (1, 65534),
          (13, 17), (15, 33), (0, 1023), (0, 1024), (0, 1025), (7, 1024),
          (4096, 4096), (32768, 32768))


def layout(fmt):
    """(data_off, crc_off, block_stride, crc_stride) of an ec(3,2) part file:
    chunk.cc:126-188 (signature 1 KiB, CRC array of ceil(1024 / 3) entries,
    header rounded up to 4 KiB) and chunk.cc:191-209."""
    if fmt == "moosefs":
        header = -(-(1024 + 4 * -(-1024 // 3)) // 4096) * 4096
        return header, 1024, BLOCK, 4
    return 4, 0, HDD_BLOCK, HDD_BLOCK


def be32(v):
    return np.frombuffer(int(v).to_bytes(4, "big"), np.uint8)


def aligned(n, fill=0):
    """n bytes of `fill` at a 64-byte aligned address."""
    raw = np.empty(n + 64, np.uint8)
    at = -raw.ctypes.data % 64
    out = raw[at:at + n]
    out[:] = fill
    return out


def restate(block, stored, offset, size, sparse):
    """(status, packet) as the reference decides them.  block: the block's
    65536 bytes, or None for a block at or past the end of the chunk;
    stored: its 4 stored CRC bytes."""
    if block is None:                                          # :1535-1541
        return OK, np.concatenate([be32(zlib.crc32(bytes(size))),
                                   np.zeros(size, np.uint8)])
    data = block[offset:offset + size]
    if sparse and not np.any(stored):                          # :1571
        # never checked; recomputed for a block of zeros       # :1582-1586
        blockcrc = 0 if np.any(block) else EMPTY_BLOCK_CRC
    else:
        blockcrc = int.from_bytes(bytes(stored), "big")
        if blockcrc != zlib.crc32(block.tobytes()):            # :1552, :1591
            return BAD_BLOCK, np.concatenate([np.zeros(4, np.uint8), data])
    if size == BLOCK:                                          # :1711-1712
        return OK, np.concatenate([be32(blockcrc), data])
    return OK, np.concatenate([be32(zlib.crc32(data.tobytes())), data])  # :1718


class Req:
    """One request.  boff / soff: byte offsets of the block and of its
    stored CRC in image `img` (None: past the end of the chunk); d: the
    packet's placement, (out + 4 - block - offset) mod 16."""

    def __init__(self, name, img, boff, soff, offset, size, d):
        self.name, self.img, self.boff, self.soff = name, img, boff, soff
        self.offset, self.size, self.d = offset, size, d


class World:
    def __init__(self):
        self.images, self.fmts, self.reqs = [], [], []
        self.starts, self.arena_size = None, 0
        self._expect = {}

    def add_image(self, fmt, blocks, stored=None):
        """A part-file image of 64 KiB blocks; stored[b] overrides the CRC
        bytes of block b."""
        data_off, crc_off, bstride, cstride = layout(fmt)
        size = (len(blocks) * HDD_BLOCK if fmt == "interleaved"
                else data_off + len(blocks) * BLOCK)
        img = aligned(size)
        for b, blk in enumerate(blocks):
            img[data_off + b * bstride:data_off + b * bstride + BLOCK] = blk
            s = be32(zlib.crc32(blk.tobytes()))
            if stored is not None and stored[b] is not None:
                s = stored[b]
            img[crc_off + b * cstride:crc_off + b * cstride + 4] = s
        self.images.append(img)
        self.fmts.append(fmt)
        return len(self.images) - 1

    def read(self, name, img, b, offset, size, d):
        """A request for block index b of image img."""
        data_off, crc_off, bstride, cstride = layout(self.fmts[img])
        if b >= NBLOCKS:
            self.reqs.append(Req(name, img, None, None, offset, size, d))
        else:
            self.reqs.append(Req(name, img, data_off + b * bstride,
                                 crc_off + b * cstride, offset, size, d))

    def place(self):
        """Packets in request order, at least one byte apart, each at the
        first position that gives its placement."""
        at, starts = 1, []
        for r in self.reqs:
            src = (r.boff or 0) + r.offset
            at += (r.d - (at + 4 - src)) % 16
            starts.append(at)
            at += 4 + r.size + 1
        self.starts, self.arena_size = np.array(starts, np.int64), at + 16

    def expect(self, sparse):
        """(status, arena) for the whole request list, computed once."""
        if sparse not in self._expect:
            status = np.zeros(len(self.reqs), np.int32)
            arena = np.full(self.arena_size, FILL, np.uint8)
            for i, r in enumerate(self.reqs):
                if r.boff is None:
                    st, pkt = restate(None, None, r.offset, r.size, sparse)
                else:
                    img = self.images[r.img]
                    st, pkt = restate(img[r.boff:r.boff + BLOCK],
                                      img[r.soff:r.soff + 4], r.offset,
                                      r.size, sparse)
                status[i] = st
                arena[self.starts[i]:self.starts[i] + 4 + r.size] = pkt
            arena.setflags(write=False)
            status.setflags(write=False)
            self._expect[sparse] = (status, arena)
        return self._expect[sparse]

    def ops(self, dtype, image_addrs, arena_addr):
        """The op table over images and an arena at these addresses."""
        assert arena_addr % 16 == 0 and all(a % 16 == 0 for a in image_addrs)
        ops = np.zeros(len(self.reqs), dtype)
        for i, r in enumerate(self.reqs):
            if r.boff is not None:
                ops[i]["block"] = image_addrs[r.img] + r.boff
                ops[i]["stored"] = image_addrs[r.img] + r.soff
            ops[i]["out"] = arena_addr + int(self.starts[i])
            ops[i]["offset"], ops[i]["size"] = r.offset, r.size
        return ops

    def select(self, pred):
        return [i for i, r in enumerate(self.reqs) if pred(r)]


def first_mismatch(got, want, starts, reqs):
    """Which packet (or which gap) the first differing arena byte lies in."""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    at = int(bad[0])
    i = int(np.searchsorted(starts, at, side="right")) - 1
    if i >= 0 and at < starts[i] + 4 + reqs[i].size:
        return f"byte {at - int(starts[i])} of the packet of '{reqs[i].name}'" \
               f" is {got[at]:#04x}, expected {want[at]:#04x}"
    return f"byte {at} outside every packet (behind request {i}) is " \
           f"{got[at]:#04x}"


def _flip(img, at, bit=0x10):
    img[at] ^= bit


@functools.lru_cache(maxsize=None)
def world():
    rng = np.random.default_rng(77001)
    w = World()

    def rnd():
        return rng.integers(0, 256, BLOCK, np.uint8)

    # --- the sweep: every range at every placement, both formats; block
    #     data at 0 mod 16 (MooseFS) and 4, 8, 12 mod 16 (INTERLEAVED)
    for fmt in FORMATS:
        img = w.add_image(fmt, [rnd() for _ in range(NBLOCKS)])
        k = 0
        for offset, size in RANGES:
            for d in range(16):
                w.read(f"{fmt} sweep ({offset},{size}) d={d}", img,
                       k % NBLOCKS, offset, size, d)
                k += 1
        # --- past the end of the chunk: whole and partial, all three forms
        for offset, size, d in ((0, 65536, 0), (0, 65536, 5), (0, 65536, 8),
                                (100, 3001, 0), (100, 3001, 4), (7, 50, 11),
                                (65535, 1, 2), (3, 9, 0)):
            w.read(f"{fmt} past end ({offset},{size}) d={d}", img, NBLOCKS,
                   offset, size, d)

    # --- damage, one bit at a time, around a partial read in the middle of
    #     block 1; blocks 0 and 2 of the same image are read in the same call
    for fmt in FORMATS:
        data_off, crc_off, bstride, cstride = layout(fmt)
        for offset, size in ((4096, 4096), (12345, 6789)):
            end = offset + size
            for region, at in (("pre", offset - 1), ("range", offset + size // 2),
                               ("post", end), ("post-last", BLOCK - 1),
                               ("pre-first", 0), ("stored", None)):
                img = w.add_image(fmt, [rnd() for _ in range(NBLOCKS)])
                if at is None:
                    _flip(w.images[img], crc_off + cstride + 2)
                else:
                    _flip(w.images[img], data_off + bstride + at)
                d = (len(w.reqs) * 5) % 16
                w.read(f"{fmt} damage in {region}, read ({offset},{size})",
                       img, 1, offset, size, d)
                w.read(f"{fmt} damage in {region}, whole read", img, 1, 0,
                       BLOCK, (d + 4) % 16)
                w.read(f"{fmt} clean block 0 beside damage in {region}", img,
                       0, offset, size, (d + 1) % 16)
                w.read(f"{fmt} clean block 2 beside damage in {region}", img,
                       2, 0, BLOCK, 0)

    # --- the sparse rule: the flag is the call's, every case runs with both
    zero = np.zeros(BLOCK, np.uint8)
    zero4 = np.zeros(4, np.uint8)

    def one_set(at):
        b = zero.copy()
        b[at] = 1
        return b

    for fmt in FORMATS:
        a = w.add_image(fmt, [zero, one_set(5), one_set(4096 + 7)],
                        stored=[zero4, zero4, zero4])
        b = w.add_image(fmt, [one_set(65535), zero, zero],
                        stored=[zero4, None, be32(EMPTY_BLOCK_CRC ^ 1)])
        for img, blk, what in ((a, 0, "zero block, stored 0"),
                               (a, 1, "byte 5 set (pre), stored 0"),
                               (a, 2, "byte 4103 set (range), stored 0"),
                               (b, 0, "byte 65535 set (post), stored 0"),
                               (b, 1, "zero block, stored its CRC"),
                               (b, 2, "zero block, stored a wrong CRC")):
            d = (len(w.reqs) * 3) % 16
            w.read(f"{fmt} sparse: {what}, whole read", img, blk, 0, BLOCK, d)
            w.read(f"{fmt} sparse: {what}, read (4096,4096)", img, blk, 4096,
                   4096, (d + 7) % 16)

    # --- blocks that overlap each other, at any byte address, and repeat;
    #     their stored CRCs lie behind the data at odd addresses
    raw = aligned(BLOCK + 8192)
    raw[:BLOCK + 4200] = rng.integers(0, 256, BLOCK + 4200, np.uint8)
    w.images.append(raw)
    w.fmts.append("raw")
    for k, boff in enumerate((0, 1000, 1001, 4093, 1001, 15)):
        soff = BLOCK + 4200 + 5 * k + 1
        raw[soff:soff + 4] = be32(zlib.crc32(raw[boff:boff + BLOCK].tobytes()))
        for offset, size, d in ((0, BLOCK, k), (31, 4097, 4 * k + 3),
                                (65000, 536, 0)):
            w.reqs.append(Req(f"raw block at {boff}, read ({offset},{size})",
                              len(w.images) - 1, boff, soff, offset, size,
                              d % 16))
    w.place()
    for img in w.images:
        img.setflags(write=False)
    return w
