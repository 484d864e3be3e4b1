"""What the engine carries from one call to the next: the per-stream scratch
of lizec_gpu.hip (pinned staging guarded by the `uploaded` event, device
pointer / table / index buffers that grow by free + malloc) and the Python
plan cache of lizardfs_amd.ec.  Everything is bit-exact against a CPU
reference; tests/KERNEL_COVERAGE.md, "State between calls", lists the cells.

A sequence runs on a fresh engine (scratch capacities last for an engine's
life) and on one torch stream.  Before its first call the stream gets a
spin kernel of about DELAY_MS (torch.cuda._sleep, calibrated once) and an
event right behind it; straight after the first call returns the event must
still be pending, so the first call's uploads sat unexecuted in the queue
while the second call's host code ran.  Nothing blocks between the first
and the last call; outputs are read back after the last one.

All outputs of a sequence lie in one buffer filled with 0xA5, every output
part between two 256-byte canaries; all inputs in one buffer of random
bytes.  Both whole buffers are compared at the end.

References: ref_encode / isal_tables / coef_matrices of test_gpu_ec_matrix.py
(checked there against the oracle) for the uniform and multi-table calls;
oracle.ec_encode_data over zero-padded sources, the reference of
test_gpu_ec_strided.py, test_gpu_ec_ragged.py and test_gpu_ec_view.py, for
those three entry points; oracle.crc32 / crc32_blocks and
scrub.build_chunk_image for CRCs and images; oracle.rs_encode / rs_recover
for the plan-cache tests.
"""
import contextlib
import ctypes
import threading

import numpy as np
import pytest

import oracle
from test_gpu_ec_matrix import coef_matrices, isal_tables, ref_encode

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
BLOCK = 65536
HDD_BLOCK = BLOCK + 4        # INTERLEAVED: 4-byte CRC, then the block
GUARD = 256
FILL = 0xA5
CLEAN = 0x7FFFFFFF
DELAY_MS = 50.0              # only has to outlast one call's host code

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def p8(a):
    return a.ctypes.data_as(u8p)


def p32(a):
    return None if a is None else a.ctypes.data_as(u32p)


def p64(a):
    return a.ctypes.data_as(u64p)


# ------------------------------------------------------------------ buffers

class Buf:
    """One host array and its device copy.  take()/take_many() hand out
    offsets, each region `phase` bytes past a 16-byte boundary and with
    `guard` bytes free on either side.  seed None: filled with FILL (an
    output buffer: after upload() the host side is turned into the expected
    image); else random bytes (inputs)."""

    def __init__(self, cap, seed=None):
        cap = (cap + 4 * GUARD + 15) // 16 * 16
        if seed is None:
            self.host = np.full(cap, FILL, np.uint8)
        else:
            self.host = np.random.default_rng(seed).integers(
                0, 256, cap, np.uint8)
        self.top = 0
        self.dev = None

    def take_many(self, count, n, guard=0, phase=0):
        slot = (n + 2 * guard + 15) // 16 * 16
        first = (self.top + 15) // 16 * 16 + (guard + 15) // 16 * 16 + phase
        self.top = first + (count - 1) * slot + n + guard
        assert self.top <= self.host.size, "Buf too small for this cell"
        return first + np.arange(count, dtype=np.int64) * slot

    def take(self, n, guard=0, phase=0):
        return int(self.take_many(1, n, guard, phase)[0])

    def upload(self):
        self.host = self.host[:(self.top + GUARD + 15) // 16 * 16]
        self.dev = torch.from_numpy(self.host).cuda()
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0
        return self

    def addr(self, offs):
        return np.uint64(self.base) + np.asarray(offs).astype(np.uint64)

    def view(self, off, n):
        return self.host[off:off + n]

    def check(self, what):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, self.host):
            bad = np.flatnonzero(got != self.host)
            pytest.fail(f"{what}: {bad.size} bytes differ, first offsets "
                        f"{bad[:6].tolist()} (got {got[bad[:6]].tolist()}, "
                        f"want {self.host[bad[:6]].tolist()})")


# --------------------------------------------------------- engine and delay

_cycles = None


def delay_cycles():
    """Spin cycles for about DELAY_MS, from one timed short spin."""
    global _cycles
    if _cycles is None:
        probe = 2_000_000
        torch.cuda._sleep(probe)          # first use loads the kernel
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        ms = max(e0.elapsed_time(e1), 0.2)   # bounds the delay at 250x probe
        _cycles = int(probe * DELAY_MS / ms)
    return _cycles


class Sequence:
    def __init__(self, lib, eng, stream):
        self.lib, self.eng, self.stream = lib, eng, stream
        self.sarg = ctypes.c_void_p(stream.cuda_stream)
        self.busy = None
        self.calls = 0

    def start(self):
        """The delay and the event behind it; every upload is over."""
        torch.cuda.synchronize()
        cycles = delay_cycles()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(cycles)
            self.busy = torch.cuda.Event()
            self.busy.record()

    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.eng, *args, self.sarg)
        assert rc == LIZEC_OK, f"{name} (call {self.calls}) returned {rc}"
        self.calls += 1
        if self.calls == 1 and self.busy is not None:
            assert not self.busy.query(), \
                f"the {DELAY_MS} ms delay ended before call 0 returned: " \
                f"the hand-over was not exercised; lengthen DELAY_MS"


@contextlib.contextmanager
def fresh_engine():
    from lizardfs_amd import lib as L
    lib = L.lib()
    eng = ctypes.c_void_p()
    assert lib.lizec_engine_create(ctypes.byref(eng), 0) == LIZEC_OK
    try:
        yield lib, eng
    finally:
        torch.cuda.synchronize()
        lib.lizec_engine_destroy(eng)


def run_sequence(ops, src_cap, out_cap, seed, what):
    """prepare() every op (regions, planted inputs), upload, enqueue every
    op's call behind the delay without blocking, then build the expected
    output image op by op and compare both buffers."""
    src, out = Buf(src_cap, seed), Buf(out_cap)
    for op in ops:
        op.prepare(src, out)
    src.upload()
    out.upload()
    with fresh_engine() as (lib, eng):
        seq = Sequence(lib, eng, torch.cuda.Stream())
        seq.start()
        for op in ops:
            op.run(seq, src, out)
        assert seq.calls == len(ops)
        seq.stream.synchronize()
        torch.cuda.synchronize()
        for op in ops:
            op.expect(src, out)
        out.check(f"{what}: outputs")
        src.check(f"{what}: inputs were modified")


def oracle_ec(coef, data):
    """oracle.ec_encode_data per stripe: data [S, srcs, L] -> [S, dests, L]."""
    dests, srcs = coef.shape
    tbl = oracle.init_tables(coef)
    exp = np.empty((data.shape[0], dests, data.shape[2]), np.uint8)
    for s in range(data.shape[0]):
        outs = [np.full(data.shape[2], 0x77, np.uint8) for _ in range(dests)]
        oracle.ec_encode_data(
            tbl, [np.ascontiguousarray(data[s, j]) for j in range(srcs)],
            outs)
        exp[s] = np.stack(outs)
    return exp


# ---------------------------------------------------------------------- ops

class Encode:
    """lizec_ec_encode_batch, or _multi when `index` is given.  perm: the
    order in which every stripe's sources are passed.  like: another Encode
    whose sources this one reads.  skip: (stripe, dest) passed as 0."""

    def __init__(self, srcs, dests, S, plen, coefs, perm=None, index=None,
                 skip=None, like=None):
        self.srcs, self.dests, self.S, self.plen = srcs, dests, S, plen
        self.coefs = [np.ascontiguousarray(c, np.uint8) for c in coefs]
        for c in self.coefs:
            assert c.shape == (dests, srcs)
        self.perm = np.arange(srcs) if perm is None else np.asarray(perm)
        self.index = None if index is None else \
            np.ascontiguousarray(index, np.uint32)
        self.skip, self.like = skip, like

    def prepare(self, src, out):
        if self.like is None:
            self.so = src.take_many(self.S * self.srcs, self.plen)
        else:
            assert (self.like.S, self.like.srcs, self.like.plen) == \
                (self.S, self.srcs, self.plen)
            self.so = self.like.so
        self.do = out.take_many(self.S * self.dests, self.plen, GUARD)

    def run(self, seq, src, out):
        so = self.so.reshape(self.S, self.srcs)[:, self.perm]
        sp = np.ascontiguousarray(src.addr(so).ravel())
        dp = np.ascontiguousarray(out.addr(self.do))
        assert not (sp % 16).any() and not (dp % 16).any()
        if self.skip is not None:
            dp[self.skip[0] * self.dests + self.skip[1]] = 0
        tbl = np.concatenate([isal_tables(c) for c in self.coefs])
        if self.index is None:
            seq.call("lizec_ec_encode_batch", self.plen, self.srcs,
                     self.dests, p8(tbl), p64(sp), p64(dp), self.S)
        else:
            seq.call("lizec_ec_encode_batch_multi", self.plen, self.srcs,
                     self.dests, p8(tbl), len(self.coefs), p32(self.index),
                     p64(sp), p64(dp), self.S)

    def expect(self, src, out):
        data = np.stack([src.view(o, self.plen) for o in self.so]).reshape(
            self.S, self.srcs, self.plen)[:, self.perm]
        index = np.zeros(self.S, np.uint32) if self.index is None \
            else self.index
        exp = np.empty((self.S, self.dests, self.plen), np.uint8)
        for t, coef in enumerate(self.coefs):
            sel = np.flatnonzero(index == t)
            if sel.size:
                exp[sel] = ref_encode(coef, data[sel])
        exp = exp.reshape(self.S * self.dests, self.plen)
        for i, o in enumerate(self.do):
            if self.skip is not None and \
                    i == self.skip[0] * self.dests + self.skip[1]:
                continue
            out.view(o, self.plen)[:] = exp[i]


class Strided:
    """lizec_ec_encode_batch_strided from contiguous aligned sources into
    INTERLEAVED-layout images: block b of a part at image + 4 + 65540*b.
    The images start at 0, 4, 8, 12 mod 16 in turn."""

    def __init__(self, nblocks, srcs, dests, S, coef):
        self.nb, self.srcs, self.dests, self.S = nblocks, srcs, dests, S
        self.coef = np.ascontiguousarray(coef, np.uint8)

    def prepare(self, src, out):
        self.so = src.take_many(self.S * self.srcs, self.nb * BLOCK)
        self.img = np.array([out.take(self.nb * HDD_BLOCK, GUARD,
                                      phase=(4 * i) % 16)
                             for i in range(self.S * self.dests)], np.int64)

    def run(self, seq, src, out):
        sp = np.ascontiguousarray(src.addr(self.so))
        dp = np.ascontiguousarray(out.addr(self.img + 4))
        tbl = isal_tables(self.coef)
        seq.call("lizec_ec_encode_batch_strided", self.nb, self.srcs,
                 self.dests, p8(tbl), p64(sp), p64(dp), self.S, BLOCK,
                 HDD_BLOCK)

    def blocks(self, src):
        """Reference parts [S*dests, nb, BLOCK]."""
        data = np.stack([src.view(o, self.nb * BLOCK) for o in self.so])
        data = data.reshape(self.S, self.srcs, self.nb * BLOCK)
        return oracle_ec(self.coef, data).reshape(self.S * self.dests,
                                                  self.nb, BLOCK)

    def expect(self, src, out):
        for i, blocks in enumerate(self.blocks(src)):
            for b in range(self.nb):
                out.view(self.img[i] + 4 + b * HDD_BLOCK, BLOCK)[:] = \
                    blocks[b]


class Fill:
    """lizec_crc_fill_batch_strided over the images a Strided op wrote."""

    def __init__(self, strided):
        self.st = strided

    def prepare(self, src, out):
        pass

    def run(self, seq, src, out):
        n = self.st.img.size
        dptrs = np.ascontiguousarray(out.addr(self.st.img))
        doffs = np.full(n, 4, np.uint32)
        coffs = np.zeros(n, np.uint32)
        counts = np.full(n, self.st.nb, np.uint32)
        seq.call("lizec_crc_fill_batch_strided", p64(dptrs), p32(doffs),
                 p32(coffs), p32(counts), n, HDD_BLOCK, HDD_BLOCK)

    def expect(self, src, out):
        from lizardfs_amd import scrub
        for i, blocks in enumerate(self.st.blocks(src)):
            img = scrub.build_chunk_image(1, 1, 0, 0, list(blocks),
                                          crc32_fn=oracle.crc32,
                                          fmt="interleaved")
            for b in range(self.st.nb):
                stored = int.from_bytes(img[b * HDD_BLOCK:][:4].tobytes(),
                                        "big")
                assert stored == oracle.crc32(blocks[b].tobytes())
            out.view(self.st.img[i], img.size)[:] = img


class Scrub:
    """lizec_scrub_batch_strided over INTERLEAVED images planted among the
    inputs.  real: {image index: (blocks, damage)}, damage None, ("data",
    block, byte) or ("crc", block, byte).  Every other of the `total`
    images has no blocks and shares the first real image's address."""

    def __init__(self, real, total=None, seed=0):
        self.real = dict(real)
        self.total = len(self.real) if total is None else total
        self.seed = seed

    def prepare(self, src, out):
        from lizardfs_amd import scrub
        rng = np.random.default_rng(self.seed)
        self.at, self.want = {}, {}
        for k, (i, (nb, damage)) in enumerate(sorted(self.real.items())):
            blocks = [rng.integers(0, 256, BLOCK, np.uint8)
                      for _ in range(nb)]
            img = scrub.build_chunk_image(1, 1, 0, 0, blocks,
                                          crc32_fn=oracle.crc32,
                                          fmt="interleaved")
            self.want[i] = CLEAN
            if damage is not None:
                kind, b, byte = damage
                img[b * HDD_BLOCK + (4 if kind == "data" else 0) + byte] ^= \
                    0x40
                self.want[i] = b
            self.at[i] = src.take(img.size, phase=(0, 4, 12)[k % 3])
            src.view(self.at[i], img.size)[:] = img
        self.status = out.take(4 * self.total, GUARD)

    def run(self, seq, src, out):
        n = self.total
        shared = src.addr(self.at[min(self.at)])
        dptrs = np.full(n, shared, np.uint64)
        counts = np.zeros(n, np.uint32)
        for i, off in self.at.items():
            dptrs[i] = src.addr(off)
            counts[i] = self.real[i][0]
        doffs = np.full(n, 4, np.uint32)
        coffs = np.zeros(n, np.uint32)
        seq.call("lizec_scrub_batch_strided", p64(dptrs), p32(doffs),
                 p32(coffs), p32(counts), n, HDD_BLOCK, HDD_BLOCK,
                 ctypes.c_void_p(int(out.addr(self.status))))

    def expect(self, src, out):
        st = np.full(self.total, CLEAN, np.int32)
        for i, v in self.want.items():
            st[i] = v
        out.view(self.status, 4 * self.total)[:] = st.view(np.uint8)


class Ragged:
    """lizec_ec_encode_batch_ragged, both strides 65536, all aligned.
    src_nb [S, srcs], dst_nb [S, dests]; NB blocks are laid out for every
    part that has any.  pool: sources are not per (stripe, part) but alias
    `pool` regions of NB blocks, in turn."""

    def __init__(self, srcs, dests, coefs, index, src_nb, dst_nb, NB,
                 pool=None):
        self.srcs, self.dests, self.NB, self.pool = srcs, dests, NB, pool
        self.coefs = [np.ascontiguousarray(c, np.uint8) for c in coefs]
        self.index = np.ascontiguousarray(index, np.uint32)
        self.src_nb = np.ascontiguousarray(src_nb, np.uint32)
        self.dst_nb = np.ascontiguousarray(dst_nb, np.uint32)
        self.S = self.index.size
        assert self.src_nb.shape == (self.S, srcs)
        assert self.dst_nb.shape == (self.S, dests)
        assert self.src_nb.max() <= NB and self.dst_nb.max() <= NB

    def prepare(self, src, out):
        n = self.S * self.srcs
        if self.pool is None:
            self.so = src.take_many(n, self.NB * BLOCK)
        else:
            regions = src.take_many(self.pool, self.NB * BLOCK)
            self.so = regions[np.arange(n) % self.pool]
        self.do = np.zeros(self.S * self.dests, np.int64)
        for i in np.flatnonzero(self.dst_nb.ravel()):
            self.do[i] = out.take(self.NB * BLOCK, GUARD)

    def run(self, seq, src, out):
        sp = np.ascontiguousarray(src.addr(self.so))
        dp = np.where(self.dst_nb.ravel() > 0, out.addr(self.do),
                      np.uint64(0))
        dp = np.ascontiguousarray(dp, np.uint64)
        tbl = np.concatenate([isal_tables(c) for c in self.coefs])
        seq.call("lizec_ec_encode_batch_ragged", self.srcs, self.dests,
                 p8(tbl), len(self.coefs), p32(self.index), p64(sp),
                 p32(self.src_nb), p64(dp), p32(self.dst_nb), self.S, BLOCK,
                 BLOCK)

    def expect(self, src, out):
        so = self.so.reshape(self.S, self.srcs)
        for s in np.flatnonzero(self.dst_nb.any(axis=1)):
            data = np.zeros((1, self.srcs, self.NB * BLOCK), np.uint8)
            for j in range(self.srcs):
                n = int(self.src_nb[s, j]) * BLOCK
                data[0, j, :n] = src.view(so[s, j], n)
            exp = oracle_ec(self.coefs[self.index[s]], data)[0]
            for l in range(self.dests):
                n = int(self.dst_nb[s, l]) * BLOCK
                out.view(self.do[s * self.dests + l], n)[:] = exp[l, :n]


class View:
    """lizec_ec_encode_batch_view, one chunk of n blocks held in ks view
    parts (chunk block c is block c // ks of part c % ks), cut into rows of
    rc = srcs columns from column 0: a parity target."""

    def __init__(self, srcs, dests, ks, n, coef):
        self.srcs, self.dests, self.ks, self.n = srcs, dests, ks, n
        self.coef = np.ascontiguousarray(coef, np.uint8)
        self.vb = -(-n // ks)             # blocks laid out per view part
        self.rows = -(-n // srcs)

    def prepare(self, src, out):
        self.vo = src.take_many(self.ks, self.vb * BLOCK)
        self.do = out.take_many(self.dests, self.rows * BLOCK, GUARD)

    def run(self, seq, src, out):
        vp = np.ascontiguousarray(src.addr(self.vo))
        dp = np.ascontiguousarray(out.addr(self.do))
        tbl = isal_tables(self.coef)
        chunk_nb = np.array([self.n], np.uint32)
        dst_nb = np.full(self.dests, self.rows, np.uint32)
        seq.call("lizec_ec_encode_batch_view", self.srcs, self.dests,
                 p8(tbl), 1, None, p64(vp), self.ks, p32(chunk_nb),
                 self.srcs, None, p64(dp), p32(dst_nb), 1, BLOCK, BLOCK)

    def expect(self, src, out):
        chunk = np.zeros((self.rows * self.srcs, BLOCK), np.uint8)
        for c in range(self.n):
            chunk[c] = src.view(self.vo[c % self.ks] + (c // self.ks) * BLOCK,
                                BLOCK)
        rows = chunk.reshape(self.rows, self.srcs, BLOCK)
        data = np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(
            1, self.srcs, self.rows * BLOCK)
        exp = oracle_ec(self.coef, data)[0]
        for l in range(self.dests):
            out.view(self.do[l], self.rows * BLOCK)[:] = exp[l]


class Crc:
    """lizec_crc32_batch over nblocks blocks of block_len bytes."""

    def __init__(self, nblocks, block_len):
        self.nblocks, self.block_len = nblocks, block_len

    def prepare(self, src, out):
        self.so = src.take(self.nblocks * self.block_len)
        self.do = out.take(4 * self.nblocks, GUARD)

    def run(self, seq, src, out):
        seq.call("lizec_crc32_batch",
                 ctypes.c_void_p(int(src.addr(self.so))), self.block_len,
                 self.nblocks, 0, ctypes.c_void_p(int(out.addr(self.do))))

    def expect(self, src, out):
        buf = np.ascontiguousarray(
            src.view(self.so, self.nblocks * self.block_len))
        crcs = oracle.crc32_blocks(buf, self.block_len)
        out.view(self.do, 4 * self.nblocks)[:] = \
            crcs.astype("<u4").view(np.uint8)


def four_matrices(dests, srcs, seed):
    """Four coefficient matrices from coef_matrices whose first rows all
    differ (and are not zero)."""
    mats = []
    for i in range(8):
        for c in coef_matrices(dests, srcs, seed + i, rot=i % 5):
            if c[0].any() and not any(np.array_equal(c[0], o[0])
                                      for o in mats):
                mats.append(c)
    assert len(mats) >= 4
    return mats[:4]


# ------------------------------------------------------------------ 1a, 1b

def test_handoff_single_table():
    """Four lizec_ec_encode_batch calls of one shape behind the delay, each
    with its own matrix, source order and output parts.  All pointer arrays
    have the same length and point into the same two buffers."""
    srcs, dests, S, plen = 3, 2, 3, 4096 + 16
    mats = four_matrices(dests, srcs, 41)
    perms = ([0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0])
    ops = [Encode(srcs, dests, S, plen, [mats[0]], perms[0])]
    for i in range(1, 4):
        ops.append(Encode(srcs, dests, S, plen, [mats[i]], perms[i],
                          like=ops[0]))
    run_sequence(ops, S * srcs * plen, 4 * S * dests * (plen + 2 * GUARD),
                 seed=410, what="handoff_single_table")


def test_handoff_across_entry_points():
    """Nine calls through every entry point that uses the stream's scratch
    (and lizec_crc32_batch, which uses none), unsynchronised."""
    srcs, dests, S, plen = 3, 2, 3, 4096 + 16
    m = four_matrices(dests, srcs, 52)
    strided = Strided(2, srcs, dests, 2, m[2])
    ops = [
        Encode(srcs, dests, S, plen, [m[0]], [1, 0, 2]),
        Encode(srcs, dests, S, plen, [m[1], m[2]], [2, 1, 0],
               index=[0, 1, 0], skip=(1, 1)),
        strided,
        Scrub({0: (2, None), 1: (3, ("data", 2, 100)),
               2: (2, ("crc", 0, 3))}, seed=53),
        Ragged(srcs, dests, [m[3], m[0]], [1, 0],
               src_nb=[[2, 2, 1], [1, 1, 1]], dst_nb=[[2, 2], [1, 1]], NB=2),
        Fill(strided),
        View(srcs, dests, ks=2, n=4, coef=m[1]),
        Crc(8, 8192),
        Encode(srcs, dests, S, plen, [m[3]], [0, 2, 1]),
    ]
    run_sequence(ops, 4 * 1024 * 1024, 2 * 1024 * 1024, seed=520,
                 what="handoff_across_entry_points")


# ----------------------------------------------------------------------- 1c

def small_encode(seed, multi=False):
    srcs, dests, S = 3, 2, 3
    m = four_matrices(dests, srcs, seed)
    if multi:
        return Encode(srcs, dests, S, 16, [m[0], m[1]], index=[1, 0, 1])
    return Encode(srcs, dests, S, 16, [m[0]])


def small_ragged(seed):
    m = four_matrices(1, 2, seed)
    return Ragged(2, 1, [m[0], m[1]], [1, 0], src_nb=[[1, 1], [1, 1]],
                  dst_nb=[[1], [1]], NB=1)


def growth_ptrs():
    """6 + 2 pointers for each of 16,400 stripes: 131,200 slots > 65,536,
    1,049,600 bytes of them > 1 MiB - 32 KiB of staging."""
    coef = np.random.default_rng(61).integers(0, 256, (2, 6), np.uint8)
    return (small_encode(610), Encode(6, 2, 16400, 16, [coef]),
            small_encode(620))


def growth_mtbls():
    """65 tables of 8 x 8 coefficients: 133,120 bytes > 64 KiB of d_mtbls,
    and with 65 index entries > 128 KiB of h_mstaging."""
    rng = np.random.default_rng(62)
    coefs = [rng.integers(0, 256, (8, 8), np.uint8) for _ in range(65)]
    index = rng.permutation(65)
    return (small_encode(630, multi=True),
            Encode(8, 8, 65, 16, coefs, index=index),
            small_encode(640, multi=True))


def growth_mindex():
    """16,385 stripes > 16,384 index entries; 49,155 pointers stay below
    the pointer array's 65,536."""
    rng = np.random.default_rng(63)
    coefs = [rng.integers(0, 256, (1, 2), np.uint8) for _ in range(2)]
    index = rng.integers(0, 2, 16385)
    return (small_encode(650, multi=True),
            Encode(2, 1, 16385, 16, coefs, index=index),
            small_encode(660, multi=True))


def growth_ragged():
    """8,200 stripes of 2 sources and 1 destination: 4 + 8 + 4 bytes of
    index and counts each, 131,200 bytes > 128 KiB before tables and map.
    Three stripes have destination blocks; the sources of all alias four
    pool regions of two blocks."""
    S = 8200
    rng = np.random.default_rng(64)
    coefs = [rng.integers(0, 256, (1, 2), np.uint8) for _ in range(2)]
    index = rng.integers(0, 2, S)
    src_nb = np.ones((S, 2), np.uint32)
    dst_nb = np.zeros((S, 1), np.uint32)
    src_nb[0], dst_nb[0] = (2, 1), 2
    src_nb[4100], dst_nb[4100] = (1, 1), 1
    src_nb[S - 1], dst_nb[S - 1] = (1, 2), 2
    return (small_ragged(670),
            Ragged(2, 1, coefs, index, src_nb, dst_nb, NB=2, pool=4),
            small_ragged(680))


def growth_scrub():
    """65,537 images: 2.5 slots each, 163,851 slots > 65,536.  Three have
    blocks; the others have none and share an address."""
    return (Scrub({0: (1, None), 1: (2, ("data", 1, 0)),
                   2: (1, ("crc", 0, 0))}, seed=690),
            Scrub({0: (2, ("data", 1, 65535)), 30000: (3, None),
                   65536: (2, ("crc", 0, 2))}, total=65537, seed=691),
            Scrub({0: (1, ("data", 0, 7)), 1: (1, None),
                   2: (2, ("crc", 1, 1))}, seed=692))


GROWTH = {"d_ptrs+h_staging": growth_ptrs, "d_mtbls+h_mstaging": growth_mtbls,
          "d_mindex": growth_mindex, "d_ragged": growth_ragged,
          "d_ptrs-via-scrub": growth_scrub}


@pytest.mark.parametrize("buffer", tuple(GROWTH))
def test_scratch_growth(buffer):
    """A small call behind the delay, then unsynchronised a call just large
    enough to make the named buffer grow, then a small call with new
    tables; all three are compared."""
    run_sequence(list(GROWTH[buffer]()), 3 * 1024 * 1024, 20 * 1024 * 1024,
                 seed=len(buffer), what=f"scratch_growth[{buffer}]")


# ----------------------------------------------------------------------- 1d

def test_two_streams_distinct_tables():
    """Two threads, each with its own stream, matrix and shape, on one
    engine; 10 unsynchronised calls each, every call with its own source
    order and output parts.  Expected values from ref_encode."""
    iters, S, plen = 10, 8, 4096
    shapes = ((3, 2, 71), (4, 3, 72))
    work = []
    for srcs, dests, seed in shapes:
        coef = four_matrices(dests, srcs, seed)[0]
        src = Buf(S * srcs * plen, seed)
        out = Buf(iters * S * dests * (plen + 2 * GUARD))
        ops = [Encode(srcs, dests, S, plen, [coef],
                      np.roll(np.arange(srcs), it)) for it in range(iters)]
        for it, op in enumerate(ops):
            if it:
                op.like = ops[0]
            op.prepare(src, out)
        work.append((src.upload(), out.upload(), ops))
    torch.cuda.synchronize()
    errors = []
    barrier = threading.Barrier(len(work))
    with fresh_engine() as (lib, eng):
        def worker(t):
            try:
                src, out, ops = work[t]
                seq = Sequence(lib, eng, torch.cuda.Stream())
                barrier.wait()
                for op in ops:
                    op.run(seq, src, out)
                seq.stream.synchronize()
            except BaseException as exc:
                errors.append((t, repr(exc)))

        threads = [threading.Thread(target=worker, args=(t,))
                   for t in range(len(work))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
    assert not errors, errors
    for t, (src, out, ops) in enumerate(work):
        for op in ops:
            op.expect(src, out)
        out.check(f"thread {t}: outputs")
        src.check(f"thread {t}: inputs were modified")


# ----------------------------------------------------------- 2: plan cache

def test_recover_plan_key_includes_row_strides():
    """Finding A.  Two recover_batch calls with the same `out`, whose
    fragment views share base addresses and differ in row stride:
    X[:, 0, :] of a [S, 2, L] tensor names rows 0, 2, 4 of X.view(2*S, L),
    X.view(2*S, L)[:S] rows 0, 1, 2.  With the strides missing from the
    "rec" key the second call ran the first call's plan."""
    from lizardfs_amd.ec import ReedSolomon
    k, m, S, L = 4, 2, 3, 4096
    erased = (1, 5)
    rs = ReedSolomon(k, m)
    rng = np.random.default_rng(81)
    X = {i: rng.integers(0, 256, (S, 2, L), np.uint8)
         for i in range(k + m) if i not in erased}
    dX = {i: torch.from_numpy(x).cuda() for i, x in X.items()}
    outs = {i: torch.full((S, L), FILL, dtype=torch.uint8, device="cuda")
            for i in erased}
    views = (lambda t: t[:, 0, :], lambda t: t.view(2 * S, L)[:S])
    named = (lambda x: x[:, 0, :], lambda x: x.reshape(2 * S, L)[:S])
    got = []
    for v in views:
        frags = [v(dX[i]) if i in dX else None for i in range(k + m)]
        rs.recover_batch(frags, erased, out=outs)
        got.append({i: outs[i].clone() for i in erased})
    a, b = (views[0](dX[0]), views[1](dX[0]))
    assert a.data_ptr() == b.data_ptr() and a.stride(0) != b.stride(0)
    torch.cuda.synchronize()
    emask = sum(1 << i for i in erased)
    for call, rows in enumerate(named):
        for s in range(S):
            frags = [np.ascontiguousarray(rows(X[i])[s]) if i in X else None
                     for i in range(k + m)]
            exp = oracle.rs_recover(k, m, frags, emask, set(erased), L)
            for i in erased:
                assert np.array_equal(got[call][i][s].cpu().numpy(), exp[i]), \
                    f"call {call}, stripe {s}, part {i}"


def test_plan_eviction_keeps_results_right():
    """70 cached encode plans through a cache of 64, enqueued without a
    sync: the oldest plans are destroyed while later ones may still run.
    Every output is compared, then the evicted key 0 is run again."""
    from lizardfs_amd import ec
    k, m, L, N = 8, 2, 1024, 70
    rs = ec.ReedSolomon(k, m)
    data_np = np.random.default_rng(82).integers(0, 256, (N, 1, k, L),
                                                 np.uint8)
    data = torch.from_numpy(data_np).cuda()
    par = torch.full((N, 1, m, L), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i in range(N):
        rs.encode_batch(data[i], parity=par[i])
        assert len(rs._plans) <= 64
    torch.cuda.synchronize()
    got = par.cpu().numpy()
    exp = [oracle.rs_encode(k, m, list(data_np[i, 0]), L) for i in range(N)]
    for i in range(N):
        assert np.array_equal(got[i, 0], np.stack(exp[i])), f"input {i}"
    key0 = ec.enc_plan_key(data[0].data_ptr(), par[0].data_ptr(), 1, L)
    keyN = ec.enc_plan_key(data[N - 1].data_ptr(), par[N - 1].data_ptr(), 1,
                           L)
    assert key0 not in rs._plans and keyN in rs._plans
    par[0].fill_(FILL)
    rs.encode_batch(data[0], parity=par[0])
    assert key0 in rs._plans and len(rs._plans) <= 64
    torch.cuda.synchronize()
    assert np.array_equal(par[0, 0].cpu().numpy(), np.stack(exp[0]))
    assert np.array_equal(data.cpu().numpy(), data_np)


def test_single_and_multi_table_plans_interleaved():
    """A cached single-table plan (encode_batch with parity=) and a cached
    multi-table plan (recover_batch_mixed with out=) run alternately, three
    times each, without a sync."""
    from lizardfs_amd.ec import ReedSolomon
    k, m, S, L = 4, 2, 4, 4096
    rs = ReedSolomon(k, m)
    rng = np.random.default_rng(83)
    data_np = rng.integers(0, 256, (S, k, L), np.uint8)
    parts = np.empty((S, k + m, L), np.uint8)
    parts[:, :k] = data_np
    for s in range(S):
        parts[s, k:] = np.stack(oracle.rs_encode(k, m, list(data_np[s]), L))
    erased = [(0, 1), (2, 5), (4, 5), (1, 3)]
    poisoned = parts.copy()
    for s, e in enumerate(erased):
        poisoned[s, list(e)] ^= 0x5A       # erased rows must not be read
    frags = [torch.from_numpy(np.ascontiguousarray(poisoned[:, i])).cuda()
             for i in range(k + m)]
    data = torch.from_numpy(data_np).cuda()
    par = torch.full((S, m, L), FILL, dtype=torch.uint8, device="cuda")
    mixed = torch.full((S, m, L), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    slots = None
    for _ in range(3):
        rs.encode_batch(data, parity=par)
        _, slots = rs.recover_batch_mixed(frags, erased, out=mixed)
    assert len(rs._plans) == 2
    torch.cuda.synchronize()
    assert np.array_equal(par.cpu().numpy(), parts[:, k:])
    got = mixed.cpu().numpy()
    for s in range(S):
        assert sorted(slots[s]) == sorted(erased[s])
        for j, part in enumerate(slots[s]):
            assert np.array_equal(got[s, j], parts[s, part]), (s, j, part)
