#!/usr/bin/env python3
"""A/B of the ragged streaming rebuild (lizec_replicate_run_ragged) against
the uniform one (lizec_replicate_run), host to host, PCIe inclusive.

Both calls are synchronous, so a host clock around the call is the time of
the whole pipeline.  Buffers are pinned.  Every comparison runs a warm-up
pass and then PASSES timed passes in which the sides alternate, in one
process; each figure is reported as median [min, max] over the passes.

  A  48 full ec(8,2) chunks, one pattern: the new call against the uniform
     one, and the uniform one against itself (two alternating series), which
     is the spread a ratio has to be read against.
  B  256 ec(8,2) chunks, seeded: half 1024 blocks, a quarter uniform in
     1..1023, a quarter uniform in 1..16; the lost part uniform over the 10
     parts.  One new call against what a caller has to do without it: pad
     every part to ceil(n/k) blocks and run lizec_replicate_run once per
     (padded length, pattern) group.
  C  4096 one-block chunks: the API-overhead regime.
  D  population A with source verification on and off.

The sources are random bytes, not codewords: both calls compute the same
linear map over them, and what they emit is compared (B) or checked against
the host twin on a sample (A, C) outside the timed passes.

  python scripts/replicate_ragged_ab.py [--passes N] [--only ABCD]
      [--dump-json FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd import scrub, slice_traits as st  # noqa: E402
from lizardfs_amd.ec import _pattern_tables  # noqa: E402

K, M = 8, 2
NPARTS = K + M
BLOCK = st.BLOCK_SIZE
T = st.ec_slice_type(K, M)
HDR = scrub.header_size(T)
CRC_OFF = scrub.SIGNATURE_BLOCK
SIG_LEN = 22
GIB = float(1 << 30)

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "n": len(xs)}


def ratio_stats(num, den):
    """Per-pass ratios of two alternating series."""
    return stats([a / b for a, b in zip(num, den)])


def fmt_s(s, scale=1.0, unit="s"):
    return (f"{s['median'] * scale:.4g} {unit} "
            f"[{s['min'] * scale:.4g}, {s['max'] * scale:.4g}]")


class Population:
    """Chunks of given lengths, each missing one part: pinned, zero-padded
    source buffers (every part ceil(n/k) blocks long, so the same bytes
    serve the ragged and the uniform call) and pinned outputs for both."""

    def __init__(self, chunk_blocks, lost, seed, with_crcs=False):
        self.n = np.asarray(chunk_blocks, np.int64)
        self.S = S = self.n.size
        self.lost = np.asarray(lost, np.int64)
        # the second erased part pads the pattern to m parts and is not
        # rebuilt (ec_read_plan.h:126-133)
        pad = np.where(self.lost == NPARTS - 1, NPARTS - 2, NPARTS - 1)
        erased = np.sort(np.stack([self.lost, pad], axis=1), axis=1)
        self.tables, self.index, pslots, pemask = _pattern_tables(
            K, M, erased, self.lost[:, None])
        assert pslots.shape[1] == 1
        palive = np.array([[i for i in range(NPARTS) if not (int(e) >> i) & 1]
                           for e in pemask], np.intp)
        self.alive = palive[self.index]                         # [S, K]
        pb = np.array([[st.number_of_blocks(T, i, int(n))
                        for i in range(NPARTS)] for n in self.n], np.int64)
        self.src_nb = np.ascontiguousarray(
            np.take_along_axis(pb, self.alive, axis=1).astype(np.uint32))
        self.dst_nb = np.ascontiguousarray(
            pb[np.arange(S), self.lost].astype(np.uint32)[:, None])
        self.padded = (self.n + K - 1) // K                     # blocks
        plen = self.padded * BLOCK
        # sources: chunk after chunk, slot after slot, padded length each
        slot_len = np.repeat(plen[:, None], K, axis=1)
        self.src_off = np.concatenate(
            [[0], np.cumsum(slot_len.ravel())[:-1]]).reshape(S, K)
        self.src_arena = L.pinned_empty(max(int(slot_len.sum()), 1))
        rng = np.random.default_rng(seed)
        tile = rng.integers(0, 256, 1 << 24, np.uint8)
        a = self.src_arena
        for at in range(0, a.size, tile.size):
            a[at:at + tile.size] = tile[:a.size - at]
        for s in range(S):
            for j in range(K):
                lo = int(self.src_off[s, j]) + int(self.src_nb[s, j]) * BLOCK
                a[lo:int(self.src_off[s, j]) + int(slot_len[s, j])] = 0
        self.src = (a.ctypes.data + self.src_off).astype(np.uint64)
        # outputs: ragged images of their own size, uniform ones padded
        rsize = HDR + self.dst_nb[:, 0].astype(np.int64) * BLOCK
        usize = HDR + plen
        self.r_off = np.concatenate([[0], np.cumsum((rsize + 15) & ~15)[:-1]])
        self.u_off = np.concatenate([[0], np.cumsum(usize)[:-1]])
        self.r_size, self.u_size = rsize, usize
        self.r_out = L.pinned_empty(int(((rsize + 15) & ~15).sum()))
        self.u_out = L.pinned_empty(int(usize.sum()))
        self.r_dst = (self.r_out.ctypes.data + self.r_off).astype(
            np.uint64)[:, None]
        self.u_dst = (self.u_out.ctypes.data + self.u_off).astype(np.uint64)
        self.sigs = np.zeros((S, 1, SIG_LEN), np.uint8)
        for s in range(S):
            sig = scrub.build_signature(s + 1, 3, T, int(self.lost[s]))
            self.sigs[s, 0, :len(sig)] = np.frombuffer(sig, np.uint8)
        self.crcs = self.crc_ptrs = None
        if with_crcs:
            # one big-endian CRC per source block, as a part file holds them
            nb = self.src_nb.astype(np.int64)
            coff = np.concatenate([[0], np.cumsum(nb.ravel() * 4)[:-1]])
            self.crcs = np.zeros(int(nb.sum()) * 4, np.uint8)
            for i, (s, j) in enumerate(np.ndindex(S, K)):
                for b in range(int(nb[s, j])):
                    lo = int(self.src_off[s, j]) + b * BLOCK
                    c = zlib.crc32(a[lo:lo + BLOCK])
                    self.crcs[int(coff[i]) + 4 * b:int(coff[i]) + 4 * b + 4] = \
                        np.frombuffer(c.to_bytes(4, "big"), np.uint8)
            self.crc_ptrs = (self.crcs.ctypes.data + coff).astype(
                np.uint64).reshape(S, K)
        self.bad = np.zeros(S, np.uint32)
        # what each side moves over PCIe
        self.r_in = int(self.src_nb.astype(np.int64).sum()) * BLOCK
        self.r_outb = int(rsize.sum())
        self.u_in = int((plen * K).sum())
        self.u_outb = int(usize.sum())
        # uniform groups: (padded length, pattern)
        keys = self.padded * (int(self.index.max()) + 1) + self.index
        self.groups = [np.flatnonzero(keys == g) for g in np.unique(keys)]
        self._group_args = []
        for g in self.groups:
            self._group_args.append((
                int(plen[g[0]]), int(self.index[g[0]]),
                np.ascontiguousarray(self.src[g].ravel()),
                np.ascontiguousarray(self.sigs[g].ravel()),
                np.ascontiguousarray(self.u_dst[g]), int(g.size)))

    def copies_ragged(self, stages):
        """hipMemcpyAsync calls of one ragged run: sources and images with a
        block or a header, and metadata (and masks) per stage."""
        n = int(np.count_nonzero(self.src_nb)) + self.S
        return n + stages * (2 if self.crc_ptrs is not None else 1)

    def stages(self, stage_bytes=0):
        return int(L.lib().lizec_replicate_ragged_stages(
            K, 1, self.src_nb.ctypes.data_as(u32p),
            self.r_dst.ctypes.data_as(u64p), self.dst_nb.ctypes.data_as(u32p),
            self.S, HDR, 0, stage_bytes, None, 0))

    def run_ragged(self, verify=False):
        crc = self.crc_ptrs.ctypes.data_as(u64p) if verify else None
        bad = self.bad.ctypes.data_as(u32p) if verify else None
        t0 = time.perf_counter()
        L.check(L.lib().lizec_replicate_run_ragged(
            L.engine(0), K, 1, self.tables.ctypes.data_as(u8p),
            self.tables.shape[0], self.index.ctypes.data_as(u32p),
            self.src.ctypes.data_as(u64p), self.src_nb.ctypes.data_as(u32p),
            crc, self.sigs.ctypes.data_as(u8p), SIG_LEN, HDR, CRC_OFF,
            self.r_dst.ctypes.data_as(u64p), self.dst_nb.ctypes.data_as(u32p),
            self.S, 0, 0, bad), "lizec_replicate_run_ragged")
        dt = time.perf_counter() - t0
        if verify:
            assert not self.bad.any(), "a clean source failed its check"
        return dt

    def run_uniform(self):
        """lizec_replicate_run once per (padded length, pattern) group."""
        lib, e = L.lib(), L.engine(0)
        t0 = time.perf_counter()
        for plen, p, src, sigs, dst, n in self._group_args:
            L.check(lib.lizec_replicate_run(
                e, plen, K, 1, self.tables[p].ctypes.data_as(u8p),
                src.ctypes.data_as(u64p), sigs.ctypes.data_as(u8p), SIG_LEN,
                HDR, CRC_OFF, dst.ctypes.data_as(u64p), n, 0),
                "lizec_replicate_run")
        return time.perf_counter() - t0

    def compare_outputs(self):
        """The ragged images equal the uniform ones cut to their own block
        count (the CRC array compared that far)."""
        for s in range(self.S):
            nb = int(self.dst_nb[s, 0])
            r = self.r_out[int(self.r_off[s]):int(self.r_off[s] + self.r_size[s])]
            u = self.u_out[int(self.u_off[s]):int(self.u_off[s] + self.u_size[s])]
            assert np.array_equal(r[:CRC_OFF + 4 * nb], u[:CRC_OFF + 4 * nb]), s
            assert np.array_equal(r[HDR:], u[HDR:HDR + nb * BLOCK]), s

    def check_sample(self, sample):
        """The ragged images of a few chunks against the host twin."""
        for s in sample:
            out = np.zeros(int(self.r_size[s]), np.uint8)
            dst = np.array([out.ctypes.data], np.uint64)
            L.check(L.lib().lizec_replicate_ragged_host(
                K, 1, self.tables.ctypes.data_as(u8p), self.tables.shape[0],
                self.index[s:s + 1].ctypes.data_as(u32p),
                np.ascontiguousarray(self.src[s]).ctypes.data_as(u64p),
                self.src_nb[s].ctypes.data_as(u32p), None,
                self.sigs[s].ctypes.data_as(u8p), SIG_LEN, HDR, CRC_OFF,
                dst.ctypes.data_as(u64p), self.dst_nb[s].ctypes.data_as(u32p),
                1, 0, None), "lizec_replicate_ragged_host")
            got = self.r_out[int(self.r_off[s]):int(self.r_off[s] + self.r_size[s])]
            assert np.array_equal(got, out), s


def alternate(sides, passes):
    """One warm-up pass of every side, then `passes` passes in which the
    sides run one after the other; returns a list of times per side."""
    for f in sides:
        f()
    times = [[] for _ in sides]
    for _ in range(passes):
        for t, f in zip(times, sides):
            t.append(f())
    return times


def case_a(passes):
    pop = Population([1024] * 48, [1] * 48, 42)
    u1, r, u2 = alternate([pop.run_uniform, pop.run_ragged, pop.run_uniform],
                          passes)
    pop.compare_outputs()
    pop.check_sample([0, 47])
    return {"case": "A", "chunks": pop.S, "passes": passes,
            "pcie_bytes": pop.r_in + pop.r_outb,
            "uniform_s": stats(u1), "uniform_again_s": stats(u2),
            "ragged_s": stats(r),
            "uniform_again_over_uniform": ratio_stats(u2, u1),
            "ragged_over_uniform": ratio_stats(r, u1),
            "ragged_gibs": stats([(pop.r_in + pop.r_outb) / GIB / t
                                  for t in r]),
            "stages": pop.stages()}


def case_b(passes):
    rng = np.random.default_rng(20260)
    n = np.concatenate([np.full(128, 1024), rng.integers(1, 1024, 64),
                        rng.integers(1, 17, 64)])
    rng.shuffle(n)
    pop = Population(n, rng.integers(0, NPARTS, n.size), 43)
    u, r = alternate([pop.run_uniform, pop.run_ragged], passes)
    pop.compare_outputs()
    return {"case": "B", "chunks": pop.S, "passes": passes,
            "groups": len(pop.groups), "stages": pop.stages(),
            "ragged_pcie_bytes": pop.r_in + pop.r_outb,
            "grouped_pcie_bytes": pop.u_in + pop.u_outb,
            "grouped_s": stats(u), "ragged_s": stats(r),
            "ragged_over_grouped": ratio_stats(r, u),
            "ragged_gibs": stats([(pop.r_in + pop.r_outb) / GIB / t
                                  for t in r]),
            "grouped_gibs": stats([(pop.u_in + pop.u_outb) / GIB / t
                                   for t in u])}


def case_c(passes):
    rng = np.random.default_rng(20261)
    pop = Population([1] * 4096, rng.integers(0, NPARTS, 4096), 44)
    (r,) = alternate([pop.run_ragged], passes)
    pop.check_sample([0, 1, 2, 4095])
    stages = pop.stages()
    return {"case": "C", "chunks": pop.S, "passes": passes, "stages": stages,
            "pcie_bytes": pop.r_in + pop.r_outb,
            "copy_calls": pop.copies_ragged(stages), "ragged_s": stats(r),
            "chunks_per_s": stats([pop.S / t for t in r]),
            "ragged_gibs": stats([(pop.r_in + pop.r_outb) / GIB / t
                                  for t in r])}


def case_d(passes):
    pop = Population([1024] * 48, [1] * 48, 42, with_crcs=True)
    off, on = alternate([pop.run_ragged, lambda: pop.run_ragged(True)],
                        passes)
    return {"case": "D", "chunks": pop.S, "passes": passes,
            "pcie_bytes": pop.r_in + pop.r_outb,
            "verify_off_s": stats(off), "verify_on_s": stats(on),
            "on_over_off": ratio_stats(on, off)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--only", default="ABCD")
    ap.add_argument("--dump-json")
    a = ap.parse_args()
    if a.passes < 3:
        ap.error("at least 3 timed passes")
    import torch
    if not torch.cuda.is_available():
        sys.exit("replicate_ragged_ab needs a GPU: nothing is measured "
                 "without one")
    results = []
    for name, fn in (("A", case_a), ("B", case_b), ("C", case_c),
                     ("D", case_d)):
        if name in a.only:
            res = fn(a.passes)
            results.append(res)
            print(json.dumps(res), flush=True)
            if a.dump_json:
                with open(a.dump_json, "w") as f:
                    json.dump({"bench": "replicate_ragged_ab", "k": K, "m": M,
                               "host_buffers": "pinned",
                               "pcie_inclusive": True, "results": results},
                              f, indent=1)


if __name__ == "__main__":
    main()
