#!/usr/bin/env python3
"""Measure the degraded chunk write on one MI355X, by the method of
scripts/chunk_write_ab.py: all legs in one process, after warm-up, in
alternating repeats, a sample being INNER back-to-back calls between two
device events, divided by INNER.  ec(8,2), 16 chunks of 1024 blocks; data
part LOST_COL of every chunk is lost.

  (b') deg_write4   4096 writes of 4 whole blocks at random block offsets
                    through lizec_chunk_write_degraded_batch
       base_write4  what the parent offers for the same result:
                    lizec_chunk_read_batch rebuilds, per write and touched
                    row in which the lost column is a fill, that block of the
                    lost part into a scratch block; lizec_chunk_write_batch
                    then fills from the scratch
  (c') deg_sub4k    4096 writes of 4 KiB into one block each, at odd `from`,
                    odd data addresses, packet-compact odd parity addresses
       base_sub4k   the same composition: the read call works on whole 64 KiB
                    blocks, so it reads k whole blocks per write
  (h)  deg_healthy  leg (b) with nothing lost through the new entry
       base_healthy lizec_chunk_write_batch: what the wider source walk costs

Algorithmic bytes: every byte a call has to read once, plus what it writes.
Checked at the timed size, before and after timing: the degraded legs equal
the host twin (lizec_chunk_write_degraded_host) over the same bytes and the
baseline composition's output; the healthy leg equals lizec_chunk_write_batch.
Prints one JSON document (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lizardfs_amd import chunkwrite  # noqa: E402
from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd import slice_traits as st  # noqa: E402

BLOCK = 65536
K, M, NB = 8, 2, 1024
PB = NB // K
LOST_COL = 3
SRCS = K + M
WARMUP = 2
INNER = 5
HBM_PEAK = 8e12
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def stats(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms),
                spread=(max(ms) - min(ms)) / med, samples_ms=ms)


def time_legs(legs, reps):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in legs}
    for rep in range(WARMUP + reps):
        for name, fn in legs:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(e0.elapsed_time(e1) / INNER)
    return {name: stats(ms) for name, ms in times.items()}


def p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def run_mask(first, count, b):
    lo = max(first, b * K) - b * K
    hi = min(first + count, b * K + K) - b * K
    return ((1 << hi) - 1) & ~((1 << lo) - 1)


class Tables:
    """The composite tables of a batch, one per distinct row shape."""

    def __init__(self, avail):
        self.avail, self.keys, self.tbls, self.masks = avail, {}, [], []
        self.slots = np.arange(SRCS, dtype=np.uint8)

    def index(self, new_mask):
        if new_mask not in self.keys:
            tbl = np.zeros(32 * (K + SRCS) * M, np.uint8)
            mask = ctypes.c_uint32()
            L.check(L.lib().lizec_degraded_write_table(
                K, M, 0, new_mask, (1 << K) - 1, self.avail,
                p(self.slots, u8p), SRCS, p(tbl, u8p), ctypes.byref(mask)))
            self.keys[new_mask] = len(self.tbls)
            self.tbls.append(tbl)
            self.masks.append(mask.value)
        return self.keys[new_mask]

    def of(self, first, count):
        """-> tbl_index [W, 3], ranges read per write"""
        W = len(first)
        idx = np.zeros((W, 3), np.uint32)
        cols = np.zeros(W, np.int64)
        for w in range(W):
            r0, r1 = first[w] // K, (first[w] + count - 1) // K
            for t, b in enumerate((r0, (r0 + r1) // 2, r1)):
                idx[w, t] = self.index(run_mask(int(first[w]), count, int(b)))
            for b in range(int(r0), int(r1) + 1):
                nm = run_mask(int(first[w]), count, b)
                cols[w] += bin(nm).count("1") + \
                    bin(self.masks[self.index(nm)]).count("1")
        return idx, cols

    def arrays(self):
        return np.concatenate(self.tbls), np.array(self.masks, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    lib, eng = L.lib(), L.engine(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    S = args.chunks
    enc = chunkwrite.encode_table(st.ec_slice_type(K, M))

    g = torch.Generator(device="cuda").manual_seed(4712)
    chunk = torch.randint(0, 256, (S, NB, BLOCK), dtype=torch.uint8,
                          device="cuda", generator=g)
    # all parts as they are on the chunkservers: data 0..K-1, parity K..
    parts = torch.empty((SRCS, S, PB * BLOCK), dtype=torch.uint8,
                        device="cuda")
    for d in range(K):
        parts[d].view(S, PB, BLOCK).copy_(chunk[:, d::K])
    rows = np.arange(S, dtype=np.uint64)
    wr_a = np.zeros(S, chunkwrite.WRITE_DTYPE)
    wr_a["data"] = np.uint64(chunk.data_ptr()) + rows * np.uint64(NB * BLOCK)
    wr_a["data_stride"] = wr_a["par_stride"] = BLOCK
    wr_a["block_count"], wr_a["to"] = NB, BLOCK
    pp_a = np.ascontiguousarray(
        np.uint64(parts[K].data_ptr()) +
        np.arange(M, dtype=np.uint64)[None, :] * np.uint64(parts.stride(0)) +
        rows[:, None] * np.uint64(parts.stride(1)))
    L.check(lib.lizec_chunk_write_batch(
        eng, M, p(enc, u8p), ctypes.c_void_p(wr_a.ctypes.data), S,
        p(np.zeros((S, K), np.uint64), u64p),
        p(np.zeros((S, K), np.uint32), u32p), K, BLOCK, p(pp_a, u64p),
        stream))
    torch.cuda.synchronize()

    rng = np.random.default_rng(98)
    W = S * 256
    sel = np.repeat(np.arange(S), 256).astype(np.uint64)
    part_p = np.ascontiguousarray(
        np.uint64(parts.data_ptr()) +
        np.arange(SRCS, dtype=np.uint64)[None, :] *
        np.uint64(parts.stride(0)) + sel[:, None] * np.uint64(parts.stride(1)))
    idx = np.arange(W, dtype=np.uint64)
    all_parts = (1 << SRCS) - 1
    avail = all_parts & ~(1 << LOST_COL)
    # the survivors of a rebuild: the first K available parts, ascending
    surv = [q for q in range(SRCS) if q != LOST_COL][:K]
    dec = np.zeros(32 * K, np.uint8)
    ic, oc = ctypes.c_int(), ctypes.c_int()
    present = sum(1 << q for q in surv)
    L.check(lib.lizec_rs_tables(K, M, ctypes.c_uint64(present),
                                ctypes.c_uint64(present),
                                ctypes.c_uint64(1 << LOST_COL), p(dec, u8p),
                                ctypes.byref(ic), ctypes.byref(oc)))

    class Leg:
        """One write shape: its arrays for the degraded call, the healthy
        call and the baseline composition."""

        def __init__(self, first, count, frm, size, data, dstride, par_shape,
                     pstride, odd):
            self.first, self.count, self.size = first, count, size
            self.data = data
            self.par = torch.empty((W, M) + par_shape, dtype=torch.uint8,
                                   device="cuda")
            self.par_base = torch.empty_like(self.par)
            touched = (first + count - 1) // K - first // K + 1
            self.T = int(touched.max())
            self.ncrc = count + self.T * M
            self.crc = torch.empty((W, self.ncrc), dtype=torch.int32,
                                   device="cuda")
            self.crc_base = torch.empty_like(self.crc)
            wr = np.zeros(W, chunkwrite.WRITE_DTYPE)
            wr["data"] = np.uint64(data.data_ptr()) + idx * \
                np.uint64(data.stride(0))
            wr["data_stride"], wr["par_stride"] = dstride, pstride
            wr["first_block"], wr["block_count"] = first, count
            wr["from"], wr["to"] = frm, frm + size
            shift = (1 + 2 * (idx % 8)) if odd else np.zeros(W, np.uint64)
            wr["data"] += shift.astype(np.uint64)
            self.wr = wr

            def outs(par, crc):
                w2 = wr.copy()
                w2["crcs"] = np.uint64(crc.data_ptr()) + idx * \
                    np.uint64(4 * self.ncrc)
                pp = np.ascontiguousarray(
                    np.uint64(par.data_ptr()) + idx[:, None] *
                    np.uint64(par.stride(0)) +
                    np.arange(M, dtype=np.uint64)[None, :] *
                    np.uint64(par.stride(1)) + shift[:, None].astype(np.uint64))
                return w2, pp
            self.wr_new, self.pp_new = outs(self.par, self.crc)
            self.wr_base, self.pp_base = outs(self.par_base, self.crc_base)
            # the degraded call: every part a slot, the lost one nowhere
            self.old_p = part_p.copy()
            self.old_n = np.full((W, SRCS), PB, np.uint32)
            self.old_p[:, LOST_COL] = 0
            self.old_n[:, LOST_COL] = 0
            tabs = Tables(avail)
            self.index, cols = tabs.of(first, count)
            self.tbl, self.masks = tabs.arrays()
            self.bytes_new = int((cols + touched * M).sum()) * size
            healthy = Tables(all_parts)
            self.h_index, _ = healthy.of(first, count)
            self.h_tbl, self.h_masks = healthy.arrays()
            # the baseline: one read per (write, row) in which the lost
            # column is a fill, into a scratch block of the write's own
            r0 = first // K
            need = [(w, int(b)) for w in range(W)
                    for b in range(int(r0[w]), int(r0[w] + touched[w]))
                    if not (run_mask(int(first[w]), count, b) >> LOST_COL) & 1]
            self.scratch = torch.empty((W, self.T, BLOCK), dtype=torch.uint8,
                                       device="cuda")
            R = len(need)
            self.rd_src = np.ascontiguousarray(
                part_p[[w for w, _ in need]][:, surv])
            self.rd_nb = np.full((R, K), PB, np.uint32)
            cmap = np.full((R, K), 0xFF, np.uint8)
            cmap[:, LOST_COL] = 0x80
            self.rd_cmap = cmap
            self.rd_first = np.array([b * K + LOST_COL for _, b in need],
                                     np.uint32)
            self.rd_count = np.ones(R, np.uint32)
            self.rd_index = np.zeros(R, np.uint32)
            self.rd_dst = np.array(
                [self.scratch.data_ptr() +
                 (w * self.T + b - int(r0[w])) * BLOCK for w, b in need],
                np.uint64)
            self.fill_p = np.ascontiguousarray(part_p[:, :K])
            self.fill_p[:, LOST_COL] = np.uint64(self.scratch.data_ptr()) + \
                idx * np.uint64(self.T * BLOCK) - \
                r0.astype(np.uint64) * np.uint64(BLOCK)
            self.fill_n = np.full((W, K), PB, np.uint32)
            self.healthy_fill = np.ascontiguousarray(part_p[:, :K])
            # rebuild: K blocks read, one written; write: the K columns of
            # every touched row read once, M parities written
            self.bytes_base = R * (K + 1) * BLOCK + \
                int(touched.sum()) * (K + M) * size
            self.bytes_healthy = int(touched.sum()) * (K + M) * size
            self.rebuilds = R

        def degraded(self):
            L.check(lib.lizec_chunk_write_degraded_batch(
                eng, M, p(self.tbl, u8p), len(self.masks),
                p(self.masks, u32p), p(self.index, u32p),
                ctypes.c_void_p(self.wr_new.ctypes.data), W,
                p(self.old_p, u64p), p(self.old_n, u32p), SRCS, K, BLOCK,
                p(self.pp_new, u64p), stream))

        def degraded_healthy(self):
            L.check(lib.lizec_chunk_write_degraded_batch(
                eng, M, p(self.h_tbl, u8p), len(self.h_masks),
                p(self.h_masks, u32p), p(self.h_index, u32p),
                ctypes.c_void_p(self.wr_new.ctypes.data), W,
                p(part_p, u64p), p(np.full((W, SRCS), PB, np.uint32), u32p),
                SRCS, K, BLOCK, p(self.pp_new, u64p), stream))

        def healthy(self):
            L.check(lib.lizec_chunk_write_batch(
                eng, M, p(enc, u8p),
                ctypes.c_void_p(self.wr_base.ctypes.data), W,
                p(self.healthy_fill, u64p), p(self.fill_n, u32p), K, BLOCK,
                p(self.pp_base, u64p), stream))

        def baseline(self):
            if self.rebuilds:
                L.check(lib.lizec_chunk_read_batch(
                    eng, K, 1, p(dec, u8p), 1, p(self.rd_index, u32p),
                    p(self.rd_src, u64p), p(self.rd_nb, u32p), K,
                    p(self.rd_cmap, u8p), p(self.rd_first, u32p),
                    p(self.rd_count, u32p), p(self.rd_dst, u64p),
                    self.rebuilds, BLOCK, BLOCK, stream))
            L.check(lib.lizec_chunk_write_batch(
                eng, M, p(enc, u8p),
                ctypes.c_void_p(self.wr_base.ctypes.data), W,
                p(self.fill_p, u64p), p(self.fill_n, u32p), K, BLOCK,
                p(self.pp_base, u64p), stream))

        def host_twin(self):
            if hasattr(self, "twin"):
                return self.twin
            h_parts, h_data = parts.cpu().numpy(), self.data.cpu().numpy()
            h_par = np.full(tuple(self.par.shape), 0xA5, np.uint8)
            h_crc = np.zeros(tuple(self.crc.shape), np.uint32)
            w2 = self.wr_new.copy()
            w2["data"] = w2["data"] - np.uint64(self.data.data_ptr()) + \
                np.uint64(h_data.ctypes.data)
            w2["crcs"] = w2["crcs"] - np.uint64(self.crc.data_ptr()) + \
                np.uint64(h_crc.ctypes.data)
            o2 = np.where(self.old_n > 0, self.old_p -
                          np.uint64(parts.data_ptr()) +
                          np.uint64(h_parts.ctypes.data), np.uint64(0))
            o2 = np.ascontiguousarray(o2.astype(np.uint64))
            p2 = self.pp_new - np.uint64(self.par.data_ptr()) + \
                np.uint64(h_par.ctypes.data)
            L.check(lib.lizec_chunk_write_degraded_host(
                M, p(self.tbl, u8p), len(self.masks), p(self.masks, u32p),
                p(self.index, u32p), ctypes.c_void_p(w2.ctypes.data), W,
                p(o2, u64p), p(self.old_n, u32p), SRCS, K, BLOCK,
                p(p2, u64p)))
            self.twin = h_par, h_crc
            return self.twin

        def check(self, name, res):
            for t in (self.par, self.par_base):
                t.fill_(0xA5)
            self.crc.zero_()
            self.crc_base.zero_()
            self.degraded()
            self.baseline()
            torch.cuda.synchronize()
            h_par, h_crc = self.host_twin()
            res[name + "_parity_eq_host"] = bool(
                np.array_equal(self.par.cpu().numpy(), h_par))
            res[name + "_crcs_eq_host"] = bool(np.array_equal(
                self.crc.cpu().numpy().view(np.uint32), h_crc))
            res[name + "_parity_eq_baseline"] = bool(
                torch.equal(self.par, self.par_base))
            res[name + "_crcs_eq_baseline"] = bool(
                torch.equal(self.crc, self.crc_base))

    first4 = rng.integers(0, NB - 3, W).astype(np.uint32)
    data4 = torch.randint(0, 256, (W, 4 * BLOCK), dtype=torch.uint8,
                          device="cuda", generator=g)
    leg_b = Leg(first4, 4, 0, BLOCK, data4, BLOCK, (2 * BLOCK,), BLOCK, False)
    SUB = 4096
    first_c = rng.integers(0, NB, W).astype(np.uint32)
    from_c = (rng.integers(0, (BLOCK - SUB) // 2, W) * 2 + 1).astype(np.uint32)
    data_c = torch.randint(0, 256, (W, SUB + 34), dtype=torch.uint8,
                           device="cuda", generator=g)
    leg_c = Leg(first_c, 1, from_c, SUB, data_c, SUB, (SUB + 18,), SUB, True)

    def check_all():
        res = {}
        leg_b.check("write4", res)
        leg_c.check("sub4k", res)
        leg_b.par.fill_(0xA5)
        leg_b.par_base.fill_(0xA5)
        leg_b.crc.zero_()
        leg_b.crc_base.zero_()
        leg_b.degraded_healthy()
        leg_b.healthy()
        torch.cuda.synchronize()
        res["healthy_parity_eq_write_batch"] = bool(
            torch.equal(leg_b.par, leg_b.par_base))
        res["healthy_crcs_eq_write_batch"] = bool(
            torch.equal(leg_b.crc, leg_b.crc_base))
        return res

    legs = [("deg_write4", leg_b.degraded), ("base_write4", leg_b.baseline),
            ("deg_sub4k", leg_c.degraded), ("base_sub4k", leg_c.baseline),
            ("deg_healthy", leg_b.degraded_healthy),
            ("base_healthy", leg_b.healthy)]
    checks = check_all()
    st_ = time_legs(legs, args.reps)
    checks_after = check_all()

    bytes_of = dict(deg_write4=leg_b.bytes_new, base_write4=leg_b.bytes_base,
                    deg_sub4k=leg_c.bytes_new, base_sub4k=leg_c.bytes_base,
                    deg_healthy=leg_b.bytes_healthy,
                    base_healthy=leg_b.bytes_healthy)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               warmup=WARMUP, calls_per_sample=INNER, slice="ec(8,2)",
               lost_part=LOST_COL, chunks=S, blocks_per_chunk=NB, writes=W,
               sub_bytes=SUB, tables=dict(write4=len(leg_b.masks),
                                          sub4k=len(leg_c.masks)),
               rebuilt_blocks=dict(write4=leg_b.rebuilds,
                                   sub4k=leg_c.rebuilds),
               checks=checks, checks_after=checks_after, legs={}, verdict={})
    for name, s in st_.items():
        gbps = bytes_of[name] / (s["median_ms"] / 1e3) / 1e9
        doc["legs"][name] = dict(s, algorithmic_bytes=bytes_of[name],
                                 gbps=gbps, hbm_share=gbps * 1e9 / HBM_PEAK)
        print(f"chunk_write_degraded_ab {name:13s} {s['median_ms']:.4f} ms "
              f"{bytes_of[name] / 1e6:.1f} MB {gbps:.0f} GB/s "
              f"({100 * gbps * 1e9 / HBM_PEAK:.1f}% of peak) "
              f"spread={s['spread']:.3f}", flush=True)
    for shape, new, base in (("write4", "deg_write4", "base_write4"),
                             ("sub4k", "deg_sub4k", "base_sub4k"),
                             ("healthy", "deg_healthy", "base_healthy")):
        n, b = st_[new], st_[base]
        spread_ms = max(n["max_ms"] - n["min_ms"], b["max_ms"] - b["min_ms"])
        doc["verdict"][shape] = dict(
            new_ms=n["median_ms"], baseline=base, baseline_ms=b["median_ms"],
            ratio=n["median_ms"] / b["median_ms"], sample_spread_ms=spread_ms,
            not_above_baseline_by_more_than_spread=n["median_ms"] -
            b["median_ms"] <= spread_ms)
        print(f"chunk_write_degraded_ab {shape}: new {n['median_ms']:.4f} ms, "
              f"{base} {b['median_ms']:.4f} ms, ratio "
              f"{n['median_ms'] / b['median_ms']:.3f}", flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all(checks.values()) and all(checks_after.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
