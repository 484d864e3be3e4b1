#!/usr/bin/env python3
"""Measure the verified chunk read against what a caller could compose
without it, on one MI355X.  Method of scripts/chunk_read_ab.py: all legs in
one process, after warm-up, in alternating repeats, device events around
synchronised work, a sample being INNER back-to-back calls divided by INNER.

The slice is ec(8,2); 16 chunks of 1024 blocks hold 1 GiB of chunk data, past
the 256 MiB last-level cache.  Both strides are 65536, the CRCs are arrays at
stride 4.  Whole-chunk reads, two shapes: healthy, and data part 3 lost (the
first parity read in its place).  Legs, per shape:

  new        lizec_chunk_read_verified_batch
  base_crc   lizec_crc32_ranges over the same source blocks (16384 addresses,
             the list built outside the timed region)
  base_read  lizec_chunk_read_batch alone — the unverified read, for
             orientation
  base_both  base_crc then base_read, back to back on the stream: the
             parent's composition.  Its copy of 64 KiB of CRCs to the host
             and the compare there are NOT timed, in the baseline's favour.

lizec_crc32_ranges and lizec_chunk_read_batch are untouched by the verified
read, so one process measures the parent's composition and the new call side
by side.

Checked at the timed size, before and after timing: the output equals the
chunk data and every mask is 0; one flipped source byte sets exactly the bit
of its slot in its chunk's mask; the composition's CRCs equal the stored
ones.  Prints one JSON document (and writes it to --out).
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

from lizardfs_amd import chunkread  # noqa: E402
from lizardfs_amd import crc as lcrc  # noqa: E402
from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd.ec import ReedSolomon, _pattern_table  # noqa: E402

BLOCK = 65536
K, M, NB = 8, 2, 1024
PB = NB // K                      # blocks per part
WARMUP = 2
INNER = 5
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

    # ---- the chunks, their parts and the parts' CRCs
    g = torch.Generator(device="cuda").manual_seed(4712)
    chunk = torch.randint(0, 256, (S, NB, BLOCK), dtype=torch.uint8,
                          device="cuda", generator=g)
    parts = torch.empty((K + M, S, PB * BLOCK), dtype=torch.uint8,
                        device="cuda")
    for d in range(K):
        parts[d].view(S, PB, BLOCK).copy_(chunk[:, d::K])
    rs = ReedSolomon(K, M)
    parity = rs.encode_batch(parts[:K].permute(1, 0, 2).contiguous())
    parts[K:].copy_(parity.permute(1, 0, 2))
    rs.sync()
    del parity
    native = lcrc.crc32_blocks(parts.view(-1), BLOCK)      # [(K+M)*S*PB]
    torch.cuda.synchronize()
    crcs = native.view(torch.uint8).view(-1, 4).flip(1).contiguous() \
        .view(K + M, S, 4 * PB)                            # big-endian
    native = native.view(K + M, S, PB)
    out = torch.empty((S, NB * BLOCK), dtype=torch.uint8, device="cuda")
    flat = chunk.view(S, NB * BLOCK)
    rows = np.arange(S, dtype=np.uint64)
    out_ptrs = np.ascontiguousarray(
        np.uint64(out.data_ptr()) + rows * np.uint64(out.stride(0)))
    bad = torch.empty(S, dtype=torch.int32, device="cuda")

    def ptrs(t, plist):
        return np.ascontiguousarray(
            np.uint64(t.data_ptr()) +
            np.array(plist, np.uint64)[None, :] * np.uint64(t.stride(0)) +
            rows[:, None] * np.uint64(t.stride(1)))

    def make(lost):
        srcs = [q for q in range(K + M) if q not in lost][:K] if lost \
            else list(range(K))
        cmap = np.array([srcs.index(c) if c in srcs
                         else chunkread.LOST + sorted(lost).index(c)
                         for c in range(K)], np.uint8)
        tbl = None
        if lost:
            em = ((1 << (K + M)) - 1) & ~sum(1 << q for q in srcs)
            tbl, got = _pattern_table(K, M, em, sum(1 << q for q in lost))
            assert list(got) == sorted(lost)
            tbl = np.ascontiguousarray(tbl)
        sp, cp = ptrs(parts, srcs), ptrs(crcs, srcs)
        nb = np.full((S, K), PB, np.uint32)
        cm = np.ascontiguousarray(np.tile(cmap, (S, 1)))
        first, count = np.zeros(S, np.uint32), np.full(S, NB, np.uint32)
        head = (K, len(lost), p(tbl, u8p), 1 if lost else 0, None,
                p(sp, u64p), p(nb, u32p), K, p(cm, u8p), p(first, u32p),
                p(count, u32p), p(out_ptrs, u64p), S, BLOCK, BLOCK)
        keep = (tbl, sp, cp, nb, cm, first, count)
        # the composition's address list: every block of every source
        addrs = np.ascontiguousarray(
            (sp[:, :, None] + np.arange(PB, dtype=np.uint64)[None, None, :] *
             np.uint64(BLOCK)).reshape(-1))
        lens = np.full(addrs.size, BLOCK, np.uint32)
        got_crcs = torch.empty(addrs.size, dtype=torch.int32, device="cuda")
        want_crcs = native[srcs].permute(1, 0, 2).reshape(-1)

        def new():
            L.check(lib.lizec_chunk_read_verified_batch(
                eng, *head, p(cp, u64p), 4, ctypes.c_void_p(bad.data_ptr()),
                stream))

        def base_crc():
            L.check(lib.lizec_crc32_ranges(
                eng, p(addrs, u64p), p(lens, u32p), addrs.size, 0,
                ctypes.c_void_p(got_crcs.data_ptr()), stream))

        def base_read():
            L.check(lib.lizec_chunk_read_batch(eng, *head, stream))

        def base_both():
            base_crc()
            base_read()
        return dict(new=new, base_crc=base_crc, base_read=base_read,
                    base_both=base_both, keep=keep, srcs=srcs,
                    got=got_crcs, want=want_crcs, blocks=int(addrs.size))

    shapes = {"healthy": make(()), "lost1": make((3,))}
    legs = [(f"{leg}_{name}", sh[leg]) for name, sh in shapes.items()
            for leg in ("new", "base_crc", "base_read", "base_both")]

    def check_all():
        res = {}
        for name, sh in shapes.items():
            for leg in ("new", "base_both"):
                out.fill_(0xA5)
                bad.fill_(-1)
                sh["got"].fill_(0)
                sh[leg]()
                torch.cuda.synchronize()
                ok = bool(torch.equal(out, flat))
                if leg == "new":
                    ok = ok and not bool(bad.any())
                else:
                    ok = ok and bool(torch.equal(sh["got"], sh["want"]))
                res[f"{leg}_{name}"] = ok
            # one flipped byte: chunk 5, slot 2, block 77
            part = sh["srcs"][2]
            parts[part, 5, 77 * BLOCK + 4321] ^= 0x20
            sh["new"]()
            torch.cuda.synchronize()
            parts[part, 5, 77 * BLOCK + 4321] ^= 0x20
            want = [0] * S
            want[5] = 1 << 2
            res[f"flip_{name}"] = bad.cpu().tolist() == want
        return res

    checks = check_all()
    st_ = time_legs(legs, args.reps)
    checks_after = check_all()

    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               warmup=WARMUP, calls_per_sample=INNER, slice="ec(8,2)",
               chunks=S, blocks_per_chunk=NB, chunk_bytes=S * NB * BLOCK,
               source_blocks={n: sh["blocks"] for n, sh in shapes.items()},
               checks=checks, checks_after=checks_after, legs=st_,
               verdict={})
    for name, s in st_.items():
        print(f"chunk_read_verified_ab {name:18s} {s['median_ms']:.4f} ms "
              f"spread={s['spread']:.3f}", flush=True)
    for name in shapes:
        n, c, r, b = (st_[f"{leg}_{name}"] for leg in
                      ("new", "base_crc", "base_read", "base_both"))
        total = c["median_ms"] + r["median_ms"]
        spread_ms = max(x["max_ms"] - x["min_ms"] for x in (n, c, r))
        doc["verdict"][name] = dict(
            new_ms=n["median_ms"], base_crc_ms=c["median_ms"],
            base_read_ms=r["median_ms"], base_sum_ms=total,
            base_both_ms=b["median_ms"], ratio_to_sum=n["median_ms"] / total,
            sample_spread_ms=spread_ms,
            not_above_sum_by_more_than_spread=n["median_ms"] - total <=
            spread_ms)
        print(f"chunk_read_verified_ab {name}: new {n['median_ms']:.4f} ms, "
              f"crc {c['median_ms']:.4f} + read {r['median_ms']:.4f} = "
              f"{total:.4f} ms (back to back {b['median_ms']:.4f}), ratio "
              f"{n['median_ms'] / total:.3f}", flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all(checks.values()) and all(checks_after.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
