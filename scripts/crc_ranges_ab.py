#!/usr/bin/env python3
"""Measure the byte-range CRC kernel and the write gate on one MI355X.

All legs run in one process, after warm-up, in alternating repeats, with
device events around synchronised work; a sample is INNER back-to-back calls
between two events, divided by INNER.  Every buffer is sized past the
256 MiB last-level cache.  Tables and op arrays are built outside the timed
region; a timed call still stages and uploads them, as every call does.

  (a) 64 KiB ranges, 16-byte aligned, back to back (lizec_crc32_ranges)
      against lizec_crc32_batch over the same bytes: what per-range
      addressing and the uneven split cost
  (b) the same at 4 mod 16, against the batch call's dword-load path
  (c) 4 KiB ranges at random byte alignment (no comparator)
  (d) lizec_write_gate_batch over 4 KiB partial writes into resident
      64 KiB blocks, in GiB/s of bytes read (block + data per op)

Results are checked at the timed size: (a), (b) ranges == batch; (c) a
sample of ranges against zlib; (d) every op OK and a sample of new CRCs
against zlib of the written block.  Prints one JSON document (and writes it
to --out).  No pass mark depends on these figures.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd import writegate as wg  # noqa: E402

BLOCK = 65536
WARMUP = 2
INNER = 20
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)


def stats(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms),
                spread=(max(ms) - min(ms)) / med, samples_ms=ms)


def time_legs(legs, reps):
    """legs: [(name, fn)].  Alternates the legs; returns name -> stats."""
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


def random_bytes(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda",
                         generator=g)


def aligned(n, skew, seed):
    """n random device bytes whose first byte is `skew` past a 16-byte
    boundary."""
    raw = random_bytes(n + 32, seed)
    start = (-raw.data_ptr()) % 16 + skew
    buf = raw[start:start + n]
    assert buf.data_ptr() % 16 == skew
    return buf


class Ranges:
    """A prepared lizec_crc32_ranges call."""

    def __init__(self, lib, eng, stream, base, offs, lens):
        self.lib, self.eng, self.stream = lib, eng, stream
        self.dptrs = (np.asarray(offs, np.uint64) + np.uint64(base))
        self.lens = np.asarray(lens, np.uint32)
        self.n = self.dptrs.size
        self.out = torch.zeros(self.n, dtype=torch.int32, device="cuda")

    def __call__(self):
        L.check(self.lib.lizec_crc32_ranges(
            self.eng, self.dptrs.ctypes.data_as(u64p),
            self.lens.ctypes.data_as(u32p), self.n, 0,
            ctypes.c_void_p(self.out.data_ptr()), self.stream))


def leg_report(st, nbytes, ref=None):
    out = {}
    for name, s in st.items():
        out[name] = dict(s, gbps=nbytes / (s["median_ms"] / 1e3) / 1e9,
                         gibps=nbytes / (s["median_ms"] / 1e3) / 2 ** 30)
        if ref:
            out[name]["of_" + ref] = st[ref]["median_ms"] / s["median_ms"]
    return out


def blocks_vs_batch(lib, eng, stream, nblocks, skew, reps):
    buf = aligned(nblocks * BLOCK, skew, 11 + skew)
    rg = Ranges(lib, eng, stream, buf.data_ptr(),
                np.arange(nblocks, dtype=np.uint64) * BLOCK,
                np.full(nblocks, BLOCK))
    bout = torch.zeros(nblocks, dtype=torch.int32, device="cuda")

    def batch():
        L.check(lib.lizec_crc32_batch(
            eng, ctypes.c_void_p(buf.data_ptr()), BLOCK, nblocks, 0,
            ctypes.c_void_p(bout.data_ptr()), stream))

    st = time_legs([("batch", batch), ("ranges", rg)], reps)
    same = bool(torch.equal(bout, rg.out))
    host = buf[:BLOCK].cpu().numpy().tobytes()
    first = int(rg.out[0].item()) & 0xFFFFFFFF
    return dict(ranges=nblocks, range_len=BLOCK, start_mod_16=skew,
                bytes=nblocks * BLOCK, ranges_equal_batch=same,
                first_equals_zlib=first == zlib.crc32(host),
                legs=leg_report(st, nblocks * BLOCK, "batch"))


def small_ranges(lib, eng, stream, n, length, reps):
    slot = length + 16
    buf = aligned(n * slot, 0, 21)
    rng = np.random.default_rng(20240)
    offs = np.arange(n, dtype=np.uint64) * slot + \
        rng.integers(0, 16, n).astype(np.uint64)
    rg = Ranges(lib, eng, stream, buf.data_ptr(), offs, np.full(n, length))
    st = time_legs([("ranges", rg)], reps)
    got = rg.out.cpu().numpy().view(np.uint32)
    sample = rng.choice(n, 256, replace=False)
    ok = all(int(got[i]) == zlib.crc32(
        buf[int(offs[i]):int(offs[i]) + length].cpu().numpy().tobytes())
        for i in sample)
    return dict(ranges=n, range_len=length, bytes=n * length,
                alignments=sorted(set(int(o) % 16 for o in offs)),
                sample_equals_zlib=bool(ok),
                legs=leg_report(st, n * length))


def gate(lib, eng, stream, n, size, reps):
    from lizardfs_amd import crc as lcrc
    blocks = aligned(n * BLOCK, 0, 31)
    data = aligned(n * size, 0, 32)
    stored = lcrc.crc32_blocks(blocks, BLOCK).view(torch.uint8) \
        .view(n, 4).flip(1).contiguous()             # big-endian bytes
    claimed = lcrc.crc32_blocks(data, size).cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    rng = np.random.default_rng(20241)
    offsets = rng.integers(0, BLOCK // size, n) * size
    ops = np.zeros(n, wg.OP_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    ops["data"] = np.uint64(data.data_ptr()) + idx * np.uint64(size)
    ops["block"] = np.uint64(blocks.data_ptr()) + idx * np.uint64(BLOCK)
    ops["stored"] = np.uint64(stored.data_ptr()) + idx * np.uint64(4)
    ops["offset"], ops["size"], ops["crc"] = offsets, size, claimed
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    newcrc = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        L.check(lib.lizec_write_gate_batch(
            eng, ctypes.c_void_p(ops.ctypes.data), n, 0,
            ctypes.c_void_p(status.data_ptr()),
            ctypes.c_void_p(newcrc.data_ptr()), stream))

    st = time_legs([("gate", call)], reps)
    all_ok = bool((status == 0).all().item())
    got = newcrc.cpu().numpy().view(np.uint32)
    ok = True
    for i in rng.choice(n, 16, replace=False):
        b = blocks[i * BLOCK:(i + 1) * BLOCK].cpu().numpy().copy()
        o = int(offsets[i])
        b[o:o + size] = data[i * size:(i + 1) * size].cpu().numpy()
        ok = ok and int(got[i]) == zlib.crc32(b.tobytes())
    read = n * (BLOCK + size)
    return dict(ops=n, write_size=size, bytes_read=read, all_ok=all_ok,
                sample_newcrc_equals_zlib=bool(ok),
                legs=leg_report(st, read))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1,
                    help="divide the sizes (quick dry runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    lib, eng = L.lib(), L.engine(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nblocks = 8192 // args.scale                     # 512 MiB of blocks
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               warmup=WARMUP, calls_per_sample=INNER)
    doc["a_64k_aligned"] = blocks_vs_batch(lib, eng, stream, nblocks, 0,
                                           args.reps)
    torch.cuda.empty_cache()
    doc["b_64k_4mod16"] = blocks_vs_batch(lib, eng, stream, nblocks, 4,
                                          args.reps)
    torch.cuda.empty_cache()
    doc["c_4k_random_alignment"] = small_ranges(lib, eng, stream,
                                                nblocks * 16, 4096, args.reps)
    torch.cuda.empty_cache()
    doc["d_gate_4k_partial"] = gate(lib, eng, stream, nblocks, 4096,
                                    args.reps)
    for key in ("a_64k_aligned", "b_64k_4mod16", "c_4k_random_alignment",
                "d_gate_4k_partial"):
        for name, x in doc[key]["legs"].items():
            print(f"crc_ranges_ab {key:22s} {name:7s} {x['median_ms']:.4f} ms "
                  f"{x['gbps']:.0f} GB/s ({x['gibps']:.0f} GiB/s) "
                  f"spread={x['spread']:.3f}", flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    ok = (doc["a_64k_aligned"]["ranges_equal_batch"] and
          doc["a_64k_aligned"]["first_equals_zlib"] and
          doc["b_64k_4mod16"]["ranges_equal_batch"] and
          doc["c_4k_random_alignment"]["sample_equals_zlib"] and
          doc["d_gate_4k_partial"]["all_ok"] and
          doc["d_gate_4k_partial"]["sample_newcrc_equals_zlib"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
