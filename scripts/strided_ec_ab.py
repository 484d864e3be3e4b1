#!/usr/bin/env python3
"""A/B the block-strided EC kernel against the uniform one on one MI355X.

For ec(8,2) and ec(16,4) encode over device-resident 8 MiB parts (128 blocks
of 64 KiB), times — in one process, after warm-up, in alternating repeats,
with device events around synchronised work —
  uniform     lizec_ec_encode_batch: contiguous 16-byte-aligned parts;
and lizec_ec_encode_batch_strided on the same bytes laid out as
  il-il       sources and destinations INTERLEAVED (stride 65540, block 0 at
              4 bytes into an image, images packed back to back);
  flat-il     contiguous aligned sources, INTERLEAVED destinations (rebuild
              into images);
  il-flat     INTERLEAVED sources, contiguous aligned destinations (read
              survivors from images);
  al-strided  16-byte-aligned but strided on both sides (65552 / 65600): the
              strided kernel with no misalignment, which separates the cost
              of the kernel's shape from that of the misaligned accesses.
The batch is sized past the 256 MiB last-level cache.  Every strided output
is checked byte-identical to the uniform one at the timed size.  Prints one
JSON document (and writes it to --out).
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

from lizardfs_amd import lib as L  # noqa: E402

BLOCK = 65536
WARMUP = 2
INNER = 20          # calls per timed sample (one call is ~0.3 ms)
# name -> ((source stride, offset of block 0), (destination stride, offset))
LAYOUTS = {
    "il-il": ((65540, 4), (65540, 4)),
    "flat-il": ((BLOCK, 0), (65540, 4)),
    "il-flat": ((65540, 4), (BLOCK, 0)),
    "al-strided": ((65552, 0), (65600, 0)),
}

u8p = ctypes.POINTER(ctypes.c_uint8)
u64p = ctypes.POINTER(ctypes.c_uint64)


class Parts:
    """n parts of nblocks blocks at `stride`, block 0 `off` bytes into a
    part's slot; slots are packed back to back, so with stride 65540 the
    parts start at every 4-byte phase."""

    def __init__(self, n, nblocks, stride, off):
        self.n, self.nblocks, self.stride, self.off = n, nblocks, stride, off
        self.slot = nblocks * stride
        self.buf = torch.zeros(n * self.slot + 16, dtype=torch.uint8,
                               device="cuda")
        self.ptrs = (np.uint64(self.buf.data_ptr() + off) +
                     np.arange(n, dtype=np.uint64) * np.uint64(self.slot))

    def blocks(self):
        """[n, nblocks, BLOCK] view of the data."""
        v = self.buf[:self.n * self.slot].view(self.n, self.nblocks,
                                               self.stride)
        return v[:, :, self.off:self.off + BLOCK]


def stats(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms),
                spread=(max(ms) - min(ms)) / med, samples_ms=ms)


def run_shape(lib, eng, k, m, S, nblocks, reps):
    tbl = np.zeros(32 * k * m, np.uint8)
    L.check(lib.lizec_rs_encode_tables(k, m, tbl.ctypes.data_as(u8p)))
    g = torch.Generator(device="cuda").manual_seed(7)
    flat_src = Parts(S * k, nblocks, BLOCK, 0)
    flat_src.blocks().copy_(torch.randint(
        0, 256, (S * k, nblocks, BLOCK), dtype=torch.uint8, device="cuda",
        generator=g))
    flat_dst = Parts(S * m, nblocks, BLOCK, 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def uniform():
        L.check(lib.lizec_ec_encode_batch(
            eng, nblocks * BLOCK, k, m, tbl.ctypes.data_as(u8p),
            flat_src.ptrs.ctypes.data_as(u64p),
            flat_dst.ptrs.ctypes.data_as(u64p), S, stream))

    legs = [("uniform", uniform, flat_dst)]
    for name, ((ss, so), (ds, do)) in LAYOUTS.items():
        src = flat_src if (ss, so) == (BLOCK, 0) else Parts(S * k, nblocks,
                                                            ss, so)
        if src is not flat_src:
            src.blocks().copy_(flat_src.blocks())
        dst = Parts(S * m, nblocks, ds, do)

        def strided(src=src, dst=dst):
            L.check(lib.lizec_ec_encode_batch_strided(
                eng, nblocks, k, m, tbl.ctypes.data_as(u8p),
                src.ptrs.ctypes.data_as(u64p), dst.ptrs.ctypes.data_as(u64p),
                S, src.stride, dst.stride, stream))
        legs.append((name, strided, dst))

    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _, _ in legs}
    for rep in range(WARMUP + reps):
        for name, fn, _ in legs:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(e0.elapsed_time(e1) / INNER)
    moved = S * nblocks * BLOCK * (k + m)      # bytes read + written
    st = {name: stats(ms) for name, ms in times.items()}
    ref = flat_dst.blocks()
    report = dict(k=k, m=m, stripes=S, nblocks=nblocks,
                  part_len=nblocks * BLOCK, bytes_moved=moved, reps=reps,
                  warmup=WARMUP, calls_per_sample=INNER, legs={})
    for name, _, dst in legs:
        report["legs"][name] = dict(
            st[name], gbps=moved / (st[name]["median_ms"] / 1e3) / 1e9,
            over_uniform=(st["uniform"]["median_ms"] /
                          st[name]["median_ms"]),
            equals_uniform=bool(torch.equal(dst.blocks(), ref)))
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1,
                    help="divide the stripe count (quick dry runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    lib, eng = L.lib(), L.engine(0)
    doc = dict(device=torch.cuda.get_device_name(0),
               expectation="a 1 KiB wave access off its 128-byte lines "
                           "touches 9 lines instead of 8: >= 8/9 = 0.889 of "
                           "uniform if HBM-bound", shapes=[])
    for k, m, S in ((8, 2, 16), (16, 4, 8)):
        r = run_shape(lib, eng, k, m, max(1, S // args.scale), 128, args.reps)
        doc["shapes"].append(r)
        for name, x in r["legs"].items():
            print(f"strided_ab ec({k},{m}) {name:10s} "
                  f"{x['median_ms']:.3f} ms {x['gbps']:.0f} GB/s "
                  f"x{x['over_uniform']:.3f} of uniform "
                  f"spread={x['spread']:.3f} same={x['equals_uniform']}",
                  flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    ok = all(x["equals_uniform"] for r in doc["shapes"]
             for x in r["legs"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
