#!/usr/bin/env python3
"""Measure the read gate against what a caller could do without it, on one
MI355X.

All legs run in one process, after warm-up, in alternating repeats, with
device events around synchronised work; a sample is INNER back-to-back calls
between two events, divided by INNER.  The images hold 512 MiB of blocks, past
the 256 MiB last-level cache.  Tables and op arrays are built outside the
timed region; a timed call still stages and uploads them, as every call does.

Images are MooseFS-format parts of 64 blocks (header 4 KiB, CRC array at
1024), so blocks are 16-byte aligned.  Two workloads, one request per block:
whole-block reads and 4 KiB reads at a random 4 KiB offset.  Each with three
packet placements, named by (out + 4 - block - offset) mod 16:

  d0   16-byte stores (the packet's data aligned with its source)
  d4   dword-aligned stores (the packet itself 16-byte aligned)
  d5   byte stores (an odd placement)

Legs per workload:

  scrub     lizec_scrub_batch_strided over all images       } the baseline:
  ranges    lizec_crc32_ranges over the requested ranges    } three passes a
  copy_dK   one strided device copy into the packets' data  } caller has today
  baseline_dK   the three back to back, as one timed sequence
  gate_dK   lizec_read_gate_batch
  ceiling   lizec_crc32_ranges over the whole blocks (read-only; orientation)

The baseline neither writes the packets' CRC fields nor tells which request
hit a damaged block (the scrub names one block per image); both would cost it
more.  The functions of the baseline are unchanged by the read gate (their
kernels compile to the same instructions), so this one process measures the
parent's baseline and the new call side by side.

Checked at the timed size: every status OK, a sample of packets against zlib,
the copy legs' data equal to the gate's.  Prints one JSON document (and
writes it to --out).
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

from lizardfs_amd import crc as lcrc  # noqa: E402
from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd import readgate as rg  # noqa: E402

BLOCK = 65536
HEADER, CRC_OFF, PER_IMAGE = 4096, 1024, 64
IMAGE = HEADER + PER_IMAGE * BLOCK
WARMUP = 2
INNER = 10
PLACEMENTS = (("d0", 12), ("d4", 0), ("d5", 1))   # name, out mod 16
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


def build_images(nimages):
    """nimages MooseFS-format images back to back in one 16-byte aligned
    buffer, random blocks, correct stored CRCs."""
    g = torch.Generator(device="cuda").manual_seed(4711)
    buf = torch.randint(0, 256, (nimages * IMAGE,), dtype=torch.uint8,
                        device="cuda", generator=g)
    assert buf.data_ptr() % 16 == 0
    v = buf.view(nimages, IMAGE)
    for i in range(nimages):
        crcs = lcrc.crc32_blocks(v[i, HEADER:], BLOCK)
        v[i, CRC_OFF:CRC_OFF + 4 * PER_IMAGE] = \
            crcs.view(torch.uint8).view(PER_IMAGE, 4).flip(1).reshape(-1)
    torch.cuda.synchronize()
    return buf


def workload(lib, eng, stream, images, nimages, size, reps, name):
    n = nimages * PER_IMAGE
    base = images.data_ptr()
    idx = np.arange(n, dtype=np.int64)
    boff = (idx // PER_IMAGE) * IMAGE + HEADER + (idx % PER_IMAGE) * BLOCK
    soff = (idx // PER_IMAGE) * IMAGE + CRC_OFF + 4 * (idx % PER_IMAGE)
    rng = np.random.default_rng(99)
    offset = np.zeros(n, np.int64) if size == BLOCK else \
        rng.integers(0, BLOCK // size, n) * size
    pstride = size + 16                          # keeps every packet's phase
    arena = torch.zeros(n * pstride + 64, dtype=torch.uint8, device="cuda")
    abase = arena.data_ptr()
    assert abase % 16 == 0

    # --- baseline legs
    dptrs = (base + np.arange(nimages, dtype=np.uint64) * IMAGE) \
        .astype(np.uint64)
    doffs = np.full(nimages, HEADER, np.uint32)
    coffs = np.full(nimages, CRC_OFF, np.uint32)
    counts = np.full(nimages, PER_IMAGE, np.uint32)
    scrub_out = torch.zeros(nimages, dtype=torch.int32, device="cuda")

    def scrub():
        L.check(lib.lizec_scrub_batch_strided(
            eng, dptrs.ctypes.data_as(u64p), doffs.ctypes.data_as(u32p),
            coffs.ctypes.data_as(u32p), counts.ctypes.data_as(u32p), nimages,
            BLOCK, 4, ctypes.c_void_p(scrub_out.data_ptr()), stream))

    raddr = (base + boff + offset).astype(np.uint64)
    rlens = np.full(n, size, np.uint32)
    rout = torch.zeros(n, dtype=torch.int32, device="cuda")
    waddr = (base + boff).astype(np.uint64)
    wlens = np.full(n, BLOCK, np.uint32)

    def ranges(addr=raddr, lens=rlens):
        L.check(lib.lizec_crc32_ranges(
            eng, addr.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), n, 0,
            ctypes.c_void_p(rout.data_ptr()), stream))

    # the copy.  Whole blocks: one strided copy, images -> packets.  4 KiB
    # reads: the ranges here start at multiples of their size (and so do
    # header and image), which lets the caller select them as rows of the
    # image buffer — one gather into a temporary, one strided copy; ranges
    # at arbitrary byte offsets would need a per-byte index and cost more.
    src_blocks = torch.as_strided(images, (nimages, PER_IMAGE, BLOCK),
                                  (IMAGE, BLOCK, 1), HEADER)
    if size != BLOCK:
        assert HEADER % size == 0 and IMAGE % size == 0
        rows = images.view(-1, size)
        row_index = torch.from_numpy((boff + offset) // size).cuda()

    def make_copy(first):
        if size == BLOCK:
            d3 = torch.as_strided(arena, (nimages, PER_IMAGE, BLOCK),
                                  (PER_IMAGE * pstride, pstride, 1), first + 4)
            return lambda: d3.copy_(src_blocks)
        d2 = torch.as_strided(arena, (n, size), (pstride, 1), first + 4)
        return lambda: d2.copy_(rows.index_select(0, row_index))

    # --- the gate
    status = torch.zeros(n, dtype=torch.int32, device="cuda")

    def make_gate(first):
        ops = np.zeros(n, rg.OP_DTYPE)
        ops["block"] = base + boff
        ops["stored"] = base + soff
        ops["out"] = abase + first + idx * pstride
        ops["offset"], ops["size"] = offset, size

        def call():
            L.check(lib.lizec_read_gate_batch(
                eng, ctypes.c_void_p(ops.ctypes.data), n, 0,
                ctypes.c_void_p(status.data_ptr()), stream))
        return call, ops

    legs = [("scrub", scrub), ("ranges", ranges),
            ("ceiling", lambda: ranges(waddr, wlens))]
    gates = {}
    for pname, first in PLACEMENTS:
        copy = make_copy(first)
        gate, ops = make_gate(first)
        gates[pname] = (gate, ops, copy, first)
        assert (int(ops["out"][0]) + 4 - int(ops["block"][0]) -
                int(ops["offset"][0])) % 16 == int(pname[1:])

        def baseline(copy=copy):
            scrub()
            ranges()
            copy()
        legs += [("copy_" + pname, copy), ("baseline_" + pname, baseline),
                 ("gate_" + pname, gate)]
    st = time_legs(legs, reps)

    # --- checks at the timed size
    checks = {}
    host_rng = np.random.default_rng(5)
    for pname, (gate, ops, copy, first) in gates.items():
        arena.zero_()
        gate()
        torch.cuda.synchronize()
        all_ok = bool((status == 0).all().item())
        got = arena.clone()
        ok = True
        for i in host_rng.choice(n, 24, replace=False):
            at = first + int(i) * pstride
            pkt = got[at:at + 4 + size].cpu().numpy()
            a = int(boff[i] + offset[i])
            body = images[a:a + size].cpu().numpy()
            ok = ok and np.array_equal(pkt[4:], body) and \
                int.from_bytes(bytes(pkt[:4]), "big") == \
                zlib.crc32(body.tobytes())
        arena.zero_()
        copy()
        torch.cuda.synchronize()
        d_gate = torch.as_strided(got, (n, size), (pstride, 1), first + 4)
        d_copy = torch.as_strided(arena, (n, size), (pstride, 1), first + 4)
        checks[pname] = dict(all_ok=all_ok, sample_equals_zlib=bool(ok),
                             copy_equals_gate=bool(torch.equal(d_gate,
                                                               d_copy)))
    scrub()
    torch.cuda.synchronize()
    checks["scrub_clean"] = bool((scrub_out == 0x7FFFFFFF).all().item())

    read = n * BLOCK
    out = dict(workload=name, ops=n, read_size=size, bytes_read=read,
               bytes_written=n * (4 + size), checks=checks, legs={},
               verdict={})
    for leg, s in st.items():
        out["legs"][leg] = dict(s, gbps_read=read / (s["median_ms"] / 1e3)
                                / 1e9)
    for pname, _ in PLACEMENTS:
        parts = st["scrub"]["median_ms"] + st["ranges"]["median_ms"] + \
            st["copy_" + pname]["median_ms"]
        seq = st["baseline_" + pname]
        g = st["gate_" + pname]
        out["verdict"][pname] = dict(
            baseline_sum_of_steps_ms=parts,
            baseline_sequence_ms=seq["median_ms"],
            baseline_spread=seq["spread"],
            gate_ms=g["median_ms"], gate_spread=g["spread"],
            gate_over_baseline_sum=g["median_ms"] / parts,
            gate_over_baseline_sequence=g["median_ms"] / seq["median_ms"],
            not_slower=g["median_ms"] <= parts * (1 + seq["spread"]))
    return out


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
    nimages = max(1, 128 // args.scale)              # 512 MiB of blocks
    images = build_images(nimages)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               warmup=WARMUP, calls_per_sample=INNER, images=nimages,
               blocks=nimages * PER_IMAGE)
    for name, size in (("whole_block", BLOCK), ("read_4k", 4096)):
        doc[name] = workload(lib, eng, stream, images, nimages, size,
                             args.reps, name)
        torch.cuda.empty_cache()
        for leg, x in doc[name]["legs"].items():
            print(f"read_gate_ab {name:12s} {leg:12s} {x['median_ms']:.4f} ms"
                  f" {x['gbps_read']:.0f} GB/s of blocks "
                  f"spread={x['spread']:.3f}", flush=True)
        for pname, v in doc[name]["verdict"].items():
            print(f"read_gate_ab {name:12s} {pname}: gate "
                  f"{v['gate_ms']:.4f} ms, baseline sum "
                  f"{v['baseline_sum_of_steps_ms']:.4f} ms, ratio "
                  f"{v['gate_over_baseline_sum']:.3f}", flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    ok = all(doc[w]["checks"]["scrub_clean"] and
             all(c["all_ok"] and c["sample_equals_zlib"] and
                 c["copy_equals_gate"]
                 for k, c in doc[w]["checks"].items() if k != "scrub_clean")
             for w in ("whole_block", "read_4k"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
