#!/usr/bin/env python3
"""A/B the chunk-view EC call (lizec_ec_encode_batch_view) on one MI355X.

Target slices ec(8,2) (16 chunks) and ec(16,4) (8 chunks), parity parts
wanted, 8 MiB target parts (128 block rows), everything device-resident,
contiguous and 16-byte aligned.  The same chunk bytes are laid out three
ways and every leg computes the same parity:
  ragged        lizec_ec_encode_batch_ragged over the chunk already stored as
                the target slice (k parts of 128 blocks): the yardstick;
  view-std      the view call, view_parts = 1 (a standard copy);
  view-ec3      the view call, view_parts = 3 (an ec(3,m) slice);
  per-row       the view-ec3 conversion emulated with the ragged call: one
                "stripe" per block row, its k source addresses walking the
                three parts; metadata built outside the timed region;
  per-row+meta  the same with the metadata built inside it (numpy, then
                the call), every call.
All legs run in one process, after 2 warm-up rounds, in 10 alternating
rounds, with device events around the calls of a sample (an event pair
spans the host work between them too).  Outputs are compared byte for byte
at the timed size.  Prints one JSON document (and writes it to --out).
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
ROWS = 128

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def p8(a):
    return a.ctypes.data_as(u8p)


def p32(a):
    return a.ctypes.data_as(u32p)


def p64(a):
    return a.ctypes.data_as(u64p)


def stats(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms),
                spread=(max(ms) - min(ms)) / med, samples_ms=ms)


def time_legs(legs, reps, inner):
    """legs: [(name, fn)] -> {name: stats}; rounds alternate the legs."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in legs}
    for rep in range(WARMUP + reps):
        for name, fn in legs:
            torch.cuda.synchronize()
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(e0.elapsed_time(e1) / inner)
    return {name: stats(ms) for name, ms in times.items()}


def split(chunks, k):
    """chunks [S, n, BLOCK] -> [S, k, n / k, BLOCK]: part c % k, block
    c // k (n a multiple of k, or padded with blocks nobody reads)."""
    S, n, _ = chunks.shape
    per = -(-n // k)
    out = torch.zeros((S, k, per, BLOCK), dtype=torch.uint8, device="cuda")
    for p in range(k):
        mine = chunks[:, p::k]
        out[:, p, :mine.shape[1]] = mine
    return out


def row_ptrs(base3, per3, S, k):
    """Source addresses [S * ROWS, k] of the per-row emulation over the
    three-part layout."""
    c = (np.arange(ROWS, dtype=np.uint64)[:, None] * np.uint64(k) +
         np.arange(k, dtype=np.uint64)[None, :])                # [ROWS, k]
    off = ((c % np.uint64(3)) * np.uint64(per3) + c // np.uint64(3)) * \
        np.uint64(BLOCK)
    chunk0 = np.arange(S, dtype=np.uint64) * np.uint64(3 * per3 * BLOCK)
    return np.ascontiguousarray(
        (np.uint64(base3) + chunk0[:, None, None] + off[None]).reshape(-1, k))


def run_shape(lib, eng, k, m, S, reps, inner):
    n = k * ROWS
    tbl = np.zeros(32 * k * m, np.uint8)
    L.check(lib.lizec_rs_encode_tables(k, m, p8(tbl)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(13)
    tile = torch.randint(0, 256, (1 << 26,), dtype=torch.uint8, device="cuda",
                         generator=g)
    chunks = tile.repeat(-(-S * n * BLOCK // tile.numel()))[:S * n * BLOCK]
    chunks = chunks.view(S, n, BLOCK).contiguous()
    as_target = split(chunks, k)
    as_ec3 = split(chunks, 3)
    per3 = as_ec3.shape[2]
    del tile
    names = ("ragged", "view-std", "view-ec3", "per-row", "per-row+meta")
    dst = {leg: torch.zeros((S, m, ROWS * BLOCK), dtype=torch.uint8,
                            device="cuda") for leg in names}

    def dptr(t, count, step):
        return (np.uint64(t.data_ptr()) +
                np.arange(count, dtype=np.uint64) * np.uint64(step))

    dp = {leg: dptr(d, S * m, ROWS * BLOCK) for leg, d in dst.items()}
    dnb = np.full(S * m, ROWS, np.uint32)
    cb = np.full(S, n, np.uint32)
    sp_t = dptr(as_target, S * k, ROWS * BLOCK)
    snb = np.full(S * k, ROWS, np.uint32)
    vp_std = dptr(chunks, S, n * BLOCK)
    vp_ec3 = dptr(as_ec3, S * 3, per3 * BLOCK)

    def ragged():
        L.check(lib.lizec_ec_encode_batch_ragged(
            eng, k, m, p8(tbl), 1, None, p64(sp_t), p32(snb),
            p64(dp["ragged"]), p32(dnb), S, BLOCK, BLOCK, stream))

    def view(leg, vp, ks):
        def fn():
            L.check(lib.lizec_ec_encode_batch_view(
                eng, k, m, p8(tbl), 1, None, p64(vp), ks, p32(cb), k, None,
                p64(dp[leg]), p32(dnb), S, BLOCK, BLOCK, stream))
        return fn

    def row_meta(leg):
        sp = row_ptrs(as_ec3.data_ptr(), per3, S, k)
        rows = np.arange(ROWS, dtype=np.uint64) * np.uint64(BLOCK)
        rdp = np.ascontiguousarray(
            (dp[leg].reshape(S, 1, m) + rows[None, :, None]).reshape(-1, m))
        return (sp, np.ones(sp.shape, np.uint32), rdp,
                np.ones(rdp.shape, np.uint32))

    def row_call(meta):
        sp, sn, rdp, rdn = meta
        L.check(lib.lizec_ec_encode_batch_ragged(
            eng, k, m, p8(tbl), 1, None, p64(sp), p32(sn), p64(rdp),
            p32(rdn), S * ROWS, BLOCK, BLOCK, stream))

    fixed = row_meta("per-row")
    legs = [("ragged", ragged), ("view-std", view("view-std", vp_std, 1)),
            ("view-ec3", view("view-ec3", vp_ec3, 3)),
            ("per-row", lambda: row_call(fixed)),
            ("per-row+meta", lambda: row_call(row_meta("per-row+meta")))]
    stt = time_legs(legs, reps, inner)
    moved = S * ROWS * BLOCK * (k + m)
    meta_bytes = sum(a.nbytes for a in fixed)
    ref = dst["ragged"]
    report = dict(k=k, m=m, chunks=S, chunk_blocks=n, bytes_moved=moved,
                  per_row_metadata_bytes=meta_bytes, reps=reps, warmup=WARMUP,
                  calls_per_sample=inner, legs={})
    for name, _ in legs:
        report["legs"][name] = dict(
            stt[name], gbps=moved / (stt[name]["median_ms"] / 1e3) / 1e9,
            over_ragged=stt["ragged"]["median_ms"] / stt[name]["median_ms"],
            equals_ragged=bool(torch.equal(dst[name], ref)) and
            bool(ref.any()))
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1,
                    help="divide the chunk counts (quick dry runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    lib, eng = L.lib(), L.engine(0)
    doc = dict(device=torch.cuda.get_device_name(0), shapes=[])
    ok = True
    for k, m, S in ((8, 2, 16), (16, 4, 8)):
        r = run_shape(lib, eng, k, m, max(1, S // args.scale), args.reps, 20)
        doc["shapes"].append(r)
        for name, x in r["legs"].items():
            ok &= x["equals_ragged"]
            print(f"reslice_ab ec({k},{m}) {name:12s} {x['median_ms']:.3f} ms "
                  f"{x['gbps']:.0f} GB/s x{x['over_ragged']:.3f} of ragged "
                  f"spread={x['spread']:.3f} same={x['equals_ragged']}",
                  flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
