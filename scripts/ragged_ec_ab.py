#!/usr/bin/env python3
"""A/B the ragged EC call (lizec_ec_encode_batch_ragged) on one MI355X.

(a) Uniform lengths: ec(8,2) and ec(16,4) encode over device-resident 8 MiB
    parts (128 blocks), the shapes of scripts/strided_ec_ab.py.  Legs:
      uniform      lizec_ec_encode_batch, contiguous aligned parts;
      strided      lizec_ec_encode_batch_strided, the al-strided layout
                   (65552 / 65600, every address 16-byte aligned);
      ragged       the ragged call on the same al-strided buffers, every
                   count = 128;
      ragged-flat  the ragged call on the uniform leg's contiguous buffers.
(b) Ragged populations from a fixed seed, ec(8,2) encode, parts packed back
    to back (contiguous, aligned):
      pop1   256 chunks, chunk_blocks uniform in 1..1024;
      pop2   16384 chunks of 1..8 blocks.
    Legs:
      ragged   one ragged call for the whole population;
      grouped  what a caller had to do before: per distinct chunk length one
               lizec_ec_encode_batch over the full stripe rows, plus a
               second one over the short last row with the table of its
               fewer non-NULL sources (lizec_rs_tables nonnull mask).
All legs of a case run in one process, after warm-up, in alternating rounds,
with device events around the calls of a sample.  Outputs are compared
byte for byte between the legs at the timed size.  Prints one JSON document
(and writes it to --out).
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
from lizardfs_amd import slice_traits as st  # noqa: E402

BLOCK = 65536
WARMUP = 2

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


def fill_random(buf, seed):
    """Random bytes from a 64 MiB tile (the content does not matter to the
    timing, only that it is not constant)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    tile = torch.randint(0, 256, (min(buf.numel(), 1 << 26),),
                         dtype=torch.uint8, device="cuda", generator=g)
    for at in range(0, buf.numel(), tile.numel()):
        n = min(tile.numel(), buf.numel() - at)
        buf[at:at + n] = tile[:n]


class Parts:
    """n parts of nblocks blocks at `stride`, slots packed back to back."""

    def __init__(self, n, nblocks, stride):
        self.n, self.nblocks, self.stride = n, nblocks, stride
        self.slot = nblocks * stride
        self.buf = torch.zeros(n * self.slot, dtype=torch.uint8,
                               device="cuda")
        self.ptrs = (np.uint64(self.buf.data_ptr()) +
                     np.arange(n, dtype=np.uint64) * np.uint64(self.slot))

    def blocks(self):
        return self.buf.view(self.n, self.nblocks, self.stride)[:, :, :BLOCK]


def run_uniform_shape(lib, eng, k, m, S, nblocks, reps, inner):
    tbl = np.zeros(32 * k * m, np.uint8)
    L.check(lib.lizec_rs_encode_tables(k, m, p8(tbl)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat_src = Parts(S * k, nblocks, BLOCK)
    fill_random(flat_src.buf, 7)
    al_src = Parts(S * k, nblocks, 65552)
    al_src.blocks().copy_(flat_src.blocks())
    dsts = dict(uniform=Parts(S * m, nblocks, BLOCK),
                strided=Parts(S * m, nblocks, 65600),
                ragged=Parts(S * m, nblocks, 65600))
    dsts["ragged-flat"] = Parts(S * m, nblocks, BLOCK)
    snb = np.full(S * k, nblocks, np.uint32)
    dnb = np.full(S * m, nblocks, np.uint32)

    def uniform():
        L.check(lib.lizec_ec_encode_batch(
            eng, nblocks * BLOCK, k, m, p8(tbl), p64(flat_src.ptrs),
            p64(dsts["uniform"].ptrs), S, stream))

    def strided():
        L.check(lib.lizec_ec_encode_batch_strided(
            eng, nblocks, k, m, p8(tbl), p64(al_src.ptrs),
            p64(dsts["strided"].ptrs), S, 65552, 65600, stream))

    def ragged():
        L.check(lib.lizec_ec_encode_batch_ragged(
            eng, k, m, p8(tbl), 1, None, p64(al_src.ptrs), p32(snb),
            p64(dsts["ragged"].ptrs), p32(dnb), S, 65552, 65600, stream))

    def ragged_flat():
        L.check(lib.lizec_ec_encode_batch_ragged(
            eng, k, m, p8(tbl), 1, None, p64(flat_src.ptrs), p32(snb),
            p64(dsts["ragged-flat"].ptrs), p32(dnb), S, BLOCK, BLOCK, stream))

    legs = [("uniform", uniform), ("strided", strided), ("ragged", ragged),
            ("ragged-flat", ragged_flat)]
    stt = time_legs(legs, reps, inner)
    moved = S * nblocks * BLOCK * (k + m)
    ref = dsts["uniform"].blocks()
    report = dict(k=k, m=m, stripes=S, nblocks=nblocks, bytes_moved=moved,
                  reps=reps, warmup=WARMUP, calls_per_sample=inner, legs={})
    for name, _ in legs:
        report["legs"][name] = dict(
            stt[name], gbps=moved / (stt[name]["median_ms"] / 1e3) / 1e9,
            over_uniform=stt["uniform"]["median_ms"] / stt[name]["median_ms"],
            over_strided=stt["strided"]["median_ms"] / stt[name]["median_ms"],
            equals_uniform=bool(torch.equal(dsts[name].blocks(), ref)))
    return report


def run_population(lib, eng, name, k, m, chunk_blocks, reps, inner):
    t = st.ec_slice_type(k, m)
    S = len(chunk_blocks)
    pb = np.array([[st.number_of_blocks(t, p, int(n)) for p in range(k + m)]
                   for n in chunk_blocks], np.int64)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # parts packed back to back, chunk-major
    soff = np.concatenate([[0], np.cumsum(pb[:, :k].ravel())[:-1]])
    doff = np.concatenate([[0], np.cumsum(pb[:, k:].ravel())[:-1]])
    src = torch.empty(int(pb[:, :k].sum()) * BLOCK, dtype=torch.uint8,
                      device="cuda")
    fill_random(src, 11)
    ndst = int(pb[:, k:].sum()) * BLOCK
    out = {leg: torch.zeros(ndst, dtype=torch.uint8, device="cuda")
           for leg in ("ragged", "grouped")}
    sp = (np.uint64(src.data_ptr()) +
          soff.astype(np.uint64) * np.uint64(BLOCK)).reshape(S, k)
    dp = {leg: (np.uint64(o.data_ptr()) + doff.astype(np.uint64) *
                np.uint64(BLOCK)).reshape(S, m) for leg, o in out.items()}
    snb = np.ascontiguousarray(pb[:, :k].astype(np.uint32))
    dnb = np.ascontiguousarray(pb[:, k:].astype(np.uint32))
    tbl = np.zeros(32 * k * m, np.uint8)
    L.check(lib.lizec_rs_encode_tables(k, m, p8(tbl)))
    rsp = np.ascontiguousarray(np.where(snb > 0, sp, np.uint64(0)))
    rdp = np.ascontiguousarray(dp["ragged"])

    def ragged():
        L.check(lib.lizec_ec_encode_batch_ragged(
            eng, k, m, p8(tbl), 1, None, p64(rsp), p32(snb), p64(rdp),
            p32(dnb), S, BLOCK, BLOCK, stream))

    # the grouped leg's calls, prepared outside the timed region
    data_mask = (1 << k) - 1
    par_mask = ((1 << m) - 1) << k
    calls = []
    for n in sorted(set(int(x) for x in chunk_blocks)):
        idx = np.flatnonzero(np.asarray(chunk_blocks) == n)
        rows, rem = divmod(n, k)
        if rows:
            calls.append((rows * BLOCK, k, tbl,
                          np.ascontiguousarray(sp[idx].ravel()),
                          np.ascontiguousarray(dp["grouped"][idx].ravel()),
                          len(idx)))
        if rem:
            short = np.zeros(32 * rem * m, np.uint8)
            ic, oc = ctypes.c_int(), ctypes.c_int()
            L.check(lib.lizec_rs_tables(k, m, data_mask, (1 << rem) - 1,
                                        par_mask, p8(short),
                                        ctypes.byref(ic), ctypes.byref(oc)))
            assert (ic.value, oc.value) == (rem, m)
            at = np.uint64(rows * BLOCK)
            calls.append((BLOCK, rem, short,
                          np.ascontiguousarray((sp[idx, :rem] + at).ravel()),
                          np.ascontiguousarray(
                              (dp["grouped"][idx] + at).ravel()), len(idx)))

    def grouped():
        for plen, srcs, tb, s_, d_, ns in calls:
            L.check(lib.lizec_ec_encode_batch(eng, plen, srcs, m, p8(tb),
                                              p64(s_), p64(d_), ns, stream))

    legs = [("ragged", ragged), ("grouped", grouped)]
    stt = time_legs(legs, reps, inner)
    moved = int(pb.sum()) * BLOCK
    same = bool(torch.equal(out["ragged"], out["grouped"]))
    nonzero = bool(out["ragged"].any())
    report = dict(population=name, k=k, m=m, chunks=S,
                  distinct_lengths=len(set(int(x) for x in chunk_blocks)),
                  grouped_calls=len(calls), bytes_moved=moved, reps=reps,
                  warmup=WARMUP, calls_per_sample=inner,
                  outputs_identical=same and nonzero, legs={})
    for leg, _ in legs:
        report["legs"][leg] = dict(
            stt[leg], gbps=moved / (stt[leg]["median_ms"] / 1e3) / 1e9,
            over_grouped=stt["grouped"]["median_ms"] / stt[leg]["median_ms"])
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1,
                    help="divide stripe and chunk counts (quick dry runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    lib, eng = L.lib(), L.engine(0)
    doc = dict(device=torch.cuda.get_device_name(0), uniform=[],
               populations=[])
    ok = True
    for k, m, S in ((8, 2, 16), (16, 4, 8)):
        r = run_uniform_shape(lib, eng, k, m, max(1, S // args.scale), 128,
                              args.reps, 20)
        doc["uniform"].append(r)
        for name, x in r["legs"].items():
            ok &= x["equals_uniform"]
            print(f"ragged_ab ec({k},{m}) {name:11s} {x['median_ms']:.3f} ms "
                  f"{x['gbps']:.0f} GB/s x{x['over_strided']:.3f} of strided "
                  f"x{x['over_uniform']:.3f} of uniform "
                  f"spread={x['spread']:.3f} same={x['equals_uniform']}",
                  flush=True)
        torch.cuda.empty_cache()
    rng = np.random.default_rng(20240)
    pops = (("pop1", rng.integers(1, 1025, max(1, 256 // args.scale)), 3),
            ("pop2", rng.integers(1, 9, max(1, 16384 // args.scale)), 5))
    for name, cb, inner in pops:
        r = run_population(lib, eng, name, 8, 2, cb, args.reps, inner)
        doc["populations"].append(r)
        ok &= r["outputs_identical"]
        for leg, x in r["legs"].items():
            print(f"ragged_ab {name} {leg:8s} {x['median_ms']:.3f} ms "
                  f"{x['gbps']:.0f} GB/s x{x['over_grouped']:.3f} of grouped "
                  f"spread={x['spread']:.3f} "
                  f"calls={1 if leg == 'ragged' else r['grouped_calls']} "
                  f"same={r['outputs_identical']}", flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
