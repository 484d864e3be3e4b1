#!/usr/bin/env python3
"""Measure the batched chunk read against what a caller could compose without
it, on one MI355X.

All legs run in one process, after warm-up, in alternating repeats, with
device events around synchronised work; a sample is INNER back-to-back calls
between two events, divided by INNER.  The slice is ec(8,2); 16 chunks of
1024 blocks hold 1 GiB of chunk data, past the 256 MiB last-level cache.
Tables and argument arrays are built outside the timed region; a timed call
still checks, stages and uploads them, as every call does.

Whole-chunk reads, three shapes: healthy, data part 3 lost, data parts 3 and
5 lost.  Legs:

  new_*          lizec_chunk_read_batch through the C ABI
  new_healthy_py the same through chunkread.read_chunks
  base_healthy   convert.convert_parts(..., target = standard), the call the
                 parent offers for a healthy slice
  base_healthy_abi  the one lizec_ec_encode_batch_view call inside it, through
                 the C ABI with prebuilt arrays (the like-for-like of new_*)
  base_lost1/2   one lizec_ec_encode_batch_ragged call that writes chunk
                 order: dests = 8, identity rows for the surviving data parts,
                 the recovery rows for the lost ones, destination l at
                 out + l*65536, dst_block_stride = 8*65536

and one leg that only the new call can serve:

  new_read4      4096 reads of 4 blocks at random offsets of the chunks with
                 two lost parts (the composition cannot start inside a row)

convert.py, lizec_ec_encode_batch_view and lizec_ec_encode_batch_ragged are
untouched by the chunk read (it adds a kernel and a call of its own), so this
one process measures the parent's composition and the new call side by side.

Algorithmic bytes: each needed source block once, plus the output.  A row
with a lost requested column needs k = 8 source blocks, any other row only
its requested columns; for the whole-chunk shapes both come to the chunk
size, so every such leg moves 2 GiB.

Checked at the timed size: every leg's output equals the chunk data.  Prints
one JSON document (and writes it to --out).
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

from lizardfs_amd import chunkread, convert  # noqa: E402
from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd import slice_traits as st  # noqa: E402
from lizardfs_amd.ec import ReedSolomon, _pattern_table  # noqa: E402

BLOCK = 65536
K, M, NB = 8, 2, 1024
PB = NB // K                      # blocks per part
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


def p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def survivors(lost):
    """The first K parts that are left (ec_read_plan.h:126-133)."""
    return [q for q in range(K + M) if q not in lost][:K]


def recovery_rows(lost):
    """ISA-L table rows [len(lost)][K][32] over survivors(lost)."""
    srcs = survivors(lost)
    em = ((1 << (K + M)) - 1) & ~sum(1 << q for q in srcs)
    tbl, parts = _pattern_table(K, M, em, sum(1 << q for q in lost))
    assert list(parts) == sorted(lost)
    return tbl.reshape(len(lost), K, 32)


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
    EC = st.ec_slice_type(K, M)

    # ---- the chunks and their parts
    g = torch.Generator(device="cuda").manual_seed(4711)
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
    out = torch.empty((S, NB * BLOCK), dtype=torch.uint8, device="cuda")
    assert parts.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    flat = chunk.view(S, NB * BLOCK)
    rows = np.arange(S, dtype=np.uint64)

    def part_ptrs(plist):
        return np.ascontiguousarray(
            np.uint64(parts.data_ptr()) +
            np.array(plist, np.uint64)[None, :] * np.uint64(parts.stride(0)) +
            rows[:, None] * np.uint64(parts.stride(1)))

    out_ptrs = np.ascontiguousarray(
        np.uint64(out.data_ptr()) + rows * np.uint64(out.stride(0)))
    one = np.zeros(32, np.uint8)
    lib.ec_init_tables(1, 1, p(np.ones(1, np.uint8), u8p), p(one, u8p))

    # ---- the new call
    def make_new(lost, first=None, count=None, dst=None, sel=None):
        srcs = survivors(lost) if lost else list(range(K))
        cmap = np.array([srcs.index(c) if c in srcs
                         else chunkread.LOST + sorted(lost).index(c)
                         for c in range(K)], np.uint8)
        tbl = np.ascontiguousarray(recovery_rows(lost)) if lost else None
        sp = part_ptrs(srcs)
        if sel is not None:
            sp = np.ascontiguousarray(sp[sel])
        R = sp.shape[0]
        nb = np.full((R, K), PB, np.uint32)
        cm = np.ascontiguousarray(np.tile(cmap, (R, 1)))
        first = np.zeros(R, np.uint32) if first is None else first
        count = np.full(R, NB, np.uint32) if count is None else count
        dst = out_ptrs if dst is None else dst

        def call():
            L.check(lib.lizec_chunk_read_batch(
                eng, K, len(lost), p(tbl, u8p), 1 if lost else 0, None,
                p(sp, u64p), p(nb, u32p), K, p(cm, u8p), p(first, u32p),
                p(count, u32p), p(dst, u64p), R, BLOCK, BLOCK, stream))
        return call

    # ---- the parent's compositions
    frags = [parts[q] for q in range(K + M)]
    out3 = out.view(S, 1, NB * BLOCK)

    def base_healthy():
        convert.convert_parts(EC, frags, [NB] * S, st.K_STANDARD, {0},
                              out=out3)

    view = part_ptrs(list(range(K)))
    cb = np.full(S, NB, np.uint32)
    zeros = np.zeros(S, np.uint32)

    def base_healthy_abi():
        L.check(lib.lizec_ec_encode_batch_view(
            eng, 1, 1, p(one, u8p), 1, p(zeros, u32p), p(view, u64p), K,
            p(cb, u32p), 1, p(zeros, u32p), p(out_ptrs, u64p), p(cb, u32p),
            S, BLOCK, BLOCK, stream))

    def make_ragged(lost):
        srcs = survivors(lost)
        rec = recovery_rows(lost)
        tbl = np.zeros((K, K, 32), np.uint8)        # [dest column][slot]
        for c in range(K):
            if c in lost:
                tbl[c] = rec[sorted(lost).index(c)]
            else:
                tbl[c, srcs.index(c)] = one
        sp = part_ptrs(srcs)
        nb = np.full((S, K), PB, np.uint32)
        dp = np.ascontiguousarray(
            out_ptrs[:, None] + np.arange(K, dtype=np.uint64)[None, :] *
            np.uint64(BLOCK))

        def call():
            L.check(lib.lizec_ec_encode_batch_ragged(
                eng, K, K, p(tbl, u8p), 1, None, p(sp, u64p), p(nb, u32p),
                p(dp, u64p), p(nb, u32p), S, BLOCK, K * BLOCK, stream))
        return call

    # ---- 4-block reads at random offsets of the chunks with two lost parts
    rng = np.random.default_rng(99)
    R4 = S * 256
    sel4 = np.repeat(np.arange(S), 256)
    first4 = rng.integers(0, NB - 3, R4).astype(np.uint32)
    count4 = np.full(R4, 4, np.uint32)
    out4 = torch.empty((R4, 4 * BLOCK), dtype=torch.uint8, device="cuda")
    dst4 = np.ascontiguousarray(
        np.uint64(out4.data_ptr()) +
        np.arange(R4, dtype=np.uint64) * np.uint64(out4.stride(0)))
    read4 = make_new((3, 5), first4, count4, dst4, sel4)
    # its algorithmic source blocks, row by row
    need4 = 0
    for f in first4.tolist():
        for b in range(f // K, (f + 3) // K + 1):
            cols = [c for c in range(K) if f <= b * K + c < f + 4]
            need4 += K if (3 in cols or 5 in cols) else len(cols)

    def new_healthy_py():
        chunkread.read_chunks(EC, frags, [NB] * S, 0, NB, out=out)

    legs = [("new_healthy", make_new(())), ("new_healthy_py", new_healthy_py),
            ("base_healthy", base_healthy),
            ("base_healthy_abi", base_healthy_abi),
            ("new_lost1", make_new((3,))), ("base_lost1", make_ragged((3,))),
            ("new_lost2", make_new((3, 5))),
            ("base_lost2", make_ragged((3, 5))), ("new_read4", read4)]

    # ---- checks at the timed size, before and after timing
    def check_all():
        res = {}
        for name, fn in legs:
            tgt = out4 if name == "new_read4" else out
            tgt.fill_(0xA5)
            fn()
            torch.cuda.synchronize()
            if name == "new_read4":
                idx = torch.from_numpy(first4.astype(np.int64)).cuda()[:, None] \
                    + torch.arange(4, device="cuda")[None, :]
                exp = chunk[torch.from_numpy(sel4).cuda()[:, None], idx]
                res[name] = bool(torch.equal(out4.view(R4, 4, BLOCK), exp))
                del exp
            else:
                res[name] = bool(torch.equal(out, flat))
        return res

    checks = check_all()
    st_ = time_legs(legs, args.reps)
    checks_after = check_all()

    whole = 2 * S * NB * BLOCK
    bytes_of = {name: whole for name, _ in legs}
    bytes_of["new_read4"] = (need4 + 4 * R4) * BLOCK
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               warmup=WARMUP, calls_per_sample=INNER, slice="ec(8,2)",
               chunks=S, blocks_per_chunk=NB, chunk_bytes=S * NB * BLOCK,
               reads4=R4, checks=checks, checks_after=checks_after, legs={},
               verdict={})
    for name, s in st_.items():
        gbps = bytes_of[name] / (s["median_ms"] / 1e3) / 1e9
        doc["legs"][name] = dict(s, algorithmic_bytes=bytes_of[name],
                                 gbps=gbps, hbm_share=gbps * 1e9 / HBM_PEAK)
        print(f"chunk_read_ab {name:18s} {s['median_ms']:.4f} ms "
              f"{gbps:.0f} GB/s ({100 * gbps * 1e9 / HBM_PEAK:.1f}% of peak) "
              f"spread={s['spread']:.3f}", flush=True)
    for shape, new, base in (
            ("healthy", "new_healthy", "base_healthy"),
            ("healthy_like_for_like", "new_healthy", "base_healthy_abi"),
            ("healthy_through_python", "new_healthy_py", "base_healthy"),
            ("lost1", "new_lost1", "base_lost1"),
            ("lost2", "new_lost2", "base_lost2")):
        n, b = st_[new], st_[base]
        spread_ms = max(n["max_ms"] - n["min_ms"], b["max_ms"] - b["min_ms"])
        doc["verdict"][shape] = dict(
            new_ms=n["median_ms"], baseline=base, baseline_ms=b["median_ms"],
            ratio=n["median_ms"] / b["median_ms"], sample_spread_ms=spread_ms,
            faster_by_more_than_spread=b["median_ms"] - n["median_ms"] >
            spread_ms)
        print(f"chunk_read_ab {shape}: new {n['median_ms']:.4f} ms, {base} "
              f"{b['median_ms']:.4f} ms, ratio "
              f"{n['median_ms'] / b['median_ms']:.3f}", flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if all(checks.values()) and all(checks_after.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
