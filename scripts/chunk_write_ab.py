#!/usr/bin/env python3
"""Measure the batched chunk write on one MI355X.

All legs run in one process, after warm-up, in alternating repeats, with
device events around synchronised work; a sample is INNER back-to-back calls
between two events, divided by INNER.  The slice is ec(8,2); 16 chunks of
1024 blocks hold 1 GiB of chunk data, past the 256 MiB last-level cache.
Tables and argument arrays are built outside the timed region; a timed call
still checks, stages and uploads them, as every call does.

  (a) whole-chunk, whole-block, aligned writes: one write per chunk of all
      1024 blocks, no fill, parity in place into the parity parts, every
      packet's CRC.
        new_whole    lizec_chunk_write_batch (the aligned kernel form)
        base_whole   what the parent offers for the same bytes: one
                     lizec_ec_encode_batch_view call over the chunk as a
                     standard view for the parity, lizec_crc32_batch over the
                     data and over the parity
        new_whole_parity / base_whole_parity
                     the same with no CRCs asked (crcs = 0) against the view
                     call alone: the parity kernels side by side
  (b) new_write4   4096 writes of 4 whole blocks at random block offsets:
      the rows they touch in part are filled from the data parts
  (c) new_sub4k    4096 writes of 4 KiB into one block each, at odd `from`,
      odd data addresses and packet-compact odd parity addresses: the
      general kernel form

(b) and (c) have no baseline: the parent has no call that starts inside a
row or inside a block.

Algorithmic bytes: each needed source byte once (new data and fill), plus
the parity written.  Checked at the timed size, before and after timing:
(a) parity and CRCs equal those of the baseline composition, which the
suite checks against the oracle; (b) and (c) equal the host twin
(lizec_chunk_write_host) over the same bytes.  Prints one JSON document
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

from lizardfs_amd import chunkwrite  # noqa: E402
from lizardfs_amd import lib as L  # noqa: E402
from lizardfs_amd import slice_traits as st  # noqa: E402

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
    tbl = chunkwrite.encode_table(st.ec_slice_type(K, M))

    g = torch.Generator(device="cuda").manual_seed(4712)
    chunk = torch.randint(0, 256, (S, NB, BLOCK), dtype=torch.uint8,
                          device="cuda", generator=g)
    # the data parts as they are on the chunkservers (the fill of leg b)
    parts = torch.empty((K, S, PB * BLOCK), dtype=torch.uint8, device="cuda")
    for d in range(K):
        parts[d].view(S, PB, BLOCK).copy_(chunk[:, d::K])
    par_new = torch.empty((M, S, PB * BLOCK), dtype=torch.uint8,
                          device="cuda")
    par_base = torch.empty_like(par_new)
    ncrc = NB + PB * M
    crc_new = torch.empty((S, ncrc), dtype=torch.int32, device="cuda")
    crc_base_d = torch.empty((S * NB,), dtype=torch.int32, device="cuda")
    crc_base_p = torch.empty((M * S * PB,), dtype=torch.int32, device="cuda")
    rows = np.arange(S, dtype=np.uint64)

    def call_new(wr, fp, fn, pp):
        L.check(lib.lizec_chunk_write_batch(
            eng, M, p(tbl, u8p), ctypes.c_void_p(wr.ctypes.data), len(wr),
            p(fp, u64p), p(fn, u32p), K, BLOCK, p(pp, u64p), stream))

    # ---- (a) whole chunks
    wr_a = np.zeros(S, chunkwrite.WRITE_DTYPE)
    wr_a["data"] = np.uint64(chunk.data_ptr()) + rows * np.uint64(NB * BLOCK)
    wr_a["crcs"] = np.uint64(crc_new.data_ptr()) + rows * np.uint64(4 * ncrc)
    wr_a["data_stride"] = wr_a["par_stride"] = BLOCK
    wr_a["block_count"], wr_a["to"] = NB, BLOCK
    wr_a0 = wr_a.copy()
    wr_a0["crcs"] = 0
    nofill_p = np.zeros((S, K), np.uint64)
    nofill_n = np.zeros((S, K), np.uint32)

    def par_ptrs(t):
        return np.ascontiguousarray(
            np.uint64(t.data_ptr()) +
            np.arange(M, dtype=np.uint64)[None, :] * np.uint64(t.stride(0)) +
            rows[:, None] * np.uint64(t.stride(1)))

    pp_new, pp_base = par_ptrs(par_new), par_ptrs(par_base)

    def new_whole():
        call_new(wr_a, nofill_p, nofill_n, pp_new)

    def new_whole_parity():
        call_new(wr_a0, nofill_p, nofill_n, pp_new)

    view = np.ascontiguousarray(wr_a["data"].reshape(S, 1))
    cb = np.full(S, NB, np.uint32)
    dnb = np.full((S, M), PB, np.uint32)

    def base_whole_parity():
        L.check(lib.lizec_ec_encode_batch_view(
            eng, K, M, p(tbl, u8p), 1, None, p(view, u64p), 1, p(cb, u32p),
            K, None, p(pp_base, u64p), p(dnb, u32p), S, BLOCK, BLOCK, stream))

    def base_whole():
        base_whole_parity()
        L.check(lib.lizec_crc32_batch(
            eng, ctypes.c_void_p(chunk.data_ptr()), BLOCK, S * NB, 0,
            ctypes.c_void_p(crc_base_d.data_ptr()), stream))
        L.check(lib.lizec_crc32_batch(
            eng, ctypes.c_void_p(par_base.data_ptr()), BLOCK, M * S * PB, 0,
            ctypes.c_void_p(crc_base_p.data_ptr()), stream))

    # ---- (b) 4-block writes at random block offsets, (c) 4 KiB sub-block
    rng = np.random.default_rng(98)
    W = S * 256
    sel = np.repeat(np.arange(S), 256).astype(np.uint64)
    fill_p = np.ascontiguousarray(
        np.uint64(parts.data_ptr()) +
        np.arange(K, dtype=np.uint64)[None, :] * np.uint64(parts.stride(0)) +
        sel[:, None] * np.uint64(parts.stride(1)))
    fill_n = np.full((W, K), PB, np.uint32)

    def writes(first, count, frm, size, data, data_stride, par, par_stride,
               crcs, ncrcs):
        wr = np.zeros(W, chunkwrite.WRITE_DTYPE)
        idx = np.arange(W, dtype=np.uint64)
        wr["data"] = np.uint64(data.data_ptr()) + idx * \
            np.uint64(data.stride(0))
        wr["crcs"] = np.uint64(crcs.data_ptr()) + idx * np.uint64(4 * ncrcs)
        wr["data_stride"], wr["par_stride"] = data_stride, par_stride
        wr["first_block"], wr["block_count"] = first, count
        wr["from"], wr["to"] = frm, frm + size
        pp = np.ascontiguousarray(
            np.uint64(par.data_ptr()) + idx[:, None] *
            np.uint64(par.stride(0)) +
            np.arange(M, dtype=np.uint64)[None, :] * np.uint64(par.stride(1)))
        return wr, pp

    first4 = rng.integers(0, NB - 3, W).astype(np.uint32)
    data4 = torch.randint(0, 256, (W, 4 * BLOCK), dtype=torch.uint8,
                          device="cuda", generator=g)
    par4 = torch.empty((W, M, 2 * BLOCK), dtype=torch.uint8, device="cuda")
    crc4 = torch.empty((W, 4 + 2 * M), dtype=torch.int32, device="cuda")
    wr_b, pp_b = writes(first4, 4, 0, BLOCK, data4, BLOCK, par4, BLOCK, crc4,
                        4 + 2 * M)
    touched4 = (first4 + 3) // K - first4 // K + 1
    # a touched row reads its K columns once, new or fill
    bytes_b = int(touched4.sum()) * (K + M) * BLOCK

    SUB = 4096
    first_c = rng.integers(0, NB, W).astype(np.uint32)
    from_c = (rng.integers(0, (BLOCK - SUB) // 2, W) * 2 + 1).astype(np.uint32)
    data_c = torch.randint(0, 256, (W, SUB + 34), dtype=torch.uint8,
                           device="cuda", generator=g)
    par_c = torch.empty((W, M, SUB + 18), dtype=torch.uint8, device="cuda")
    crc_c = torch.empty((W, 1 + M), dtype=torch.int32, device="cuda")
    wr_c, pp_c = writes(first_c, 1, from_c, SUB, data_c, SUB, par_c, SUB,
                        crc_c, 1 + M)
    wr_c["data"] += 1 + 2 * (np.arange(W, dtype=np.uint64) % 8)     # odd
    pp_c += np.uint64(1) + np.uint64(2) * \
        (np.arange(W, dtype=np.uint64)[:, None] % np.uint64(8))
    bytes_c = W * (K + M) * SUB

    def new_write4():
        call_new(wr_b, fill_p, fill_n, pp_b)

    def new_sub4k():
        call_new(wr_c, fill_p, fill_n, pp_c)

    legs = [("new_whole", new_whole), ("base_whole", base_whole),
            ("new_whole_parity", new_whole_parity),
            ("base_whole_parity", base_whole_parity),
            ("new_write4", new_write4), ("new_sub4k", new_sub4k)]

    # ---- checks at the timed size
    twins = {}

    def host_twin(name, wr, pp, data, par, crcs):
        """The same call through lizec_chunk_write_host over host copies;
        the inputs do not change, so it is computed once per leg."""
        if name in twins:
            return twins[name]
        h_parts, h_data = parts.cpu().numpy(), data.cpu().numpy()
        h_par = np.full(tuple(par.shape), 0xA5, np.uint8)
        h_crc = np.zeros(tuple(crcs.shape), np.uint32)
        w2 = wr.copy()
        w2["data"] = wr["data"] - np.uint64(data.data_ptr()) + \
            np.uint64(h_data.ctypes.data)
        w2["crcs"] = wr["crcs"] - np.uint64(crcs.data_ptr()) + \
            np.uint64(h_crc.ctypes.data)
        f2 = fill_p - np.uint64(parts.data_ptr()) + \
            np.uint64(h_parts.ctypes.data)
        p2 = pp - np.uint64(par.data_ptr()) + np.uint64(h_par.ctypes.data)
        L.check(lib.lizec_chunk_write_host(
            M, p(tbl, u8p), ctypes.c_void_p(w2.ctypes.data), len(w2),
            p(f2, u64p), p(fill_n, u32p), K, BLOCK, p(p2, u64p)))
        twins[name] = h_par, h_crc
        return twins[name]

    def check_all():
        res = {}
        for t in (par_new, par_base, par4, par_c):
            t.fill_(0xA5)
        for t in (crc_new, crc_base_d, crc_base_p, crc4, crc_c):
            t.zero_()
        new_whole()
        base_whole()
        torch.cuda.synchronize()
        res["whole_parity"] = bool(torch.equal(par_new, par_base))
        res["whole_data_crcs"] = bool(torch.equal(
            crc_new[:, :NB].reshape(-1), crc_base_d))
        # crcs[NB + i*M + r] against the baseline's [r][chunk][i]
        res["whole_parity_crcs"] = bool(torch.equal(
            crc_new[:, NB:].view(S, PB, M).permute(2, 0, 1).reshape(-1),
            crc_base_p))
        par_new.fill_(0xA5)
        new_whole_parity()
        torch.cuda.synchronize()
        res["whole_parity_alone"] = bool(torch.equal(par_new, par_base))
        for name, fn, wr, pp, data, par, crcs in (
                ("write4", new_write4, wr_b, pp_b, data4, par4, crc4),
                ("sub4k", new_sub4k, wr_c, pp_c, data_c, par_c, crc_c)):
            fn()
            torch.cuda.synchronize()
            h_par, h_crc = host_twin(name, wr, pp, data, par, crcs)
            res[name + "_parity"] = bool(
                np.array_equal(par.cpu().numpy(), h_par))
            res[name + "_crcs"] = bool(np.array_equal(
                crcs.cpu().numpy().view(np.uint32), h_crc))
        return res

    checks = check_all()
    st_ = time_legs(legs, args.reps)
    checks_after = check_all()

    whole = S * NB * BLOCK + M * S * PB * BLOCK
    bytes_of = dict(new_whole=whole, base_whole=whole, new_whole_parity=whole,
                    base_whole_parity=whole, new_write4=bytes_b,
                    new_sub4k=bytes_c)
    doc = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               warmup=WARMUP, calls_per_sample=INNER, slice="ec(8,2)",
               chunks=S, blocks_per_chunk=NB, chunk_bytes=S * NB * BLOCK,
               writes4=W, sub_writes=W, sub_bytes=SUB, checks=checks,
               checks_after=checks_after, legs={}, verdict={})
    for name, s in st_.items():
        gbps = bytes_of[name] / (s["median_ms"] / 1e3) / 1e9
        doc["legs"][name] = dict(s, algorithmic_bytes=bytes_of[name],
                                 gbps=gbps, hbm_share=gbps * 1e9 / HBM_PEAK)
        print(f"chunk_write_ab {name:18s} {s['median_ms']:.4f} ms "
              f"{gbps:.0f} GB/s ({100 * gbps * 1e9 / HBM_PEAK:.1f}% of peak) "
              f"spread={s['spread']:.3f}", flush=True)
    for shape, new, base in (("whole", "new_whole", "base_whole"),
                             ("whole_parity_only", "new_whole_parity",
                              "base_whole_parity")):
        n, b = st_[new], st_[base]
        spread_ms = max(n["max_ms"] - n["min_ms"], b["max_ms"] - b["min_ms"])
        doc["verdict"][shape] = dict(
            new_ms=n["median_ms"], baseline=base, baseline_ms=b["median_ms"],
            ratio=n["median_ms"] / b["median_ms"], sample_spread_ms=spread_ms,
            not_above_baseline_by_more_than_spread=n["median_ms"] -
            b["median_ms"] <= spread_ms)
        print(f"chunk_write_ab {shape}: new {n['median_ms']:.4f} ms, {base} "
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
