#!/usr/bin/env python3
"""A/B per-stripe erasure patterns on one MI355X.

For a batch whose stripes carry different erasure patterns, times — in one
process, after warm-up, in alternating repeats, with device events around
synchronised work —
  (a) one ReedSolomon.recover_batch_mixed call (one launch for the batch);
  (b) the same stripes grouped by pattern, one recover_batch call per group
      (what a caller had to do before the multi-table entry point);
  (c) a uniform-pattern recover_batch at the same S and L: it moves the
      same bytes with one table and is the ceiling.
Each is timed three ways: through the batch entry points (tables and
pointer arrays uploaded per call), through cached plans (caller-owned
outputs, no host->device traffic in steady state), and as bare
lizec_ec_plan_run calls on those same plans ("plan_run": launch + kernel
only, without the Python argument handling of the two modes above).

Shapes:
  rebuild   ec(8,2), 256 stripes of 8 MiB parts, the 10 single-loss
            patterns round-robin (erased = {lost, one parity as padding},
            want = {lost}, as ec_read_plan.h:126-133 pads);
  degraded  ec(8,2), 4096 stripes of 64 KiB parts, the 45 double-loss
            patterns in seeded random order, both parts wanted.

Outputs of (a) and (b) are checked byte-identical at the timed sizes, and
(a) is checked against the original data.  Prints one JSON document (and
writes it to --out).
"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lizardfs_amd.ec import ReedSolomon  # noqa: E402

K, M = 8, 2
WARMUP = 2


def shapes(scale):
    singles = []
    for lost in range(K + M):
        pad = K + M - 1 if lost != K + M - 1 else K + M - 2
        singles.append(((lost, pad), (lost,)))
    doubles = [(p, p) for p in itertools.combinations(range(K + M), 2)]
    rng = np.random.default_rng(20240)
    s_reb, s_deg = max(10, 256 // scale), max(45, 4096 // scale)
    return [
        dict(name="rebuild", S=s_reb, L=(8 << 20) // scale, patterns=singles,
             order=np.arange(s_reb) % len(singles), uniform=((0, 9), (0,))),
        dict(name="degraded_read", S=s_deg, L=65536, patterns=doubles,
             order=rng.integers(0, len(doubles), s_deg),
             uniform=((1, 5), (1, 5))),
    ]


def stats(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms),
                spread=(max(ms) - min(ms)) / med, samples_ms=ms)


def run_shape(rs, sh, reps):
    S, L, pats, order = sh["S"], sh["L"], sh["patterns"], sh["order"]
    g = torch.Generator(device="cuda").manual_seed(99)
    data = torch.randint(0, 256, (S, K, L), dtype=torch.uint8, device="cuda",
                         generator=g)
    parity = rs.encode_batch(data)
    frags = [data[:, i, :] for i in range(K)] + \
            [parity[:, j, :] for j in range(M)]
    erased = np.array([pats[p][0] for p in order])   # [S, m]
    want = np.array([pats[p][1] for p in order])     # [S, oc]
    oc = want.shape[1]

    # (b): per-pattern groups.  A group whose stripes are evenly spaced is a
    # strided view; otherwise its rows are gathered into a copy up front
    # (the sorting a caller had to do), outside the timed region.
    groups = []
    for p in sorted(set(order.tolist())):
        idx = np.flatnonzero(order == p)
        step = int(idx[1] - idx[0]) if idx.size > 1 else 1
        if idx.size > 1 and np.all(np.diff(idx) == step):
            gf = [t[int(idx[0])::step][:idx.size] for t in frags]
        else:
            sel = torch.from_numpy(idx).cuda()
            gf = [t.index_select(0, sel) for t in frags]
        e, w = pats[p]
        gf = [None if i in e else gf[i] for i in range(K + M)]
        outs = {i: torch.empty((idx.size, L), dtype=torch.uint8,
                               device="cuda") for i in w}
        groups.append((idx, e, w, gf, outs))

    ue, uw = sh["uniform"]
    ufrags = [None if i in ue else frags[i] for i in range(K + M)]
    uouts = {i: torch.empty((S, L), dtype=torch.uint8, device="cuda")
             for i in uw}
    out_a = torch.empty((S, oc, L), dtype=torch.uint8, device="cuda")

    res = {}

    def mixed(plan):
        o, slots = rs.recover_batch_mixed(frags, erased, want=want,
                                          out=out_a if plan else None)
        res["a"], res["slots"] = o, slots

    def grouped(plan):
        res["b"] = [rs.recover_batch(gf, erased=e, want=w,
                                     out=outs if plan else None)
                    for _, e, w, gf, outs in groups]

    def uniform(plan):
        res["c"] = rs.recover_batch(ufrags, erased=ue, want=uw,
                                    out=uouts if plan else None)

    legs = [("a_mixed", mixed), ("b_grouped", grouped), ("c_uniform", uniform)]
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    report = dict(name=sh["name"], k=K, m=M, stripes=S, part_len=L,
                  patterns=len(set(order.tolist())), groups=len(groups),
                  outputs_per_stripe=oc, reps=reps, warmup=WARMUP)
    for mode, plan in (("batch", False), ("plan", True)):
        times = {name: [] for name, _ in legs}
        for rep in range(WARMUP + reps):
            for name, fn in legs:
                torch.cuda.synchronize()
                e0.record()
                fn(plan)
                e1.record()
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    times[name].append(e0.elapsed_time(e1))
        # (a) == (b) byte for byte, and (a) == the original data
        a, slots = res["a"], res["slots"]
        same = True
        for (idx, e, w, _, _), outs in zip(groups, res["b"]):
            sel = torch.from_numpy(idx).cuda()
            for j, part in enumerate(sorted(w)):
                assert (slots[idx, j] == part).all()
                same &= torch.equal(a[:, j, :].index_select(0, sel),
                                    outs[part])
        truth = True
        for part in range(K + M):
            src = frags[part]
            for j in range(oc):
                sel = torch.from_numpy(np.flatnonzero(slots[:, j] == part))
                if sel.numel():
                    sel = sel.cuda()
                    truth &= torch.equal(a[:, j, :].index_select(0, sel),
                                         src.index_select(0, sel))
        st = {name: stats(ms) for name, ms in times.items()}
        moved = S * L * (K + oc)   # bytes read + written by (a)
        report[mode] = dict(
            legs=st,
            a_equals_b=bool(same), a_equals_original=bool(truth),
            a_over_c=st["a_mixed"]["median_ms"] / st["c_uniform"]["median_ms"],
            a_over_b=st["a_mixed"]["median_ms"] / st["b_grouped"]["median_ms"],
            c_spread=st["c_uniform"]["spread"],
            a_gbps=moved / (st["a_mixed"]["median_ms"] / 1e3) / 1e9)
        if not plan:
            res.clear()

    # plan_run: the plans the "plan" mode cached, run bare.  (c) is the one
    # single-table plan over all S stripes, (b) the other single-table ones.
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa = [v for key, v in rs._plans.items() if key[0] == "mix"]
    pc = [v for key, v in rs._plans.items()
          if key[0] == "rec" and key[-2] == S]
    pb = [v for key, v in rs._plans.items()
          if key[0] == "rec" and key[-2] != S]
    assert (len(pa), len(pb), len(pc)) == (1, len(groups), 1)
    run = rs._lib.lizec_ec_plan_run
    times = {name: [] for name, _ in legs}
    for rep in range(WARMUP + reps):
        for (name, _), plans in zip(legs, (pa, pb, pc)):
            torch.cuda.synchronize()
            e0.record()
            for p in plans:
                assert run(p, stream) == 0
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append(e0.elapsed_time(e1))
    st = {name: stats(ms) for name, ms in times.items()}
    report["plan_run"] = dict(
        legs=st,
        a_over_c=st["a_mixed"]["median_ms"] / st["c_uniform"]["median_ms"],
        a_over_b=st["a_mixed"]["median_ms"] / st["b_grouped"]["median_ms"],
        c_spread=st["c_uniform"]["spread"],
        a_gbps=moved / (st["a_mixed"]["median_ms"] / 1e3) / 1e9)
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1,
                    help="divide the batch sizes (quick dry runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    doc = dict(device=torch.cuda.get_device_name(0), shapes=[])
    for sh in shapes(args.scale):
        r = run_shape(ReedSolomon(K, M), sh, args.reps)
        doc["shapes"].append(r)
        for mode in ("batch", "plan", "plan_run"):
            x = r[mode]
            print(f"mixed_ab {r['name']:14s} {mode:5s} "
                  f"a={x['legs']['a_mixed']['median_ms']:.3f} ms "
                  f"b={x['legs']['b_grouped']['median_ms']:.3f} ms "
                  f"c={x['legs']['c_uniform']['median_ms']:.3f} ms "
                  f"a/c={x['a_over_c']:.3f} a/b={x['a_over_b']:.3f} "
                  f"c_spread={x['c_spread']:.3f} "
                  f"same={x.get('a_equals_b', '-')} "
                  f"truth={x.get('a_equals_original', '-')}",
                  flush=True)
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    ok = all(r[m]["a_equals_b"] and r[m]["a_equals_original"]
             for r in doc["shapes"] for m in ("batch", "plan"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
