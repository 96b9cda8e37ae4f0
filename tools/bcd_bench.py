"""learner = bcd on a Criteo-shaped synthetic (difacto_amd/synth.py), data, predictions and model resident in HBM.

Prints one JSON line (and writes it to --out): ms per epoch (every block: gradient over the training chunks, update,
prediction update; the progress after the last), the layout sizes and the bytes an epoch moves under this byte model:
  column-major slices  s_gk + s_row (+ s_val) per training entry, plus the pred and label gathers (8 B per entry)
  row-major slices     r_key (+ r_val) per entry and the dw gather (4 B per entry), 8 B of record and a pred read and
                       write (8 B) per touched row
  block state          g and h (16 B) and w, delta, dw read and written (24 B) per key
With --stats FILE (rocprofv3 --kernel-trace --stats output of this tool's run): per-kernel times and the gradient pass's
achieved TB/s (its bytes over k_bcd_grad + k_bcd_fixup time) against 5 TB/s.

  python tools/bcd_bench.py [--rows 4000000] [--chunk-rows 1000000] [--block-ratio 1] [--epochs 3] [--out FILE]
  python tools/bcd_bench.py --set-model ...   also: ms of dfh_bcd_set_model (model_in's warm start) with a value for every
                                              key of the model, keys shuffled, next to the epoch; the epochs still start cold
  python tools/bcd_bench.py --ab N            the plain object against a one-rank dfh_bcd_create_sharded object over the RCCL
                                              transport on the same chunks: N rounds of one epoch each, alternated A B A B in
                                              this process; ms per epoch of both and whether progress, model and predictions
                                              agree bit for bit (default --out profiles/bcd_sharded_ab.json).  Per block with
                                              keys the sharded object adds two self-copies and k_bcd_reduce (k_bcd_apply has
                                              no key to apply with one rank and is not launched)
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bcd_bench.py ...
  python tools/bcd_bench.py --stats DIR/.../run_kernel_stats.csv --model FILE
"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernel_stats(path, model):
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0].split("<")[0].split("::")[-1]
            if name.startswith("k_bcd") or name.startswith("k_auc"):
                tot[name] = tot.get(name, 0.0) + float(row["TotalDurationNs"])
    out = dict(kernel_total_ms={k: round(v / 1e6, 3) for k, v in sorted(tot.items())})
    if model:
        m = json.load(open(model))
        ep = m["epochs_timed"] + 1   # the warm-up epoch runs under the tracer too
        g = (tot.get("k_bcd_grad", 0) + tot.get("k_bcd_fixup", 0)) / ep
        p = tot.get("k_bcd_pred", 0) / ep
        out.update(grad_ms_per_epoch=g / 1e6, pred_ms_per_epoch=p / 1e6,
                   grad_TBps=m["bytes_grad"] / g / 1e3 if g else None, pred_TBps=m["bytes_pred"] / p / 1e3 if p else None,
                   target_TBps=5.0)
    return out


def ab(args):
    """A = capi.Bcd(ctx), B = capi.Bcd(ctx, comm) with one rank over RCCL; the same chunks, the same block orders"""
    import bcd_ref as R
    from difacto_amd import capi
    from difacto_amd.synth import CriteoSynth
    ctx = capi.Context(0)
    comm = capi.Comm.rccl(ctx, 0, 1, capi.Comm.unique_id())
    objs = [capi.Bcd(ctx), capi.Bcd(ctx, comm=comm)]
    gen = CriteoSynth(total_ids=args.ids, seed=7)
    sampled, entries, nchunks = 0, 0, 0
    for r0 in range(0, args.rows, args.chunk_rows):
        b = gen.batch(min(args.chunk_rows, args.rows - r0))
        for o in objs:
            o.add_chunk(b["offset"], b["index"], None, b["label"])
        s = len(range(0, len(b["label"]), 10))
        sampled += s
        entries += 39 * s
        nchunks += 1
    st = np.array([entries, sampled, args.rows], np.float32)
    ranges = R.partition_feature(0, R.block_counts(st, args.block_ratio))
    nkeys = [o.build(ranges, tail_feature_filter=args.tail_feature_filter, l1=1.0, lr=0.9) for o in objs]
    stream = R.RefRand()
    order = list(range(len(ranges)))
    stream.shuffle(order)
    for o in objs:
        o.epoch(order)   # warm
    ms, same = [[], []], True
    for _ in range(args.ab):
        stream.shuffle(order)
        progs = []
        for i, o in enumerate(objs):
            t = time.perf_counter()
            progs.append(o.epoch(order))
            ms[i].append(1e3 * (time.perf_counter() - t))
        same = same and progs[0].tobytes() == progs[1].tobytes()
    ma, mb = (o.get_model() for o in objs)
    same = same and all(ma[k].tobytes() == mb[k].tobytes() for k in ma)
    same = same and all(objs[0].get_pred(i).tobytes() == objs[1].get_pred(i).tobytes() for i in range(nchunks))
    sent, recv, groups = comm.stats()
    res = dict(workload="Criteo-shaped synthetic: %d rows x 39 slots, %d ids, no values, chunks of %d rows, block_ratio %g, "
               "tail_feature_filter %d" % (args.rows, args.ids, args.chunk_rows, args.block_ratio, args.tail_feature_filter),
               transport=comm.info(), nkeys=nkeys[0], nblk=len(ranges), rounds=args.ab,
               plain_ms_per_epoch=ms[0], sharded_world1_ms_per_epoch=ms[1],
               plain_ms_median=float(np.median(ms[0])), sharded_world1_ms_median=float(np.median(ms[1])),
               bits_agree=bool(same and nkeys[0] == nkeys[1]), wire_bytes_sent=int(sent), exchanges=int(groups))
    for o in objs:
        o.close()
    comm.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--chunk-rows", type=int, default=1_000_000)
    ap.add_argument("--ids", type=int, default=33_000_000)
    ap.add_argument("--block-ratio", type=float, default=1.0)
    ap.add_argument("--tail-feature-filter", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--set-model", action="store_true")
    ap.add_argument("--ab", type=int, default=0)
    ap.add_argument("--out")
    ap.add_argument("--stats")
    ap.add_argument("--model")
    args = ap.parse_args()
    if args.stats:
        r = kernel_stats(args.stats, args.model)
        print(json.dumps(r))
        if args.out:
            open(args.out, "w").write(json.dumps(r) + "\n")
        return
    if args.ab:
        r = ab(args)
        print(json.dumps(r))
        out = args.out or os.path.join(ROOT, "profiles", "bcd_sharded_ab.json")
        open(out, "w").write(json.dumps(r) + "\n")
        return
    import bcd_ref as R
    from difacto_amd import capi
    from difacto_amd.synth import CriteoSynth
    ctx = capi.Context(0)
    res = dict(workload="Criteo-shaped synthetic: %d rows x 39 slots, %d ids, no values, chunks of %d rows, block_ratio %g, "
               "tail_feature_filter %d" % (args.rows, args.ids, args.chunk_rows, args.block_ratio, args.tail_feature_filter))
    obj = capi.Bcd(ctx)
    gen = CriteoSynth(total_ids=args.ids, seed=7)
    t0 = time.perf_counter()
    nnz, sampled, entries, add_s = 0, 0, 0, 0.0
    for r0 in range(0, args.rows, args.chunk_rows):
        b = gen.batch(min(args.chunk_rows, args.rows - r0))
        n = len(b["label"])
        t1 = time.perf_counter()
        obj.add_chunk(b["offset"], b["index"], None, b["label"])
        add_s += time.perf_counter() - t1
        nnz += len(b["index"])
        s = len(range(0, n, 10))   # FeaGroupStats: every 10th row of a chunk, 39 entries each
        sampled += s
        entries += 39 * s
    res["load_s"] = time.perf_counter() - t0
    res["add_chunks_s"] = add_s   # dfh_*_add_chunk alone; load_s also generates the rows
    st = np.array([entries, sampled, args.rows], np.float32)
    ranges = R.partition_feature(0, R.block_counts(st, args.block_ratio))
    t0 = time.perf_counter()
    nkeys = obj.build(ranges, tail_feature_filter=args.tail_feature_filter, l1=1.0, lr=0.9)
    res["build_s"] = time.perf_counter() - t0
    info = [obj.block_info(b) for b in range(len(ranges))]
    touched = sum(i[3] for i in info)
    tr_nnz = sum(i[2] for i in info)
    res.update(nkeys=nkeys, nnz=nnz, nblk=len(ranges), block_nnz_max=max(i[2] for i in info), touched_rows=touched)
    res["bytes_grad"] = tr_nnz * (4 + 4 + 8)
    res["bytes_pred"] = tr_nnz * (4 + 4) + touched * (8 + 8)
    res["bytes_state"] = nkeys * (16 + 24)
    res["bytes_per_epoch"] = res["bytes_grad"] + res["bytes_pred"] + res["bytes_state"]
    if args.set_model:   # before the first step: every key of the model, shuffled; then n = 0 puts the built state back
        rng = np.random.default_rng(11)
        keys = rng.permutation(obj.get_model()["keys"])
        w = (rng.normal(size=len(keys)) * .01).astype(np.float32)
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            matched = obj.set_model(keys, w)
            ts.append(1e3 * (time.perf_counter() - t))
        assert matched == nkeys
        obj.set_model(keys[:0], w[:0])
        res.update(set_model_keys=len(keys), set_model_ms=ts, set_model_ms_best=min(ts))
    stream = R.RefRand()
    order = list(range(len(ranges)))
    stream.shuffle(order)
    obj.epoch(order)   # warm
    times, progs = [], []
    for _ in range(args.epochs):
        stream.shuffle(order)
        t = time.perf_counter()
        p = obj.epoch(order)
        times.append(time.perf_counter() - t)
        progs.append([float(x) for x in p])
    res.update(epochs_timed=args.epochs, ms_per_epoch=[1e3 * t for t in times], ms_per_epoch_best=1e3 * min(times),
               TBps_epoch=res["bytes_per_epoch"] / min(times) / 1e12, objv_per_row=[p[1] / p[0] for p in progs])
    obj.close()
    ctx.close()
    print(json.dumps(res))
    if args.out:
        open(args.out, "w").write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
