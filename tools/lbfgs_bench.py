"""learner = lbfgs on a Criteo-shaped synthetic (difacto_amd/synth.py), data and optimiser state resident in HBM.

Prints one JSON line:
  - seconds per gradient evaluation (every chunk: gather, forward, backward, scatter) and per epoch
    (direction + one line-search step + evaluation, the two-loop algebra on the host)
  - effective TB/s of the vector kernels at n >= 32 M: the one-pass inner products of CalcIncreB
    (dfh_vec_inner_multi, 3 x (2m+1) products over 2m+2 distinct vectors) and the direction (dfh_vec_combine,
    2m+1 vectors in, one out, <g, p>), bytes = distinct vectors read + written, time = wall time of the synchronous call
  - with --stats FILE (rocprofv3 --kernel-trace --stats output of this tool's run): the gather + scatter time as a share
    of the forward + backward kernel time

  python tools/lbfgs_bench.py [--rows 4000000] [--chunk-rows 1000000] [--V-dim 10] [--m 10]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/lbfgs_bench.py ...
  python tools/lbfgs_bench.py --stats DIR/.../run_kernel_stats.csv [--nparams N]
  - with --ab K: the sharded object (dfh_lbfgs_create_sharded) at world 1 over RCCL against the plain one on the same
    chunks, alternated A B A B (K rounds of one gradient evaluation and one epoch each); both must print the same bits.
    Reports seconds per evaluation and per epoch of each, the slowdown, and the bytes the exchange moves per evaluation
    (dfh_comm_stats counts bytes to other ranks: none at world 1, where the pull and the push are self-copies)
  - --stats with --nparams N (the model's floats; world 1: every float is pulled and pushed once) adds the bandwidth of
    k_lb_pack (reads index + w, writes the send buffer: 12 B per float) and k_lb_reduce (reads both index lists and the
    received gradient, writes g_new: 16 B per float) as TB/s and as a fraction of 8 TB/s
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def share_from_stats(path, nparams=0):
    """gather + scatter over forward + backward, from a rocprofv3 kernel_stats.csv"""
    tot, calls = {}, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            for key in ("k_lb_gather", "k_lb_scatter", "k_forward", "k_backward_all", "k_lb_inner", "k_lb_combine",
                        "k_lb_wstep", "k_lb_finish", "k_lb_pack", "k_lb_reduce"):
                if key in name.split("(")[0]:
                    tot[key] = tot.get(key, 0.0) + ns
                    calls[key] = calls.get(key, 0) + int(row["Calls"])
    gs = tot.get("k_lb_gather", 0) + tot.get("k_lb_scatter", 0)
    fb = tot.get("k_forward", 0) + tot.get("k_backward_all", 0)
    out = dict(kernel_total_ms={k: round(v / 1e6, 3) for k, v in sorted(tot.items())},
               gather_scatter_share_of_fwd_bwd=round(gs / fb, 4) if fb else None, target_share=0.5)
    if nparams:
        for key, per in (("k_lb_pack", 12), ("k_lb_reduce", 16)):
            if calls.get(key):
                us = tot[key] / calls[key] / 1e3
                tbps = per * nparams / (us * 1e-6) / 1e12
                out[key] = dict(calls=calls[key], us_per_call=round(us, 2), bytes_per_call=per * nparams,
                                TBps=round(tbps, 3), of_8TBps=round(tbps / 8, 3))
    return out


def timed(fn, reps):
    fn()   # warm
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps


def vector_kernels(capi, ctx, n, m, reps):
    """TB/s of the inner-product and direction kernels on 2m+2 distinct device vectors of n floats"""
    rng = np.random.default_rng(0)
    base = rng.standard_normal(n).astype(np.float32)
    bufs = [capi.DeviceBuffer.from_numpy(ctx, base * (1 + 0.01 * i)) for i in range(2 * m + 2)]
    try:
        b = bufs[:2 * m + 1]                       # s_0..s_{m-1}, y_0..y_{m-1}, g
        a = [b[m - 1], b[2 * m - 1], b[2 * m]]     # s_last, y_last, g: read once with the right-hand vectors
        t_inner = timed(lambda: capi.vec_inner_multi(ctx, n, a, b), reps)
        coef = np.linspace(-0.5, 0.5, 2 * m + 1).astype(np.float32)
        out = bufs[2 * m + 1]
        t_comb = timed(lambda: capi.vec_combine(ctx, n, b, coef, out, dot=b[2 * m]), reps)
    finally:
        for x in bufs:
            x.close()
    inner_bytes = (2 * m + 1) * n * 4
    comb_bytes = (2 * m + 1 + 1) * n * 4           # 2m+1 read (g once, also for <g, p>), p written
    return dict(n=n, m=m, inner_products_s=t_inner, inner_products_TBps=inner_bytes / t_inner / 1e12,
                direction_s=t_comb, direction_TBps=comb_bytes / t_comb / 1e12, target_TBps=4.5)


def ab_main(args):
    """the sharded object at world 1 over RCCL against the plain object on the same chunks, alternated A B A B"""
    from difacto_amd import capi
    from difacto_amd.synth import CriteoSynth
    from oracle.lbfgs_driver import Twoloop
    ctx = capi.Context(0)
    comm = capi.Comm.rccl(ctx, 0, 1, capi.Comm.unique_id())
    res = dict(workload="Criteo-shaped synthetic: %d rows x 39 slots, %d ids, V_dim %d, V_threshold %d, m %d, chunks of %d rows"
               % (args.rows, args.ids, args.V_dim, args.V_threshold, args.m, args.chunk_rows), transport=comm.info())
    objs = dict(plain=capi.Lbfgs(ctx, args.V_dim, args.m), sharded=capi.Lbfgs(ctx, args.V_dim, args.m, comm=comm))
    gen = CriteoSynth(total_ids=args.ids, seed=7)
    nnz = 0
    for r0 in range(0, args.rows, args.chunk_rows):
        b = gen.batch(min(args.chunk_rows, args.rows - r0))
        for o in objs.values():
            o.add_chunk(b["offset"], b["index"], None, b["label"])
        nnz += len(b["index"])
    for name, o in objs.items():
        nkeys, n = o.init_model(tail_feature_filter=4, V_threshold=args.V_threshold, V_init_scale=0.01, l2=100, V_l2=10)
        res.update(nkeys=nkeys, nparams=n, nnz=nnz)
    loss = {name: o.calc_grad()[0] for name, o in objs.items()}   # warm
    tls = {name: Twoloop() for name in objs}
    grad = {name: [] for name in objs}
    epoch = {name: [] for name in objs}
    objv = {name: [] for name in objs}
    comm.stats(reset=True)
    for rnd in range(args.ab):
        for name in ("plain", "sharded") if rnd % 2 == 0 else ("sharded", "plain"):
            o = objs[name]
            grad[name].append(timed(lambda: o.calc_grad(), 1))
            t = time.perf_counter()
            incr = o.prepare_direction()
            if incr is None:
                o.calc_direction(None)
            else:
                tls[name].apply_incre_B([float(x) for x in incr])
                o.calc_direction(np.array(tls[name].calc_delta(), np.float32))
            f, _, _ = o.line_search(1.0 if rnd else args.rows / nnz)
            o.evaluate()
            epoch[name].append(time.perf_counter() - t)
            objv[name].append(f)
    sent, recv, groups = comm.stats()
    med = lambda v: float(np.median(v))
    res.update(grad_eval_s={k: med(v) for k, v in grad.items()}, epoch_s={k: med(v) for k, v in epoch.items()},
               grad_eval_all_s=grad, epoch_all_s=epoch,
               slowdown_grad_eval=med(grad["sharded"]) / med(grad["plain"]) - 1,
               slowdown_epoch=med(epoch["sharded"]) / med(epoch["plain"]) - 1,
               same_bits=loss["plain"] == loss["sharded"] and objv["plain"] == objv["sharded"], objv=objv["sharded"],
               bytes_to_other_ranks_per_eval=sent / (3 * args.ab), exchange_groups=groups,
               self_exchange_bytes_per_eval=2 * 4 * res["nparams"])
    for o in objs.values():
        o.close()
    comm.close()
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--chunk-rows", type=int, default=1_000_000)
    ap.add_argument("--ids", type=int, default=33_000_000)
    ap.add_argument("--V-dim", type=int, default=10)
    ap.add_argument("--V-threshold", type=int, default=10)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--vec-n", type=int, default=1 << 25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats", help="only summarise a rocprofv3 kernel_stats.csv")
    ap.add_argument("--nparams", type=int, default=0, help="with --stats: the model's floats, for k_lb_pack / k_lb_reduce")
    ap.add_argument("--ab", type=int, default=0, help="rounds of plain vs sharded (world 1, RCCL), alternated")
    args = ap.parse_args()
    if args.stats:
        print(json.dumps(share_from_stats(args.stats, args.nparams)))
        return
    if args.ab:
        ab_main(args)
        return
    from difacto_amd import capi
    from difacto_amd.synth import CriteoSynth
    from oracle.lbfgs_driver import Twoloop
    ctx = capi.Context(0)
    res = dict(workload="Criteo-shaped synthetic: %d rows x 39 slots, %d ids, V_dim %d, V_threshold %d, m %d, chunks of %d rows"
               % (args.rows, args.ids, args.V_dim, args.V_threshold, args.m, args.chunk_rows))
    obj = capi.Lbfgs(ctx, args.V_dim, args.m)
    gen = CriteoSynth(total_ids=args.ids, seed=7)
    t0 = time.perf_counter()
    nnz, add_s = 0, 0.0
    for r0 in range(0, args.rows, args.chunk_rows):
        b = gen.batch(min(args.chunk_rows, args.rows - r0))
        t1 = time.perf_counter()
        obj.add_chunk(b["offset"], b["index"], None, b["label"])
        add_s += time.perf_counter() - t1
        nnz += len(b["index"])
    res["load_s"] = time.perf_counter() - t0
    res["add_chunks_s"] = add_s   # dfh_*_add_chunk alone; load_s also generates the rows
    t0 = time.perf_counter()
    nkeys, n = obj.init_model(tail_feature_filter=4, V_threshold=args.V_threshold, V_init_scale=0.01, l2=100, V_l2=10)
    res["init_s"] = time.perf_counter() - t0
    res.update(nkeys=nkeys, nparams=n, nnz=nnz)
    res["grad_eval_s"] = timed(lambda: obj.calc_grad(), args.reps)
    loss, _ = obj.calc_grad()
    tl = Twoloop()
    epochs = []
    for ep in range(args.epochs):   # direction + one line-search step + evaluation (the step count of a typical epoch)
        t = time.perf_counter()
        incr = obj.prepare_direction()
        if incr is None:
            obj.calc_direction(None)
        else:
            tl.apply_incre_B([float(x) for x in incr])
            obj.calc_direction(np.array(tl.calc_delta(), np.float32))
        f, _, _ = obj.line_search(1.0 if ep else args.rows / nnz)
        obj.evaluate()
        epochs.append(time.perf_counter() - t)
    res.update(epoch_s=epochs, objv_first=loss, objv_last=f)
    obj.close()
    res["vector_kernels"] = vector_kernels(capi, ctx, args.vec_n, args.m, args.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
