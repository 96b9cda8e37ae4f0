#!/usr/bin/env python
"""What explain_out costs, on one box (profiles/explain_ab.txt).

(a) --kernels: the Criteo-shaped minibatch (10 000 rows x 39 ids, K = 10) at V_dim 64 and 128, every key with V.  Per V_dim, the
variants are alternated E F T, F T E, ... `--rounds` times, each a burst of `--reps` queued calls between two waits, after a
warm-up burst; per burst the wall-clock per call, per variant min / median / max over the bursts:
  E  dfh_explain_append_batch on the stepped minibatch (the object reset before every burst)
  F  dfh_sgd_step(is_train = 0): lookup + k_forward + penalty, the same gather — the floor of the memory side; and k_forward
     alone by the context's timing of a burst of its own
  T  torch on the same GPU: V[index] -> [B, 39, k], x scaled, bmm, upper-triangle mask, topk of |c|, the masked sum
(b) --e2e: task = predict pred_write = device over a generated criteo .rec file (tools/predict_ab.py's), alternated
P N X, N X P, ...: P the binary given as --parent, key absent; N build/difacto, key absent; X build/difacto with
explain_out.  Rows/s by the worker loop's own clock and by the process clock; pred_out of every run has the first run's bytes.
One JSON object per measurement on stdout.  Every child run has a time limit and nothing is started after one that fails.

usage: explain_ab.py --kernels [--rounds 5] [--reps 20] | --e2e [--parent PATH] [--rows 3200000] [--base 200000] [--rounds 3]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
ROWS, IDS, K = 10000, 39, 10


def spread(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v), n=len(v))


def rev(x):
    """ReverseBytes (include/difacto/base.h): the nibbles of a 64-bit word in reverse order"""
    x = np.asarray(x, np.uint64).byteswap()
    return ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4)) | ((x & np.uint64(0xF0F0F0F0F0F0F0F0)) >> np.uint64(4))


def kernels(a):
    import torch
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    rng = np.random.default_rng(1)
    m = 1 << 18   # keys: 64 / 128 MB of V rows, beyond no cache level that a 10 000 x 39 gather would stay in
    for k in (64, 128):
        ids = np.arange(1, m + 1, dtype=np.uint64) * np.uint64(7919)
        V = rng.normal(size=(m, k)).astype(np.float32) * 0.1
        scal = np.zeros((m, 4), np.float32)
        tb = capi.Table(ctx, 2 * m, V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
        tb.import_(rev(ids), scal, np.ones(m, np.int32), np.concatenate([V, np.zeros_like(V)], 1))
        idx = rng.integers(0, m, ROWS * IDS)
        b, e = capi.Batch(ctx, ROWS, ROWS * IDS), capi.Explain(ctx, K, capi.PAIRS_ABS, capacity_hint=ROWS * a.reps)
        b.load_host(np.arange(ROWS + 1, dtype=np.uint64) * IDS, ids[idx], None, np.ones(ROWS, np.float32))
        b.localize()
        b.lookup(tb)
        b.sgd_step(tb, is_train=False)
        ctx.sync()
        tV, tI = torch.from_numpy(V).cuda(), torch.from_numpy(idx.reshape(ROWS, IDS)).cuda()
        tx = torch.ones(ROWS, IDS, device="cuda")
        iu = torch.triu(torch.ones(IDS, IDS, dtype=torch.bool, device="cuda"), 1)

        def E():
            e.reset()
            for _ in range(a.reps):
                e.append_batch(b, tb)
            ctx.sync()

        def F():
            for _ in range(a.reps):
                b.sgd_step(tb, is_train=False)
            ctx.sync()

        def T():
            for _ in range(a.reps):
                g = tV[tI] * tx[:, :, None]
                c = torch.bmm(g, g.transpose(1, 2)).masked_fill(~iu, 0.0)
                top = torch.topk(c.abs().reshape(ROWS, -1), K)
                inter = c.sum((1, 2))
            torch.cuda.synchronize()
            return top, inter

        variants = [("E", E), ("F", F), ("T", T)]
        us = {n: [] for n, _ in variants}
        for _, f in variants:
            f()   # warm-up
        for rnd in range(a.rounds):
            s = rnd % 3
            for n, f in variants[s:] + variants[:s]:
                t0 = time.perf_counter()
                f()
                us[n].append((time.perf_counter() - t0) / a.reps * 1e6)
        ctx.set_timing(True)
        F()
        E()
        timing = {n: (ms / calls * 1e3 if calls else None) for n, (ms, calls) in ctx.get_timing().items() if n in ("forward", "lookup", "explain")}
        ctx.set_timing(False)
        got = e.read()
        print(json.dumps(dict(kernels=True, V_dim=k, rows=ROWS, ids_per_row=IDS, topk=K, reps=a.reps, us_per_call={n: spread(v) for n, v in us.items()},
                              event_us_per_launch=timing, pairs_listed=int(got["n"].sum()), nonfinite=got["nonfinite"])), flush=True)
        e.close()
        b.close()
        tb.close()
        del tV, tI, tx
    ctx.close()


def e2e(a):
    import predict_ab as pa
    from sgd_cache_ab import write_criteo
    d = tempfile.mkdtemp(prefix="explain_ab_")
    try:
        rec, base = os.path.join(d, "rows.rec"), os.path.join(d, "base.criteo")
        write_criteo(base, a.base, a.base)
        pa.write_rec(rec, open(base, "rb").read(), a.rows // a.base)
        rows = a.rows // a.base * a.base
        mine, model = os.path.join(R, "build", "difacto"), os.path.join(d, "model")
        o = pa.run([mine, "task=train", "learner=sgd", "data_in=" + base, "data_format=criteo", "batch_size=10000", "shuffle=10",
                    "max_num_epochs=1", "num_jobs_per_epoch=1", "stop_rel_objv=0", "model_out=" + model] + pa.MODEL, a.timeout)
        if o["rc"] != 0:
            sys.exit("training failed (exit %d): %s" % (o["rc"], o["tail"]))
        predict = ["task=predict", "learner=sgd", "batch_size=10000", "num_jobs_per_epoch=1", "model_in=" + model, "data_in=" + rec,
                   "data_format=rec", "pred_write=device"] + pa.MODEL
        expl = os.path.join(d, "explain.txt")
        variants = ([("P", a.parent, [])] if a.parent else []) + [("N", mine, []), ("X", mine, ["explain_out=" + expl, "explain_topk=%d" % K])]
        runs, want = {}, None
        for rnd in range(a.rounds):
            s = rnd % len(variants)
            for name, exe, extra in variants[s:] + variants[:s]:
                out = os.path.join(d, "pred_" + name)
                o = pa.run([exe] + predict + extra + ["pred_out=" + out], a.timeout)
                o.update(variant=name, round=rnd, rows=rows)
                if o["rc"] != 0:
                    print(json.dumps(o), flush=True)
                    sys.exit("variant %s failed (exit %d)" % (name, o["rc"]))   # nothing more is started after a failed run
                got = pa.digest(out)
                want = want or got
                o.update(loop_rows_per_s=rows / o["loop_s"], wall_rows_per_s=rows / o["wall_s"], same_pred_bytes_as_first=got == want)
                if extra:
                    o.update(explain_mb=os.path.getsize(expl) / 1e6)
                    os.remove(expl)
                os.remove(out)
                print(json.dumps(o), flush=True)
                runs.setdefault(name, []).append(o)
        print(json.dumps(dict(summary=True, rows=rows, **{n: dict(loop_rows_per_s=spread([o["loop_rows_per_s"] for o in rs]),
                                                                  wall_rows_per_s=spread([o["wall_rows_per_s"] for o in rs]),
                                                                  cpu_s=spread([o["cpu_s"] for o in rs]),
                                                                  same_pred_bytes_as_first=all(o["same_pred_bytes_as_first"] for o in rs))
                                                          for n, rs in runs.items()})), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--parent", default="", help="build/difacto of the parent commit (absent: no variant P)")
    ap.add_argument("--rows", type=int, default=3200000)
    ap.add_argument("--base", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    a.rounds = a.rounds or (5 if a.kernels else 3)
    if a.kernels:
        kernels(a)
    if a.e2e:
        e2e(a)
