#!/usr/bin/env python
"""What exact_metrics = 1 costs, on one box (profiles/eval_metrics.txt).

1. dfh_eval_finish through capi: `--rows` (label, prediction) rows appended from the host, then finish timed `reps` times by
   the host clock (finish ends in a device synchronise; the first call, which allocates the workspace, is reported apart).
2. The command line: a criteo-text file of Criteo-shaped synthetic rows is trained for `epochs` epochs with itself as
   data_val, learner=sgd, V_dim=64, batch_size=10000, one job per epoch, DIFACTO_PROFILE=1:

     A  the binary given as --parent (a build of the parent commit), key absent
     B  build/difacto with exact_metrics=1
     C  build/difacto with the key absent

   alternated A B C A B C ..., `rounds` times.  Per run: rows/s of every validation pass by the worker loop's own clock (the
   reader + preparation + step queueing seconds of the job's "host loop over" line; the evaluator's appends are queued inside
   it, its finish comes after it), the same for the training passes, and the process's wall seconds.  One JSON object per run
   and a summary on stdout.

usage: eval_metrics_ab.py [--parent PATH] [--rows 6400000] [--cli-rows 2000000] [--rounds 3]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))


def finish_times(rows, reps):
    from difacto_amd import capi
    rng = np.random.default_rng(1)
    pred = rng.normal(size=rows).astype(np.float32)
    label = (rng.random(rows) < 1 / (1 + np.exp(-pred))).astype(np.float32)
    ctx = capi.Context(0)
    e = capi.Eval(ctx)
    e.append_host(label, pred)
    ctx.sync()
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        r = e.finish()
        ms.append((time.perf_counter() - t0) * 1e3)
    out = dict(finish=True, rows=rows, first_call_ms=ms[0], later_calls_ms=ms[1:], median_ms=statistics.median(ms[1:]),
               auc=r.auc2 / (2.0 * r.n_pos * r.n_neg), logloss=r.objv / r.n)
    e.close()
    ctx.close()
    return out


def run(exe, data, epochs, extra, timeout):
    args = [exe, "task=train", "learner=sgd", "data_in=" + data, "data_val=" + data, "data_format=criteo", "batch_size=10000",
            "shuffle=10", "max_num_epochs=%d" % epochs, "num_jobs_per_epoch=1", "V_dim=64", "V_threshold=0", "l1=0", "lr=.01",
            "V_lr=.01", "V_init=hash", "table_capacity=8388608", "stop_rel_objv=0", "stop_val_auc=-1e30"] + extra
    t0 = time.time()
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, DIFACTO_PROFILE="1"))
    wall = time.time() - t0
    loops = [float(m.group(2)) + float(m.group(3)) + float(m.group(4)) for m in re.finditer(
        r"host loop over (\d+) minibatches: reader ([0-9.e+-]+) s, stage \+ localize \+ lookup ([0-9.e+-]+) s.*step ([0-9.e+-]+) s",
        r.stderr)]
    lines = [l.split(" - ")[-1] for l in r.stderr.splitlines() if " - Validation" in l]
    return dict(rc=r.returncode, wall_s=wall, train_loop_s=loops[0::2], val_loop_s=loops[1::2], validation=lines,
                tail=r.stderr[-400:] if r.returncode else "")


def main():
    from sgd_cache_ab import write_criteo
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="build/difacto of the parent commit (absent: variants B and C only)")
    ap.add_argument("--rows", type=int, default=6400000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-rows", type=int, default=2000000)
    ap.add_argument("--base", type=int, default=200000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.rows:
        print(json.dumps(finish_times(a.rows, a.reps)), flush=True)
    if not a.cli_rows:
        return
    d = tempfile.mkdtemp(prefix="eval_metrics_ab_")
    data = os.path.join(d, "rows.criteo")
    rows = write_criteo(data, a.cli_rows, a.base)
    mine = os.path.join(R, "build", "difacto")
    variants = ([("A", a.parent, [])] if a.parent else []) + [("B", mine, ["exact_metrics=1"]), ("C", mine, [])]
    runs = {}
    for rnd in range(a.rounds):
        for name, exe, extra in variants:
            o = run(exe, data, a.epochs, extra, a.timeout)
            o.update(variant=name, round=rnd, rows=rows, val_rows_per_s=[rows / s for s in o["val_loop_s"]],
                     train_rows_per_s=[rows / s for s in o["train_loop_s"]])
            print(json.dumps(o), flush=True)
            if o["rc"] != 0:
                sys.exit("variant %s failed (exit %d)" % (name, o["rc"]))   # nothing more is started after a failed run
            runs.setdefault(name, []).append(o)
    summary = dict(summary=True, rows=rows, epochs=a.epochs)
    for name, _, _ in variants:
        val = [v for o in runs[name] for v in o["val_rows_per_s"]]
        later = [v for o in runs[name] for v in o["train_rows_per_s"][1:]]
        summary[name] = dict(val_rows_per_s=dict(min=min(val), median=statistics.median(val), max=max(val)),
                             later_train_rows_per_s=dict(min=min(later), median=statistics.median(later), max=max(later)),
                             wall_s=[o["wall_s"] for o in runs[name]],
                             same_validation_lines_as_C=[[l for l in o["validation"] if "whole set" not in l] for o in runs[name]] ==
                             [o["validation"] for o in runs["C"]])
    print(json.dumps(summary), flush=True)
    os.remove(data)
    os.rmdir(d)


if __name__ == "__main__":
    main()
