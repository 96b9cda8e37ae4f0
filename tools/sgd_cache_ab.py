#!/usr/bin/env python
"""data_cache = hbm against re-reading the file every epoch, on one box.

Writes a criteo-text file of Criteo-shaped synthetic rows (`base` distinct rows repeated up to `rows`) and trains it with
learner=sgd, V_dim=64, batch_size=10000, shuffle=10, one job per epoch, DIFACTO_PROFILE=1:

  A  the binary given as --parent (a build of the parent commit), no cache
  B  build/difacto with data_cache=hbm
  C  build/difacto without the key

alternated A B C A B C ..., `rounds` times with 4 epochs and as often with 1 epoch.  Per run: the rows/s of every epoch by the
worker loop's own clock (reader + preparation + step queueing seconds of the job's "host loop over" line), the process's wall
and CPU seconds (user + system of the child).  Per variant: CPU and wall seconds of a LATER epoch = (4-epoch run - 1-epoch
run) / 3, medians over the rounds.  One JSON object per run and one summary object on stdout.

usage: sgd_cache_ab.py --parent PATH [--rows 2000000] [--base 200000] [--rounds 3]"""
import argparse
import json
import os
import re
import resource
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_criteo(path, rows, base, seed=1):
    rng = np.random.default_rng(seed)
    ints = rng.zipf(1.3, size=(base, 13)) % 10000
    cats = (rng.zipf(1.1, size=(base, 26)) % 1000000).astype(np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)
    lab = (rng.random(base) < 0.25).astype(np.int32)
    lines = ["%d\t%s\t%s" % (lab[i], "\t".join(map(str, ints[i])), "\t".join("%08x" % c for c in cats[i])) for i in range(base)]
    blob = ("\n".join(lines) + "\n").encode()
    with open(path, "wb") as f:
        done = 0
        while done + base <= rows:
            f.write(blob)
            done += base
    return done


def run(exe, data, epochs, extra, timeout):
    args = [exe, "task=train", "learner=sgd", "data_in=" + data, "data_format=criteo", "batch_size=10000", "shuffle=10",
            "max_num_epochs=%d" % epochs, "num_jobs_per_epoch=1", "V_dim=64", "V_threshold=0", "l1=0", "lr=.01", "V_lr=.01",
            "V_init=hash", "table_capacity=8388608", "stop_rel_objv=0"] + extra
    before = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.time()
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, DIFACTO_PROFILE="1"))
    wall = time.time() - t0
    after = resource.getrusage(resource.RUSAGE_CHILDREN)
    cpu = (after.ru_utime - before.ru_utime) + (after.ru_stime - before.ru_stime)
    loops = [(int(m.group(1)), float(m.group(2)) + float(m.group(3)) + float(m.group(4))) for m in re.finditer(
        r"host loop over (\d+) minibatches: reader ([0-9.e+-]+) s, stage \+ localize \+ lookup ([0-9.e+-]+) s.*step ([0-9.e+-]+) s",
        r.stderr)]
    train = [l.split("Training: ")[-1] for l in r.stderr.splitlines() if "Training: " in l]
    cache = [l.split("] ")[-1] for l in r.stderr.splitlines() if "HBM cache" in l or ", cached " in l]
    return dict(rc=r.returncode, wall_s=wall, cpu_s=cpu, loop_s=[s for _, s in loops], minibatches=[n for n, _ in loops],
                training=train, cache=cache, tail=r.stderr[-400:] if r.returncode else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="build/difacto of the parent commit")
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--base", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="sgd_cache_ab_")
    data = os.path.join(d, "train.criteo")
    t0 = time.time()
    rows = write_criteo(data, a.rows, a.base)
    sys.stderr.write("%d rows, %.0f MB written in %.1f s\n" % (rows, os.path.getsize(data) / 1e6, time.time() - t0))
    mine = os.path.join(R, "build", "difacto")
    variants = [("A", a.parent, []), ("B", mine, ["data_cache=hbm"]), ("C", mine, [])]
    runs = {}
    for epochs in (4, 1):
        for rnd in range(a.rounds):
            for name, exe, extra in variants:
                o = run(exe, data, epochs, extra, a.timeout)
                o.update(variant=name, epochs=epochs, round=rnd, rows=rows,
                         rows_per_s_by_loop_clock=[rows / s for s in o["loop_s"]])
                print(json.dumps(o), flush=True)
                if o["rc"] != 0:
                    sys.exit("variant %s failed (exit %d)" % (name, o["rc"]))   # nothing more is started after a failed run
                runs.setdefault((name, epochs), []).append(o)
    summary = dict(summary=True, rows=rows)
    for name, _, _ in variants:
        four, one = runs[(name, 4)], runs[(name, 1)]
        later = [r_ for o in four for r_ in o["rows_per_s_by_loop_clock"][1:]]
        first = [o["rows_per_s_by_loop_clock"][0] for o in four]
        med = statistics.median
        summary[name] = dict(
            later_epochs_rows_per_s_by_loop_clock=dict(min=min(later), median=med(later), max=max(later)),
            first_epoch_rows_per_s_by_loop_clock=dict(min=min(first), median=med(first), max=max(first)),
            cpu_s_per_later_epoch=(med([o["cpu_s"] for o in four]) - med([o["cpu_s"] for o in one])) / 3,
            wall_s_per_later_epoch=(med([o["wall_s"] for o in four]) - med([o["wall_s"] for o in one])) / 3,
            cpu_s_4_epochs=[o["cpu_s"] for o in four], wall_s_4_epochs=[o["wall_s"] for o in four],
            same_training_lines_as_A=[o["training"] for o in four] == [o["training"] for o in runs[("A", 4)]])
    print(json.dumps(summary), flush=True)
    os.remove(data)
    os.rmdir(d)


if __name__ == "__main__":
    main()
