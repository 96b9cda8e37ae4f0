#!/usr/bin/env python
"""The device feed (csrc/dfh_feed.hip) against a build of the parent commit, on one box, every run a fresh process.

  bench   python bench.py --gpus 1 --steps K --warmup W in each tree: parent, this, parent, this, ... (--pairs of them), then
          the same with --min-time S (bench.py repeats the timed region and reports the median repetition and the spread)
  cli     build/difacto of each tree on a criteo-text file of Criteo-shaped synthetic rows (tools/sgd_cache_ab.py's),
          learner=sgd, V_dim=64, batch_size=10000, shuffle=10, two epochs, DFH_PROFILE_PREP=1 and DIFACTO_PROFILE=1,
          without and with data_cache=hbm, alternating the same way.  Per run the host seconds per call of
          dfh_batch_prepare_rows / _cached, summed over the job's batch objects and by section, and of the row buffer uploads.

One JSON object per run on stdout.  Nothing more is started after a run that fails.

usage: device_feed_ab.py --parent DIR [--pairs 2] [--steps 200] [--warmup 20] [--min-time 2] [--rows 1000000]
(DIR: a built checkout of the parent)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "tools"))
from sgd_cache_ab import write_criteo  # noqa: E402

SECTIONS = ("begin", "wait staged", "write description", "gather", "localize", "lookup + ready")


def bench(tree, steps, warmup, extra):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)] + extra, cwd=tree,
                       capture_output=True, text=True, timeout=600)
    if r.returncode:
        return dict(rc=r.returncode, tail=r.stderr[-400:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    return dict(rc=0, result=out)


def cli(tree, data, extra):
    args = [os.path.join(tree, "build", "difacto"), "task=train", "learner=sgd", "data_in=" + data, "data_format=criteo",
            "batch_size=10000", "shuffle=10", "max_num_epochs=2", "num_jobs_per_epoch=1", "V_dim=64", "V_threshold=0", "l1=0",
            "lr=.01", "V_lr=.01", "V_init=hash", "table_capacity=8388608", "stop_rel_objv=0"] + extra
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=dict(os.environ, DIFACTO_PROFILE="1", DFH_PROFILE_PREP="1"))
    if r.returncode:
        return dict(rc=r.returncode, tail=r.stderr[-400:])
    calls, secs = 0, [0.0] * len(SECTIONS)
    for m in re.finditer(r"dfh_batch_prepare_rows x (\d+): begin ([0-9.]+) s, wait staged ([0-9.]+), write description ([0-9.]+), "
                         r"gather ([0-9.]+), localize ([0-9.]+), lookup \+ ready ([0-9.]+)", r.stderr):
        calls += int(m.group(1))
        secs = [s + float(m.group(2 + i)) for i, s in enumerate(secs)]
    up_calls, up_secs = 0, 0.0
    for m in re.finditer(r"dfh_rowbuf_load_host x (\d+) \([0-9.]+ MB\): offsets ([0-9.]+) s, queue copies ([0-9.]+), wait ([0-9.]+)", r.stderr):
        up_calls += int(m.group(1))
        up_secs += float(m.group(2)) + float(m.group(3))   # (the wait is the copy itself)
    loops = [float(m.group(1)) for m in re.finditer(r"stage \+ localize \+ lookup ([0-9.e+-]+) s", r.stderr)]
    return dict(rc=0, prepare_calls=calls, prepare_host_us_per_call=sum(secs) / max(calls, 1) * 1e6,
                prepare_host_us_per_call_by_section={k: s / max(calls, 1) * 1e6 for k, s in zip(SECTIONS, secs)},
                upload_calls=up_calls, upload_host_us_per_call_offsets_and_queue=up_secs / max(up_calls, 1) * 1e6,
                worker_loop_prepare_s=loops, training=[l.split("Training: ")[-1] for l in r.stderr.splitlines() if "Training: " in l])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--min-time", type=float, default=2.0)
    a = ap.parse_args()
    trees = [("parent", os.path.abspath(a.parent)), ("this change", R)] * a.pairs

    def emit(o, **kw):
        o.update(kw)
        print(json.dumps(o), flush=True)
        if o["rc"] != 0:
            sys.exit("run %s failed (exit %d)" % (o["run"], o["rc"]))

    for extra in ([], ["--min-time", str(a.min_time)]):
        for i, (name, tree) in enumerate(trees):
            emit(bench(tree, a.steps, a.warmup, extra), tool="bench.py", run="AB"[i % 2] + str(i // 2 + 1), library=name,
                 workload=" ".join(["--gpus 1 --steps %d --warmup %d" % (a.steps, a.warmup)] + extra))
    d = tempfile.mkdtemp(prefix="device_feed_ab_")
    data = os.path.join(d, "train.criteo")
    rows = write_criteo(data, a.rows, min(200000, a.rows))
    try:
        for extra in ([], ["data_cache=hbm"]):
            for i, (name, tree) in enumerate(trees):
                emit(cli(tree, data, extra), tool="build/difacto", run="AB"[i % 2] + str(i // 2 + 1), library=name,
                     workload="Criteo-shaped synthetic criteo text, %d rows, learner=sgd V_dim=64 batch_size=10000 shuffle=10, "
                              "2 epochs, DFH_PROFILE_PREP=1 %s" % (rows, " ".join(extra) or "(no cache)"))
    finally:
        os.remove(data)
        os.rmdir(d)


if __name__ == "__main__":
    main()
