#!/usr/bin/env python
"""What task = predict costs by where its text is written, on one box (profiles/pred_write_ab.txt).

A criteo-text file of Criteo-shaped synthetic rows (`--base` rows repeated up to `--rows`) and the same rows as .rec; one
training epoch on the base rows gives the model.  Then task = predict, learner=sgd, V_dim=64, batch_size=10000, one job,
DIFACTO_PROFILE=1, alternated P H D R T, H D R T P, ... (a round starts one variant later than the round before), `--rounds` times:

  P  the binary given as --parent (a build of the parent commit) on the .rec file, key absent
  H  build/difacto pred_write=host on the .rec file
  D  build/difacto pred_write=device on the .rec file
  R  D with rec_decode=device
  T  build/difacto pred_write=device text_parse=device on the criteo text

Per run: rows/s by the worker loop's own clock (the reader + preparation + step seconds of the job's "host loop over" line;
the prediction writer works inside the step seconds under both values of the key), rows/s by the process clock, the host CPU
seconds of the process (user + sys), and whether pred_out has the bytes of the parent's (of H's without --parent).  Every run
has a time limit of its own and nothing more is started after a run that fails.  One JSON object per run and a summary on
stdout.  --trace: one more run of D under rocprofv3 --kernel-trace --stats, the formatter's kernels and k_forward out of its
kernel statistics.

usage: predict_ab.py [--parent PATH] [--rows 6400000] [--base 200000] [--rounds 3] [--trace DIR]"""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import resource
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

MODEL = ["V_dim=64", "V_threshold=0", "l1=0", "lr=.01", "V_lr=.01", "V_init=hash", "table_capacity=8388608"]
LOOP = r"host loop over (\d+) minibatches: reader ([0-9.e+-]+) s, stage \+ localize \+ lookup ([0-9.e+-]+) s.*step ([0-9.e+-]+) s"


def write_rec(path, text, reps):
    """the rows of the criteo text as RecordIO records of 10 000 rows (LZ4 row blocks), repeated"""
    from oracle import ingest as oi
    off, lab, idx = oi.parse_criteo(text)
    rows = len(lab)
    recs = []
    for a in range(0, rows, 10000):
        b = min(rows, a + 10000)
        recs.append(oi.write_crb_record(off[a:b + 1] - off[a], lab[a:b], idx[int(off[a]):int(off[b])]))
    blob = oi.write_recordio(recs)
    with open(path, "wb") as f:
        for _ in range(reps):
            f.write(blob)


def run(cmd, timeout, prefix=()):
    before = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.time()
    r = subprocess.run(list(prefix) + cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, DIFACTO_PROFILE="1"))
    wall = time.time() - t0
    after = resource.getrusage(resource.RUSAGE_CHILDREN)
    loops = [float(m.group(2)) + float(m.group(3)) + float(m.group(4)) for m in re.finditer(LOOP, r.stderr)]
    lines = [l.split("] ")[-1] for l in r.stderr.splitlines() if "pred_write=device:" in l or "on the device," in l or "fell back" in l]
    return dict(rc=r.returncode, wall_s=wall, loop_s=sum(loops), cpu_s=(after.ru_utime - before.ru_utime) + (after.ru_stime - before.ru_stime),
                lines=lines, tail=r.stderr[-600:] if r.returncode else "")


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest(), os.path.getsize(path)


def kernel_stats(d):
    """the rows of rocprofv3's kernel statistics for the formatter's kernels and k_forward"""
    out = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if re.search(r"k_predtext|k_forward", row.get("Name", "")):
                out.append({k: row[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in row})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="build/difacto of the parent commit (absent: no variant P)")
    ap.add_argument("--rows", type=int, default=6400000)
    ap.add_argument("--base", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--unit-rows", type=int, default=0, help="pred_unit_rows of the device variants (0: the default)")
    ap.add_argument("--trace", default="", help="directory for one rocprofv3 --kernel-trace --stats run of variant D")
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="predict_ab_")
    try:
        measure(a, d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def measure(a, d):
    from sgd_cache_ab import write_criteo
    reps = a.rows // a.base
    text, rec, base = os.path.join(d, "rows.criteo"), os.path.join(d, "rows.rec"), os.path.join(d, "base.criteo")
    t0 = time.time()
    rows = write_criteo(text, a.rows, a.base)
    write_criteo(base, a.base, a.base)
    write_rec(rec, open(base, "rb").read(), reps)
    print(json.dumps(dict(files=True, rows=rows, criteo_mb=os.path.getsize(text) / 1e6, rec_mb=os.path.getsize(rec) / 1e6,
                          seconds=time.time() - t0)), flush=True)
    mine, model = os.path.join(R, "build", "difacto"), os.path.join(d, "model")
    o = run([mine, "task=train", "learner=sgd", "data_in=" + base, "data_format=criteo", "batch_size=10000", "shuffle=10",
             "max_num_epochs=1", "num_jobs_per_epoch=1", "stop_rel_objv=0", "model_out=" + model] + MODEL, a.timeout)
    print(json.dumps(dict(o, variant="train")), flush=True)
    if o["rc"] != 0:
        sys.exit("training failed (exit %d)" % o["rc"])
    predict = ["task=predict", "learner=sgd", "batch_size=10000", "num_jobs_per_epoch=1", "model_in=" + model] + MODEL
    on_rec, on_text = ["data_in=" + rec, "data_format=rec"], ["data_in=" + text, "data_format=criteo"]
    unit = ["pred_unit_rows=%d" % a.unit_rows] if a.unit_rows else []
    variants = ([("P", a.parent, on_rec)] if a.parent else []) + [
        ("H", mine, on_rec + ["pred_write=host"]),
        ("D", mine, on_rec + ["pred_write=device"] + unit),
        ("R", mine, on_rec + ["pred_write=device", "rec_decode=device"] + unit),
        ("T", mine, on_text + ["pred_write=device", "text_parse=device"] + unit)]
    runs, want = {}, None
    for rnd in range(a.rounds):
        k = rnd % len(variants)   # every round starts one variant later: no variant always runs behind the same one
        for name, exe, extra in variants[k:] + variants[:k]:
            out = os.path.join(d, "pred_" + name)
            o = run([exe] + predict + extra + ["pred_out=" + out], a.timeout)
            o.update(variant=name, round=rnd, rows=rows)
            if o["rc"] == 0:
                o.update(loop_rows_per_s=rows / o["loop_s"] if o["loop_s"] else None, wall_rows_per_s=rows / o["wall_s"])
                got = digest(out)
                want = want or got   # the first variant's first file: the parent's when there is one
                o.update(pred_out_bytes=got[1], same_bytes_as_first=got == want)
                os.remove(out)
            print(json.dumps(o), flush=True)
            if o["rc"] != 0:
                sys.exit("variant %s failed (exit %d)" % (name, o["rc"]))   # nothing more is started after a failed run
            runs.setdefault(name, []).append(o)
    summary = dict(summary=True, rows=rows, first=variants[0][0])
    for name, _, _ in variants:
        rs = runs[name]
        summary[name] = dict(loop_rows_per_s=sorted(o["loop_rows_per_s"] for o in rs), wall_rows_per_s=sorted(o["wall_rows_per_s"] for o in rs),
                             cpu_s=sorted(o["cpu_s"] for o in rs), median_loop_rows_per_s=statistics.median(o["loop_rows_per_s"] for o in rs),
                             same_bytes_as_first=all(o["same_bytes_as_first"] for o in rs))
    print(json.dumps(summary), flush=True)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        out = os.path.join(d, "pred_trace")
        o = run([mine] + predict + variants[-3][2] + ["pred_out=" + out], a.timeout + 240,
                prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace, "-o", "predict_D", "--output-format", "csv", "--"])
        o.update(variant="D under rocprofv3", kernels=kernel_stats(a.trace))
        print(json.dumps(o), flush=True)


if __name__ == "__main__":
    main()
