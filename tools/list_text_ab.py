#!/usr/bin/env python
"""What explain_out and recommend_out cost end to end once their lines are formatted on the device (profiles/list_text_ab.txt).

task = predict pred_write = device, learner=sgd, V_dim 64, batch 10 000, K = 10, DIFACTO_PROFILE=1, on the files of
tools/explain_ab.py --e2e (a .rec of `--rows` criteo-shaped rows, the model of one epoch on the `--base` rows), alternated so
that every round starts one variant later, `--rounds` times:

  P   the binary given as --parent (a build of the parent commit), keys absent
  PX  the parent with explain_out                 N   build/difacto, keys absent
  X   build/difacto with explain_out              XU  X with pred_unit_rows=--unit-rows: several units, download over write
  PR  the parent with recommend_out: `--queries` query rows against a catalogue of `--items` rows (items_in, a .rec)
  R   build/difacto with recommend_out, the same

Per run: rows/s by the worker loop's own clock, by the process clock, the host CPU seconds, the file's size and whether the
file has the bytes of the first run that wrote one (pred_out, explain_out, recommend_out each).  Every run has a time limit of
its own and nothing more is started after a run that fails.

usage: list_text_ab.py [--parent PATH] [--rows 3200000] [--base 200000] [--queries 100000] [--items 1000000] [--rounds 3]
                       [--unit-rows 262144]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
K = 10


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1], n=len(v))


def main():
    import predict_ab as pa
    from sgd_cache_ab import write_criteo
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="build/difacto of the parent commit (absent: no variants P, PX, PR)")
    ap.add_argument("--rows", type=int, default=3200000)
    ap.add_argument("--base", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--items", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--unit-rows", type=int, default=262144)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="list_text_ab_")
    try:
        rec, qrec, irec, base = (os.path.join(d, n) for n in ("rows.rec", "queries.rec", "items.rec", "base.criteo"))
        write_criteo(base, a.base, a.base)
        text = open(base, "rb").read()
        pa.write_rec(rec, text, a.rows // a.base)
        pa.write_rec(irec, text, a.items // a.base)
        pa.write_rec(qrec, b"".join(text.splitlines(True)[:a.queries]), 1)
        mine, model = os.path.join(R, "build", "difacto"), os.path.join(d, "model")
        o = pa.run([mine, "task=train", "learner=sgd", "data_in=" + base, "data_format=criteo", "batch_size=10000", "shuffle=10",
                    "max_num_epochs=1", "num_jobs_per_epoch=1", "stop_rel_objv=0", "model_out=" + model] + pa.MODEL, a.timeout)
        if o["rc"] != 0:
            sys.exit("training failed (exit %d): %s" % (o["rc"], o["tail"]))
        predict = ["task=predict", "learner=sgd", "batch_size=10000", "num_jobs_per_epoch=1", "model_in=" + model, "data_format=rec",
                   "pred_write=device"] + pa.MODEL
        ex, rc = os.path.join(d, "explain.txt"), os.path.join(d, "recommend.txt")
        big, small = ["data_in=" + rec], ["data_in=" + qrec]
        expl = ["explain_out=" + ex, "explain_topk=%d" % K]
        reco = ["items_in=" + irec, "recommend_out=" + rc, "recommend_topk=%d" % K]
        rows_of = dict(P=a.rows // a.base * a.base, R=min(a.queries, a.base), PR=min(a.queries, a.base))
        variants = [("N", mine, big), ("X", mine, big + expl), ("XU", mine, big + expl + ["pred_unit_rows=%d" % a.unit_rows]), ("R", mine, small + reco)]
        if a.parent:
            variants = [("P", a.parent, big), ("PX", a.parent, big + expl), ("PR", a.parent, small + reco)] + variants
        runs, want = {}, {}
        for rnd in range(a.rounds):
            s = rnd % len(variants)
            for name, exe, extra in variants[s:] + variants[:s]:
                out = os.path.join(d, "pred_" + name)
                o = pa.run([exe] + predict + extra + ["pred_out=" + out], a.timeout)
                rows = rows_of.get(name, rows_of["P"])
                o.update(variant=name, round=rnd, rows=rows)
                if o["rc"] != 0:
                    print(json.dumps(o), flush=True)
                    sys.exit("variant %s failed (exit %d)" % (name, o["rc"]))   # nothing more is started after a failed run
                o.update(loop_rows_per_s=rows / o["loop_s"], wall_rows_per_s=rows / o["wall_s"])
                for key, path in (("pred", out), ("explain", ex), ("recommend", rc)):
                    if os.path.exists(path):
                        got = pa.digest(path)
                        first = want.setdefault((key, rows), got)
                        o.update({key + "_mb": got[1] / 1e6, "same_%s_bytes_as_first" % key: got == first})
                        os.remove(path)
                print(json.dumps(o), flush=True)
                runs.setdefault(name, []).append(o)
        print(json.dumps(dict(summary=True, **{n: dict(rows=rs[0]["rows"], loop_rows_per_s=spread([o["loop_rows_per_s"] for o in rs]),
                                                       wall_rows_per_s=spread([o["wall_rows_per_s"] for o in rs]),
                                                       cpu_s=spread([o["cpu_s"] for o in rs]),
                                                       same_bytes=all(v for o in rs for k, v in o.items() if k.startswith("same_")))
                                               for n, rs in runs.items()})), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
