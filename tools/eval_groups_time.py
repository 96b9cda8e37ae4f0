#!/usr/bin/env python
"""What dfh_eval_finish_groups costs beside dfh_eval_finish, on one box (profiles/eval_groups.txt).

`--rows` (label, prediction, group id) rows are appended from the host once per shape; then the two calls are timed by the host
clock (both end in a device synchronise), alternating, `--reps` times each after one warm-up of each.  Shapes: groups of about 10
rows, and 10 groups."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from difacto_amd import capi
    ctx = capi.Context(0)
    rng = np.random.default_rng(0)
    pred = rng.normal(size=a.rows).astype(np.float32)
    label = (rng.random(a.rows) < 1 / (1 + np.exp(-pred))).astype(np.float32)
    print("rows %d, normal scores, labels drawn from them; times in ms, host clock around a call that waits" % a.rows)
    for what, ngroups in (("groups of ~10 rows", a.rows // 10), ("10 groups", 10)):
        gid = rng.integers(0, ngroups, a.rows).astype(np.uint64) * np.uint64(4096) + np.uint64(7)
        e = capi.Eval(ctx, a.rows)
        e.group_by_slot(7)
        e.append_host_groups(label, pred, gid)
        times = {"finish_groups": [], "finish": []}
        for rep in range(a.reps + 1):
            for name, call in (("finish_groups", e.finish_groups), ("finish", e.finish)):
                t0 = time.perf_counter()
                r = call()
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    times[name].append(dt)
        g = e.finish_groups()
        print("%-20s n_groups %d mixed %d rows_mixed %d gauc %.6f | whole-set auc %.6f" % (
            what, g.n_groups, g.n_mixed, g.rows_mixed, g.gauc_num / max(g.rows_mixed, 1), r.auc2 / (2.0 * r.n_pos * r.n_neg)))
        for name in ("finish_groups", "finish"):
            print("  %-14s %s" % (name, "  ".join("%.2f" % t for t in times[name])))
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
