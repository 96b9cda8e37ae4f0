"""The vector passes of learner = lbfgs with and without l1 ("l1 on w"): device time per epoch of the
Prep / inner pass, the combine pass and the step pass on the shape of tests/test_lbfgs_l1_kernels.py's big case
(V_dim = 0, n = 2048 * 256 * 4 + 3 parameters, one chunk), from a rocprofv3 kernel trace.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/lbfgs_l1_bench.py --epochs 40 [--l1 0.2] [--tree PATH]
  python tools/lbfgs_l1_bench.py --stats DIR/.../run_kernel_stats.csv --epochs 40

The drive: m = 4 (the <= 11 right-hand vectors form once the ring is full), one line-search trial per epoch, fixed
coefficients; --l1 0 never calls dfh_lbfgs_set_l1.  --tree PATH imports difacto_amd from another checkout (the parent
commit's build) so that both run the same drive.  --stats prints, per pass, microseconds per epoch (total device time of
the pass's kernels, k_lb_finish left out, over the epochs that ran it) and the bytes per element the pass moves."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048 * 256 * 4 + 3
M = 4
# floats read + written per element once the ring is full (k = 4 pairs: 2k + 1 = 9 right-hand vectors)
#   inner    l1 = 0: 9 vectors read (y_last is not: 8) + gnew, w = 10 reads, g, y, s written = 3            -> 13 (alpha != 1)
#            l1 > 0: s_last and y_last not read: 7 + gnew, w, w0 = 10 reads, g, y, s, pg written = 4        -> 14
#   combine  l1 = 0: 9 in the chain + g again for the dot = 10 reads, p written                            -> 11
#            l1 > 0: the same with pg in g's place (the mask words only when V_dim > 0)                     -> 11
#   step     l1 = 0: w, p read, w written                                                                   -> 3
#            l1 > 0: w0, p, pg read, w written                                                              -> 4
FLOATS = {"inner": (13, 14), "combine": (11, 11), "wstep": (3, 4)}


def stats(path, epochs):
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0]
            if "_inner<" in name and "_inner<11" not in name:
                continue                                 # the first epoch's three-vector form: the ring is not full yet
            for key in ("inner", "combine", "wstep"):
                if "k_lb_" + key in name or "k_ow_" + key in name:
                    t = tot.setdefault(key, [0.0, 0, "ow" if "k_ow_" in name else "lb"])
                    t[0] += float(row["TotalDurationNs"])
                    t[1] += int(row["Calls"])
    out = {}
    for key, (ns, calls, kind) in sorted(tot.items()):
        fl = FLOATS[key][kind == "ow"]
        us = ns / calls / 1e3
        out[key] = dict(kernels=kind, calls=calls, us_per_call=round(us, 2), floats_per_element=fl,
                        TBps=round(fl * 4 * N / (us * 1e-6) / 1e12, 3))
    out["us_per_epoch"] = round(sum(v["us_per_call"] for k, v in out.items()), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--l1", type=float, default=0.0)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats, a.epochs)))
        return
    sys.path.insert(0, a.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from difacto_amd import capi
    from bcd_ref import reverse_bytes_np
    rng = np.random.default_rng(5)
    keys = rng.permutation(np.arange(1, N + 1)).astype(np.uint64)
    nrows = (N + 63) // 64
    off = np.minimum(np.arange(nrows + 1, dtype=np.uint64) * 64, N).astype(np.uint64)
    val = (rng.uniform(0.25, 1.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    lab = (rng.random(nrows) < 0.5).astype(np.float32)
    ctx = capi.Context(0)
    obj = capi.Lbfgs(ctx, 0, M)
    obj.add_chunk(off, reverse_bytes_np(keys), val, lab)
    obj.init_model(l2=0.1, V_l2=0.01)
    w = rng.uniform(-0.3, 0.3, N).astype(np.float32)
    w[::7] = 0
    obj.set_weights(w)
    if a.l1 > 0:
        obj.set_l1(a.l1)
    obj.calc_grad()
    pgs = []
    for e in range(a.epochs):
        incr = obj.prepare_direction()
        coef = None
        if incr is not None:
            k = (len(incr) - 1) // 6
            coef = np.linspace(0.002, 0.01, 2 * k + 1).astype(np.float32)     # none is 0: every vector is read
            coef[-1] = -0.05
        pgs.append(obj.calc_direction(coef))
        obj.line_search(0.5)
    print(json.dumps(dict(n=N, m=M, epochs=a.epochs, l1=a.l1, tree=a.tree, last_pg=pgs[-1], nnz=obj.evaluate()[1])))
    obj.close()
    ctx.close()


if __name__ == "__main__":
    main()
