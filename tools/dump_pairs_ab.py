#!/usr/bin/env python
"""What dfh_dump_pairs costs against the obvious other way, in one process on one box (profiles/dump_pairs_ab.txt).

A synthetic model built through capi: `--entries` keys, every one with V (so nV = entries), V normal floats.  Then, alternated
A B A B (`--rounds` pairs), the top `--topk` partners by |s| of ALL entries:

  A  capi.ModelDump.pairs: k_pairs_pack (first call only), k_pairs_topk, k_pairs_merge; the stages' kernel spans by the
     context's timing (HIP events around each launch), and the call's wall seconds with its downloads
  B  the yardstick, never the code under test: torch.matmul of the same fp32 rows (TF32 off) in blocks of `--q-chunk` queries
     by `--c-chunk` candidates that fit memory, the diagonal masked, torch.topk of each block and a running merge (topk of the
     kept and the new); wall seconds around a device synchronise

and how many of A's (entry, partner) pairs B also has (the two sum in different orders: near-ties may swap).  Per run one JSON
line; a summary with the sweep's share of the fp32 matrix peak (2 nV^2 kd flop over the sweep's span; the peak is `--peak-tflops`).
Nothing more is started after a run that fails.  `--only-a` leaves B out: the form for a counter run (rocprofv3 --pmc ... --
python tools/dump_pairs_ab.py --only-a), whose times are not to be used.

usage: dump_pairs_ab.py [--entries 100000] [--v-dim 64] [--topk 10] [--rounds 2] [--only-a]"""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)


def build_table(capi, ctx, n, k, seed=1):
    rng = np.random.default_rng(seed)
    tb = capi.Table(ctx, n + n // 2 + 1024, V_dim=k, init_mode=capi.INIT_HASH)
    ids = rng.permutation(np.arange(1, 4 * n + 1, dtype=np.uint64))[:n] * np.uint64(2654435761)   # distinct (an odd multiplier mod 2^64)
    for a in range(0, n, 100000):
        m = min(100000, n - a)
        scal = np.zeros((m, 4), np.float32)
        scal[:, 1] = rng.normal(size=m) * 0.1
        V = np.zeros((m, 2 * k), np.float32)
        V[:, :k] = rng.normal(size=(m, k)) * 0.05
        tb.import_(ids[a:a + m], scal, np.ones(m, np.int32), V)
    return tb


def torch_topk(torch, P, K, qc, cc):
    """-> (positions [n x K], seconds): blocked P P^T, |s|, the diagonal out, topk per block, running merge"""
    n = P.shape[0]
    out = torch.empty((n, K), dtype=torch.int64, device=P.device)
    torch.cuda.synchronize()
    t0 = time.time()
    for q0 in range(0, n, qc):
        Q = P[q0:q0 + qc]
        best_v = best_i = None
        for c0 in range(0, n, cc):
            S = torch.matmul(Q, P[c0:c0 + cc].T).abs_()
            lo, hi = max(q0, c0), min(q0 + Q.shape[0], c0 + cc)
            if lo < hi:   # the self pairs of this block
                d = torch.arange(lo, hi, device=P.device)
                S[d - q0, d - c0] = -1.0
            v, i = torch.topk(S, min(K, S.shape[1]), dim=1)
            i += c0
            if best_v is not None:
                v, i = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
                v, sel = torch.topk(v, K, dim=1)
                i = torch.gather(i, 1, sel)
            best_v, best_i = v, i
        out[q0:q0 + Q.shape[0]] = best_i
    torch.cuda.synchronize()
    return out, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=100000)
    ap.add_argument("--v-dim", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--q-chunk", type=int, default=8192)
    ap.add_argument("--c-chunk", type=int, default=65536)
    ap.add_argument("--only-a", action="store_true", help="no yardstick: dfh_dump_pairs alone, for a counter run")
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32 matrix peak of the box (MI355X: 157.3)")
    a = ap.parse_args()
    import torch
    from difacto_amd import capi
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    torch.backends.cuda.matmul.allow_tf32 = False
    n, k, K = a.entries, a.v_dim, a.topk
    ctx = capi.Context(0)
    tb = build_table(capi, ctx, n, k)
    d = capi.ModelDump(tb)
    ent = d.entries()
    assert d.shape() == (n, n, k)
    P = None if a.only_a else torch.from_numpy(ent["V"]).cuda()
    pos_of_id = ent["ids"]   # position -> id (every entry has V: positions are entries)
    names = ("pairs_pack", "pairs_sweep", "pairs_merge")
    ctx.set_timing(True)
    d.pairs(0, min(n, 256), K)   # warm-up: the first call packs; its span is reported on its own
    warm = ctx.get_timing(reset=True)
    if not a.only_a:
        torch_topk(torch, P[:min(n, 4096)], K, a.q_chunk, a.c_chunk)
    print(json.dumps(dict(setup=True, entries=n, V_dim=k, topk=K, pack_ms=warm["pairs_pack"][0])), flush=True)
    runs = {"A": [], "B": []}
    got = None
    for rnd in range(a.rounds):
        t0 = time.time()
        got = d.pairs(0, n, K)
        wall = time.time() - t0
        tm = ctx.get_timing(reset=True)
        o = dict(variant="A", round=rnd, wall_s=wall, nonfinite=got["nonfinite"], **{x + "_ms": tm[x][0] for x in names[1:]})
        o["kernels_s"] = (o["pairs_sweep_ms"] + o["pairs_merge_ms"]) / 1e3
        print(json.dumps(o), flush=True)
        runs["A"].append(o)
        if a.only_a:
            continue
        idx, sec = torch_topk(torch, P, K, a.q_chunk, a.c_chunk)
        theirs = pos_of_id[idx.cpu().numpy()]
        both = np.mean([(np.sort(got["ids"], 1) == np.sort(theirs, 1)).all(1).mean()])
        o = dict(variant="B", round=rnd, wall_s=sec, rows_with_the_same_partner_set=float(both))
        print(json.dumps(o), flush=True)
        runs["B"].append(o)
    kd = (k + 7) // 8 * 8
    sweep = sorted(o["pairs_sweep_ms"] / 1e3 for o in runs["A"])
    flop = 2.0 * n * n * kd
    print(json.dumps(dict(summary=True, entries=n, V_dim=k, topk=K, A_kernels_s=sorted(round(o["kernels_s"], 4) for o in runs["A"]),
                          A_wall_s=sorted(round(o["wall_s"], 4) for o in runs["A"]), B_wall_s=sorted(round(o["wall_s"], 4) for o in runs["B"]),
                          sweep_ms=[round(1e3 * x, 3) for x in sweep],
                          A_wall_over_B_wall=[round(x["wall_s"] / y["wall_s"], 4) for x, y in zip(runs["A"], runs["B"])],
                          sweep_tflops=[round(flop / s / 1e12, 2) for s in sweep],
                          sweep_share_of_fp32_matrix_peak=[round(flop / s / 1e12 / a.peak_tflops, 4) for s in sweep])), flush=True)
    d.close()
    tb.close()
    ctx.close()


if __name__ == "__main__":
    main()
