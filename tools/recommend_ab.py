#!/usr/bin/env python
"""What dfh_recommend costs against the obvious other way, in one process on one box (profiles/recommend_ab.txt).

A synthetic model built through capi: `--keys` keys, every one with V, normal floats.  `--items` catalogue rows of `--item-ids`
ids and `--rows` query rows of `--row-ids` ids (the criteo shape: 39), x = 1, appended in minibatches of `--batch` rows as the
prediction loop does.  Then, alternated A B A B (`--rounds` pairs), the top `--topk` items of ALL query rows:

  A  capi.Recommend over a catalogue built once (its k_rec_embed span is reported on its own): per round reset, append_batch
     per minibatch (lookup and prediction step outside the clock's kernels but inside its wall), read; the kernels' spans by the
     context's timing (the launches carry their events) and the wall seconds with the download
  B  the yardstick, never the code under test: the same operands, [S_q | 1] and [S_i | b_i] made with torch from the same V and
     w, through torch.matmul (fp32, TF32 off) in blocks of `--q-chunk` queries by `--c-chunk` items, torch.topk of each block
     and a running merge; wall seconds around a device synchronise

and how many query rows get the same item set from both (the two sum in different orders: near-ties may swap).  One JSON line
per run; a summary with the sweep's share of the fp32 matrix peak: 2 R M kd flop executed (kd = roundup(V_dim + 1, 8)) and
2 R M (V_dim + 1) useful, over the sweep's span; the peak is `--peak-tflops`.  Nothing more is started after a run that fails.

`--precision bf16` (with `--shortlist`) adds, in every round between A and B, variant A_bf16: a second capi.Recommend created
under rec_precision = 1 over the same catalogue, the same rows through it, its spans (rec_embed, rec_convert, rec_cand,
rec_rescore) and `recall`: the share of A's (row, item) pairs that A_bf16 returns.  `--no-torch` leaves B out.

usage: recommend_ab.py [--rows 100000] [--items 1000000] [--v-dim 64] [--topk 10] [--rounds 3] [--batch 10000] [--rec-split 0]
                       [--precision fp32|bf16] [--shortlist 0] [--no-torch]"""
import argparse
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
U64 = np.uint64


def rev(x):   # ReverseBytes: a batch's feature id -> the table's key
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


def torch_topk(torch, Q, I, K, qc, cc):
    """-> (items [R x K], seconds): blocked Q I^T, topk per block, running merge"""
    out = torch.empty((Q.shape[0], K), dtype=torch.int64, device=Q.device)
    torch.cuda.synchronize()
    t0 = time.time()
    for q0 in range(0, Q.shape[0], qc):
        best_v = best_i = None
        for c0 in range(0, I.shape[0], cc):
            S = torch.matmul(Q[q0:q0 + qc], I[c0:c0 + cc].T)
            v, i = torch.topk(S, min(K, S.shape[1]), dim=1)
            i += c0
            if best_v is not None:
                v, i = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
                v, sel = torch.topk(v, K, dim=1)
                i = torch.gather(i, 1, sel)
            best_v, best_i = v, i
        out[q0:q0 + qc] = best_i
    torch.cuda.synchronize()
    return out, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--items", type=int, default=1000000)
    ap.add_argument("--keys", type=int, default=262144)
    ap.add_argument("--row-ids", type=int, default=39)
    ap.add_argument("--item-ids", type=int, default=4)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--v-dim", type=int, default=64)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--q-chunk", type=int, default=8192)
    ap.add_argument("--c-chunk", type=int, default=65536)
    ap.add_argument("--rec-split", type=int, default=0, help="the sweep's item splits (0: chosen from the grid)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32", help="bf16: variant A_bf16 beside A, with its recall")
    ap.add_argument("--shortlist", type=int, default=0, help="rec_shortlist of A_bf16 (0: min(64, max(16, 4 topk)))")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick B out")
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32 matrix peak of the box (MI355X: 157.3)")
    a = ap.parse_args()
    import torch
    from difacto_amd import capi
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    torch.backends.cuda.matmul.allow_tf32 = False
    nq, M, n, k, K = a.rows, a.items, a.keys, a.v_dim, a.topk
    rng = np.random.default_rng(1)
    ctx = capi.Context(0)
    tb = capi.Table(ctx, n + n // 2 + 1024, V_dim=k, init_mode=capi.INIT_HASH)
    ids = np.arange(1, n + 1, dtype=U64) * U64(2654435761)
    w, V = (rng.normal(size=n) * 0.1).astype(np.float32), (rng.normal(size=(n, k)) * 0.05).astype(np.float32)
    for r0 in range(0, n, 100000):
        m = min(100000, n - r0)
        scal = np.zeros((m, 4), np.float32)
        scal[:, 1] = w[r0:r0 + m]
        tb.import_(rev(ids[r0:r0 + m]), scal, np.ones(m, np.int32), np.concatenate([V[r0:r0 + m], np.zeros((m, k), np.float32)], 1))
    qidx, iidx = rng.integers(0, n, (nq, a.row_ids)), rng.integers(0, n, (M, a.item_ids))
    b = capi.Batch(ctx, a.batch, a.batch * max(a.row_ids, a.item_ids))

    def feed(idx, call):
        for r0 in range(0, idx.shape[0], a.batch):
            blk = idx[r0:r0 + a.batch]
            b.load_host(np.arange(blk.shape[0] + 1, dtype=np.int64) * blk.shape[1], ids[blk.ravel()], None, np.ones(blk.shape[0], np.float32))
            b.localize()
            b.lookup(tb)
            b.sgd_step(tb, is_train=False)
            call(b, tb)

    ctx.set_option("rec_split", a.rec_split)
    rec = capi.Recommend(ctx, K, capacity_hint=M)
    recb = None
    if a.precision == "bf16":   # the options are read at creation
        ctx.set_option("rec_precision", 1)
        ctx.set_option("rec_shortlist", a.shortlist)
        recb = capi.Recommend(ctx, K, capacity_hint=M)
        ctx.set_option("rec_precision", 0)
        feed(iidx, recb.add_items)
        feed(qidx[:a.batch], recb.append_batch)
        recb.read()
    ctx.set_timing(True)
    t0 = time.time()
    feed(iidx, rec.add_items)
    ctx.sync()
    cat_wall = time.time() - t0
    tm = ctx.get_timing(reset=True)
    assert rec.item_count() == M
    # the yardstick's operands, from the same model
    Vt, wt = torch.from_numpy(V).cuda(), torch.from_numpy(w).cuda()

    def operands(idx, bias_is_one):
        out = torch.empty((idx.shape[0], k + 1), dtype=torch.float32, device="cuda")
        for r0 in range(0, idx.shape[0], 100000):
            j = torch.from_numpy(idx[r0:r0 + 100000]).cuda()
            rows = Vt[j]
            S = rows.sum(1)
            out[r0:r0 + 100000, :k] = S
            out[r0:r0 + 100000, k] = 1.0 if bias_is_one else wt[j].sum(1) + 0.5 * (S * S - (rows * rows).sum(1)).sum(1)
        return out

    Q, I = operands(qidx, True), operands(iidx, False)
    feed(qidx[:a.batch], rec.append_batch)   # warm-up of both
    rec.read()
    if not a.no_torch:
        torch_topk(torch, Q[:4096], I[:min(M, 2 * a.c_chunk)], K, a.q_chunk, a.c_chunk)
    ctx.get_timing(reset=True)
    print(json.dumps(dict(setup=True, rows=nq, items=M, V_dim=k, topk=K, batch=a.batch, rec_split=a.rec_split, catalogue_wall_s=cat_wall,
                          catalogue_rec_embed_ms=tm["rec_embed"][0])), flush=True)
    names = ("rec_embed", "rec_sweep", "rec_merge")
    runs = {"A": [], "B": []}
    for rnd in range(a.rounds):
        rec.reset()
        t0 = time.time()
        feed(qidx, rec.append_batch)
        got = rec.read()
        wall = time.time() - t0
        tm = ctx.get_timing(reset=True)
        o = dict(variant="A", round=rnd, wall_s=wall, nonfinite=got["nonfinite"], **{x + "_ms": tm[x][0] for x in names})
        o["kernels_s"] = sum(o[x + "_ms"] for x in names) / 1e3
        print(json.dumps(o), flush=True)
        runs["A"].append(o)
        if recb is not None:
            recb.reset()
            t0 = time.time()
            feed(qidx, recb.append_batch)
            gb = recb.read()
            wall = time.time() - t0
            tm = ctx.get_timing(reset=True)
            nb = ("rec_embed", "rec_convert", "rec_cand", "rec_rescore")
            slot = np.arange(K)
            same = (got["items"][:, :, None] == gb["items"][:, None, :]) & (slot[None, None, :] < gb["n"][:, None, None])
            kept = int((same.any(2) & (slot[None, :] < got["n"][:, None])).sum())
            o = dict(variant="A_bf16", round=rnd, shortlist=a.shortlist, wall_s=wall, rows_per_s=nq / wall, nonfinite=gb["nonfinite"],
                     recall=kept / max(int(got["n"].sum()), 1), **{x + "_ms": tm[x][0] for x in nb})
            o["kernels_s"] = sum(o[x + "_ms"] for x in nb) / 1e3
            print(json.dumps(o), flush=True)
            runs.setdefault("A_bf16", []).append(o)
        if a.no_torch:
            continue
        idx, sec = torch_topk(torch, Q, I, K, a.q_chunk, a.c_chunk)
        same = (np.sort(got["items"].astype(np.int64), 1) == np.sort(idx.cpu().numpy(), 1)).all(1).mean()
        o = dict(variant="B", round=rnd, wall_s=sec, rows_with_the_same_item_set=float(same))
        print(json.dumps(o), flush=True)
        runs["B"].append(o)
    kd = (k + 1 + 7) // 8 * 8
    sweep = sorted(o["rec_sweep_ms"] / 1e3 for o in runs["A"])
    flop, useful = 2.0 * nq * M * kd, 2.0 * nq * M * (k + 1)
    if recb is not None:
        print(json.dumps(dict(summary_bf16=True, shortlist=a.shortlist, kernels_s=sorted(round(o["kernels_s"], 4) for o in runs["A_bf16"]),
                              wall_s=sorted(round(o["wall_s"], 4) for o in runs["A_bf16"]), recall=[round(o["recall"], 5) for o in runs["A_bf16"]],
                              fp32_kernels_s=sorted(round(o["kernels_s"], 4) for o in runs["A"]),
                              fp32_wall_s=sorted(round(o["wall_s"], 4) for o in runs["A"]))), flush=True)
        recb.close()
    print(json.dumps(dict(summary=True, rows=nq, items=M, V_dim=k, kd=kd, topk=K,
                          A_kernels_s=sorted(round(o["kernels_s"], 4) for o in runs["A"]),
                          A_wall_s=sorted(round(o["wall_s"], 4) for o in runs["A"]), B_wall_s=sorted(round(o["wall_s"], 4) for o in runs["B"]),
                          sweep_ms=[round(1e3 * x, 3) for x in sweep],
                          A_kernels_over_B_wall=[round(x["kernels_s"] / y["wall_s"], 4) for x, y in zip(runs["A"], runs["B"])],
                          sweep_tflops_executed=[round(flop / s / 1e12, 2) for s in sweep],
                          sweep_share_of_fp32_matrix_peak_executed=[round(flop / s / 1e12 / a.peak_tflops, 4) for s in sweep],
                          sweep_share_of_fp32_matrix_peak_useful=[round(useful / s / 1e12 / a.peak_tflops, 4) for s in sweep])), flush=True)
    rec.close()
    b.close()
    tb.close()
    ctx.close()


if __name__ == "__main__":
    main()
