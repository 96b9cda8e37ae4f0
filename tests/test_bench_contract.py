"""The bench line contract, checked on the line committed under profiles/ (produced by
`python bench.py --full` on an MI355X): every key a reader of the line relies on is there, with the
types and the relations the contract states."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def newest(pattern, fallback):
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return found[-1] if found else os.path.join(ROOT, "profiles", fallback)


def test_committed_bench_line_has_the_contract_keys():
    d = json.loads(open(newest("r*_bench_c3.json", "r01_bench_default.json")).read().strip().splitlines()[-1])
    for k, typ in dict(metric=str, value=float, unit=str, n_gpus=int, steps=int, warmup=int, ms_per_step=float,
                       higher_is_better=bool, scaling=str, dtype=str, data=str, config=dict).items():
        assert isinstance(d[k], typ), k
    assert d["vs_baseline"] is None            # BASELINE.md has no published number for this metric
    assert d["unit"] == "examples/sec" and d["scaling"] == "weak" and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    # value = units processed / time
    assert abs(d["value"] - d["config"]["rows_per_step"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-6
    assert r["traffic"] is None or r["traffic"] < 1.2 * r["algorithmic_bytes_per_launch"]   # no wasted re-reads
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["unit"] == "examples/sec"


def test_pmc_summary_feeds_the_traffic_field():
    t = json.load(open(newest("r*_pmc_hbm_traffic.json", "r01_pmc_hbm_traffic.json")))
    fwd = [v for k, v in t.items() if k.startswith("k_forward<")]
    assert len(fwd) == 1 and fwd[0]["hbm_bytes_per_launch"] > 0


def test_committed_sharded_line_has_the_same_shape():
    """the N > 1 line (difacto_amd/sharded.py; here its one-rank run over RCCL, `bench.py --force-sharded`) carries
    what the N = 1 line carries — cpu_baseline, roofline with a traffic figure and its source, and the exchange priced
    against the xGMI links — so that the first run on a multi-GPU node counts"""
    d = json.loads(open(newest("r0[4-9]*_bench_sharded_w1_full.json", "r04z_bench_sharded_w1_full.json")).read().strip().splitlines()[-1])
    for k, typ in dict(metric=str, value=float, unit=str, n_gpus=int, steps=int, warmup=int, ms_per_step=float,
                       higher_is_better=bool, scaling=str, dtype=str, data=str, config=dict).items():
        assert isinstance(d[k], typ), k
    assert d["vs_baseline"] is None and d["scaling"] == "weak" and d["dtype"] == "f32"
    c = d["cpu_baseline"]
    assert c and c["kind"] in ("reference", "port") and c["value"] > 0 and c["cores"] >= 1 and "sample" in c
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] and r["traffic_source"].startswith("profiles/")
    x = d["roofline_exchange"]
    for k in ("bound", "bytes_per_gpu_step", "exchange_ms_per_step", "achieved", "peak", "unit", "frac", "links_in_use"):
        assert k in x, k
    assert x["bound"] == "xgmi" and abs(x["peak"] - 7 * 153.6) < 1e-9
    assert "rccl" in d["config"]["transport_bound"] and d["config"]["auc_every_minibatch"] is True
    assert set(d["stage_ms_per_step"]) == {"counts", "L", "K", "R", "RW", "F", "G", "P"}


def test_device_id_generation_matches_the_host_generator():
    """bench.py --emulate-world on a 1e9-id space (C5) fills the emulated rank's shard from ids generated with torch int64
    arithmetic on the device; the same code on the CPU must give the host generator's reversed keys, range filter included"""
    import numpy as np
    import torch
    from difacto_amd import sharded, synth
    g = synth.CriteoSynth(total_ids=300_000, seed=42)
    allk = np.concatenate([synth.reverse_bytes_np(g.all_ids(q)) for q in range(synth.NUM_SLOTS)])
    for lo, hi in ((0, 1 << 64), (3 << 60, 9 << 60), (9 << 60, 1 << 64)):
        want = np.sort(allk[(allk >= np.uint64(lo)) & (allk <= np.uint64(hi - 1))])
        got = np.sort(np.concatenate([t.numpy().view(np.uint64) for t in
                                      sharded._device_owned_keys(g, lo, hi, torch.device("cpu"), chunk=1 << 14)] + [np.zeros(0, np.uint64)]))
        assert np.array_equal(want, got)


def test_blended_key_ranges():
    """the three kinds of key ranges of the N > 1 bench: shares of rows and of per-step traffic per owner"""
    import numpy as np
    from difacto_amd import sharded, synth

    class A:
        rows, blend_alpha = 2000, 0.5
    out = {}
    for mode in ("ids", "data", "blend"):
        a = A()
        a.key_ranges = mode
        splits, m = sharded.bench_splits(a, 8, lambda: synth.CriteoSynth(total_ids=2_000_000, seed=42), synth.NUM_SLOTS)
        assert m == mode and len(splits) == 7 and np.all(splits[1:] >= splits[:-1])
        out[mode] = a.range_shares
    assert max(out["ids"]["rows"]) < 0.14 and max(out["data"]["traffic"]) < 0.14      # each balances what it is named after
    assert max(out["ids"]["traffic"]) > 0.18 and max(out["data"]["rows"]) > 0.18      # ... and not the other
    assert max(out["blend"]["rows"]) < max(out["data"]["rows"]) and max(out["blend"]["traffic"]) < max(out["ids"]["traffic"])


def test_committed_projection_line_says_what_it_is():
    """bench.py --emulate-world: a projection must never read like a measurement of N GPUs — it is marked, says
    which ranks were emulated on how many GPUs, carries all three wire models with their assumptions, and per rank the
    stage times, the bytes per GPU-step and the key counts the projection rests on"""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_emul_c4_w8*.json")))
    assert paths
    d = json.loads(open(paths[-1]).read().strip().splitlines()[-1])
    assert d["projection"] is True and d["n_gpus"] == 1 and d["emulated_world"] == 8 and d["vs_baseline"] is None
    assert "PROJECTED" in d["metric"] and "NOT a measurement" in d["value_note"]
    assert set(d["projected_examples_per_sec"]) <= {"off", "peak", "achievable"} and d["projected_examples_per_sec"]
    assert d["wire_models"]["peak"]["link_gbps_per_direction"] == 76.8 and "assumed" in d["wire_model_note"]
    for r in d["ranks"]:
        assert r["keys_in_per_batch"] > 0 and r["remote_keys_out_per_batch"] > 0 and r["owned_keys"] > 0
        assert set(r["bytes_per_gpu_step"]) == {"K_out", "K_in", "RW_out", "RW_in", "G_out", "G_in"}
        for m in r["models"].values():
            assert m["ms_per_step"] > 0 and m["bytes_sent_per_step"] > 0 and m["bytes_recv_per_step"] > 0
    assert d["value"] == d["projected_examples_per_sec"][[m for m in ("achievable", "peak", "off") if m in d["projected_examples_per_sec"]][0]] \
        or d["value"] in d["projected_examples_per_sec"].values()


def test_committed_default_line_carries_the_request_ceiling():
    """round 5: `roofline_requests` (the step against the chip's rate for random memory-side requests) and the two new
    `secondary` entries (first epoch on an empty table; the reference's quick-start shape with ITS CPU baseline)"""
    d = json.loads(open(newest("r0[5-9]*_bench_c3.json", "r05z_bench_c3.json")).read().strip().splitlines()[-1])
    q = d["roofline_requests"]
    assert q["per_step"] > 3e6 and 0.3 < q["frac"] < 1.0 and abs(q["frac"] - q["per_s"] / q["ceiling_per_s"]) < 1e-9
    assert q["per_step_source"].startswith("profiles/") and q["ceiling_source"].startswith("profiles/")
    sec = d["secondary"]
    assert sec["c3-cold"]["config"]["prefilled"] is False and sec["c3-cold"]["steps"] == 256 and sec["c3-cold"]["warmup"] == 0
    c2 = sec["c2"]
    assert c2["cpu_baseline"]["kind"] in ("reference", "port") and c2["value"] > 5 * c2["cpu_baseline"]["value"]


def test_committed_dry_run_line_carries_the_wire_probe():
    """`bench.py --gpus N` measures the wires before its timed region (dfh_comm_wire_probe: grouped all-to-all
    of fixed sizes per peer on the library's own communicator), so that the first run on a real node replaces the assumed
    link rate of the projection by itself.  Checked on the committed 8-rank dry run (ranks sharing one GPU, exchange staged
    over gloo: the rates are the host's, the block's shape is the real run's)."""
    d = json.loads(open(newest("r0[6-9]*_dryrun_shared_gpu_w8.json", "r06z_dryrun_shared_gpu_w8.json")).read().strip().splitlines()[-1])
    assert d["n_gpus"] == 8 and d["lr_divided_by_world"] == 8 and d["value"] > 0
    wp = d["wire_probe"]
    assert wp["peers"] == 7 and len(wp["per_size"]) >= 2
    for p in wp["per_size"]:
        assert p["bytes_per_peer"] > 0 and p["us_per_grouped_exchange"] > 0
        assert abs(p["gbps_per_link_and_direction"] - p["bytes_per_peer"] / p["us_per_grouped_exchange"] / 1e3) < 1e-9
    x = d["roofline_exchange"]
    best = max(p["gbps_per_link_and_direction"] for p in wp["per_size"])
    assert abs(x["measured_wire_gbps_per_link_and_direction"] - best) < 1e-12
    assert abs(x["frac_of_measured_wire"] - x["achieved"] / (2.0 * 7 * best)) < 1e-9
