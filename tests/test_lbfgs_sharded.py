"""learner = lbfgs over several ranks (dfh_lbfgs_create_sharded): every rank a worker for its part of the rows and the
owner of one key range of the model.  The ranks share the one GPU of the test box, through DIFACTO_COMM=file (the CLI) or
a gloo callback communicator (the C ABI); at most 4 ranks per test."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
BASIC_ARGS = ["m=5", "V_dim=0", "l2=0", "init_alpha=1", "tail_feature_filter=0", "max_num_epochs=19"]
MIXED_ARGS = ["V_dim=4", "V_threshold=2", "tail_feature_filter=2", "max_num_epochs=6"]


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _rank_env(world, rank, rv):
    return dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER=str(world), DIFACTO_RANK=str(rank), DIFACTO_DEVICE="0",
                DIFACTO_COMM="file", DIFACTO_RENDEZVOUS=rv)


def _run_ranks(built, world, args, tmp_path, tag, exe="difacto", learner="learner=lbfgs"):
    """one process per rank on the one GPU, the file transport; -> every rank's stderr"""
    rv = os.path.join(str(tmp_path), "rv_" + tag)
    os.makedirs(rv)
    procs = [subprocess.Popen([os.path.join(built, exe), learner] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=ROOT, env=_rank_env(world, r, rv)) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[1])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, err) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d: %s" % (r, err[-3000:])
    return outs


def _plain(built, args):
    r = subprocess.run([os.path.join(built, "difacto"), "learner=lbfgs"] + list(args), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _lines(log):
    """the scheduler's lines about the objective, without the log prefix"""
    return [l.split("] ", 1)[-1] for l in log.splitlines() if "objv" in l]


def _accepted(log):
    out, last = [], None
    for line in log.splitlines():
        m = re.search(r" - alpha = \S+, objv = (\S+), <p,g> = ", line)
        if m:
            last = float(m.group(1))
        if "wolfe condition is satisifed" in line or "reach the maximal number of linesearch steps" in line:
            out.append(last)
    return out


def _export_file(path, k):
    from difacto_amd import capi
    ctx = capi.Context(0)
    t = capi.Table(ctx, 1 << 16, V_dim=k)
    t.load(path)
    e = t.export()
    t.close()
    ctx.close()
    o = np.argsort(e["keys"])
    return {n: e[n][o] for n in ("keys", "scal", "has_V", "V")}


def _export_parts(prefix, k):
    nparts = int(open(prefix + ".parts").read())
    es = [_export_file("%s.part-%d" % (prefix, r), k) for r in range(nparts)]
    e = {n: np.concatenate([x[n] for x in es]) for n in es[0]}
    o = np.argsort(e["keys"])
    return {n: v[o] for n, v in e.items()}, nparts


# ------------------------------------------------------------------------------------------------ refusals (no GPU)
def test_server_role_is_refused(built):
    env = dict(os.environ, DMLC_ROLE="server", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_RENDEZVOUS="/nonexistent")
    r = subprocess.run([os.path.join(built, "difacto"), "learner=lbfgs", "data_in=" + DATA, "V_dim=0"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and "DMLC_ROLE=server: this build runs workers only" in r.stderr


def test_incomplete_worker_env_keeps_the_refusal(built):
    """DIFACTO_RENDEZVOUS missing: not the sharded mode, the single-GPU refusal word for word"""
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="1")
    env.pop("DIFACTO_RENDEZVOUS", None)
    r = subprocess.run([os.path.join(built, "difacto"), "learner=lbfgs", "data_in=" + DATA, "V_dim=0"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and "learner = lbfgs runs in one process on one GPU" in r.stderr


def test_bcd_with_a_complete_worker_env_is_still_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = subprocess.run([os.path.join(built, "difacto"), "learner=bcd", "data_in=" + DATA], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode != 0 and "learner = bcd runs in one process on one GPU" in r.stderr


# ------------------------------------------------------------------------------------------------ the command line
@pytest.mark.gpu
def test_world1_sharded_prints_the_plain_bits(built, tmp_path):
    args = ["data_in=" + DATA] + MIXED_ARGS
    plain = _plain(built, args + ["model_out=" + str(tmp_path / "plain")])
    one = _run_ranks(built, 1, args + ["model_out=" + str(tmp_path / "one")], tmp_path, "w1")[0]
    assert "rank 0 of 1 connected (file transport)" in one
    assert len(_lines(plain)) > 10 and _lines(one) == _lines(plain)
    a = _export_file(str(tmp_path / "plain"), 4)
    b, nparts = _export_parts(str(tmp_path / "one"), 4)
    assert nparts == 1
    for n in a:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_basic_trajectory_lockstep_and_repeatable(built, tmp_path, world):
    from test_lbfgs_learner import BASIC
    args = ["data_in=" + DATA] + BASIC_ARGS
    logs = _run_ranks(built, world, args, tmp_path, "a")
    for r in range(1, world):
        assert _lines(logs[r]) == _lines(logs[0]), r
    acc = _accepted(logs[0])
    assert len(acc) == 19
    for got, want in zip(acc, BASIC):
        assert abs(got - want) <= 1e-5 + 5e-6 * abs(want), (got, want)
    assert "found 100 training examples" in logs[0]
    again = _run_ranks(built, world, args, tmp_path, "b")
    assert all(_lines(again[r]) == _lines(logs[0]) for r in range(world))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_mixed_lens_follows_world1(built, tmp_path, world):
    args = ["data_in=" + DATA] + MIXED_ARGS
    want = _accepted(_plain(built, args))
    logs = _run_ranks(built, world, args, tmp_path, "m")
    got = _accepted(logs[0])
    assert len(got) == len(want) >= 3
    for r in range(1, world):
        assert _lines(logs[r]) == _lines(logs[0]), r
    np.testing.assert_allclose(got, want, rtol=1e-4)


def _fm_forward(path, e, k):
    from difacto_amd import capi
    from test_lbfgs_learner import fm_forward
    return fm_forward(path, e, k, capi.reverse_bytes)


@pytest.mark.gpu
def test_model_parts_score_and_reload_under_another_world(built, tmp_path):
    model = str(tmp_path / "m")
    logs = _run_ranks(built, 2, ["data_in=" + DATA, "V_dim=4", "V_threshold=2", "tail_feature_filter=0", "max_num_epochs=3",
                                 "model_out=" + model], tmp_path, "save")
    e, nparts = _export_parts(model, 4)
    assert nparts == 2 and len(np.unique(e["keys"])) == len(e["keys"])
    want = _fm_forward(DATA, e, 4)
    # the last accepted objective is loss + r(w) of the saved weights (defaults l2 = .1, V_l2 = .01)
    lab = np.array([float(l.split()[0]) for l in open(DATA) if l.split()])
    y = np.where(lab > 0, 1.0, -1.0)
    loss = np.logaddexp(0, -y * want).sum()
    reg = 0.5 * 0.1 * (e["scal"][:, 1].astype(np.float64) ** 2).sum() + \
        0.5 * 0.01 * ((e["V"][:, :4].astype(np.float64) * (e["has_V"][:, None] != 0)) ** 2).sum()
    printed = _accepted(logs[0])[-1]
    assert abs(printed - (loss + reg)) <= 1e-5 * abs(printed) + 1e-5, (printed, loss + reg)
    assert 0 < np.count_nonzero(e["has_V"]) < len(e["has_V"])
    # a sharded task = predict learner = sgd with three ranks loads the two parts; the prediction parts are consecutive
    # byte ranges of the data
    pred = str(tmp_path / "p")
    _run_ranks(built, 3, ["task=predict", "data_in=" + DATA, "V_dim=4", "V_init=hash", "batch_size=100", "model_in=" + model,
                          "pred_out=" + pred], tmp_path, "pred", learner="learner=sgd")
    got = np.concatenate([np.loadtxt("%s.part-%d" % (pred, i), dtype=np.float64, ndmin=1)
                          for i in range(100) if os.path.exists("%s.part-%d" % (pred, i))])
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_rank_without_rows_and_shards_without_keys(built, tmp_path):
    rows = [l for l in open(DATA) if l.split()][:3]
    three = tmp_path / "three.libsvm"
    three.write_text("".join(rows))
    # every row the same two features: the balanced split keys repeat and leave shards without a key
    same = tmp_path / "same.libsvm"
    same.write_text("1 3:1 7:0.5\n-1 3:1 7:0.5\n1 3:1 7:0.5\n")
    for path in (three, same):
        args = ["data_in=" + str(path), "V_dim=2", "V_threshold=0", "tail_feature_filter=0", "max_num_epochs=4"]
        want = _accepted(_plain(built, args))
        logs = _run_ranks(built, 4, args, tmp_path, path.stem)
        assert "found 3 training examples" in logs[0]
        assert any(re.search(r"rank \d: 0 training examples", l) for l in logs), path
        if path == same:
            assert any(re.search(r"owns 0 keys", l) for l in logs)
        got = _accepted(logs[0])
        assert len(got) == len(want) >= 1
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)
        for r in range(1, 4):
            assert _lines(logs[r]) == _lines(logs[0])


# ------------------------------------------------------------------------------------------------ the C ABI
def _rcv1_rows():
    off, idx, val, lab = [0], [], [], []
    for line in open(DATA):
        t = line.split()
        if not t:
            continue
        lab.append(float(t[0]))
        for kv in t[1:]:
            i, v = kv.split(":")
            idx.append(int(i))
            val.append(float(v))
        off.append(len(idx))
    return np.array(off, np.uint64), np.array(idx, np.uint64), np.array(val, np.float32), np.array(lab, np.float32)


def _add_rows(obj, data, r0, r1):
    off, idx, val, lab = data
    if r1 <= r0:
        return
    o = off[r0:r1 + 1]
    obj.add_chunk(o - o[0], idx[o[0]:o[-1]], val[o[0]:o[-1]], lab[r0:r1])


STATE = dict(K=3, filter=1.0, vth=2, scale=0.5, l2=0.1, V_l2=0.01, m=4, epochs=3)


def _drive(obj):
    """the scheduler's calls for a few epochs at fixed steps: incr_B and <p, g> of every epoch"""
    out = []
    obj.calc_grad()
    for ep in range(STATE["epochs"]):
        incr = obj.prepare_direction()
        coef = None
        if incr is not None:
            k = (len(incr) - 1) // 6
            coef = np.linspace(-0.5, 0.5, 2 * k + 1).astype(np.float32)   # any coefficients: the same on every side
        pg = obj.calc_direction(coef)
        f, pg2, auc = obj.line_search(0.5 if ep else 0.05)
        out.append(dict(incr=None if incr is None else incr.copy(), pg=pg, f=f, pg2=pg2, auc=auc, ev=obj.evaluate()))
    return out


def _state_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from difacto_amd import capi
    ctx = capi.Context(0)

    def exchange(send, sb, recv, rb):
        out = torch.empty(sum(rb), dtype=torch.uint8)
        dist.all_to_all_single(out, torch.from_numpy(np.array(send, copy=True)), output_split_sizes=rb, input_split_sizes=sb)
        recv[:] = out.numpy()

    comm = capi.Comm.callback(ctx, rank, world, exchange)
    data = _rcv1_rows()
    n = len(data[3])
    obj = capi.Lbfgs(ctx, STATE["K"], STATE["m"], comm=comm)
    lo, hi = rank * n // world, (rank + 1) * n // world
    mid = (lo + hi) // 2   # two chunks per rank
    _add_rows(obj, data, lo, mid)
    _add_rows(obj, data, mid, hi)
    obj.init_model(STATE["filter"], STATE["vth"], STATE["scale"], STATE["l2"], STATE["V_l2"])
    m = obj.get_model()
    comm.stats(reset=True)
    trace = _drive(obj)
    sent = comm.stats()[0]
    np.savez(os.path.join(out_dir, "state%d.npz" % rank), sent=sent, **m)
    import pickle
    pickle.dump(trace, open(os.path.join(out_dir, "trace%d.pkl" % rank), "wb"))
    obj.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_state_shards_concatenate_to_the_single_model(tmp_path, world):
    import pickle
    import torch.multiprocessing as mp
    from difacto_amd import capi
    port = 29400 + (os.getpid() % 200) + world
    mp.spawn(_state_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    ctx = capi.Context(0)
    one = capi.Lbfgs(ctx, STATE["K"], STATE["m"])
    data = _rcv1_rows()
    _add_rows(one, data, 0, len(data[3]))
    one.init_model(STATE["filter"], STATE["vth"], STATE["scale"], STATE["l2"], STATE["V_l2"])
    want = one.get_model()
    single = _drive(one)
    one.close()
    ctx.close()
    parts = [np.load(os.path.join(tmp_path, "state%d.npz" % r)) for r in range(world)]
    for name in ("keys", "lens", "cnt", "w"):
        got = np.concatenate([p[name] for p in parts])
        assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), name
    assert np.any(want["lens"] > 1) and np.any(want["lens"] == 1)
    assert all(len(p["keys"]) for p in parts) and all(int(p["sent"]) > 0 for p in parts)
    traces = [pickle.load(open(os.path.join(tmp_path, "trace%d.pkl" % r), "rb")) for r in range(world)]
    for r in range(1, world):   # the same bits on every rank
        for a, b in zip(traces[0], traces[r]):
            assert (a["incr"] is None and b["incr"] is None) or np.array_equal(a["incr"], b["incr"])
            assert (a["pg"], a["f"], a["pg2"], a["auc"], a["ev"]) == (b["pg"], b["f"], b["pg2"], b["auc"], b["ev"])
    for a, s in zip(traces[0], single):
        if s["incr"] is not None:
            np.testing.assert_allclose(a["incr"], s["incr"], rtol=1e-6, atol=1e-6 * np.abs(s["incr"]).max())
        for key in ("pg", "f", "pg2"):
            assert a[key] == pytest.approx(s[key], rel=1e-6, abs=1e-9), key
