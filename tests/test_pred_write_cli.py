"""pred_write = host | device of the command line (host/sgd_learner.cc): with `device` a task = predict job reads through the
device feed, keeps its predictions on the device and has them turned into text there (csrc/dfh_predtext.hip), a unit of
pred_unit_rows rows at a time; pred_out has the same bytes under both values.  No GPU: what Init refuses before the device is
touched.  GPU: byte-identical files over pred_prob, batch_size, num_jobs_per_epoch and pred_unit_rows, the job's log line
(rows and units formatted on the device / on the host), the whole-file line of exact_metrics = 1 beside it, a file whose
tiny predictions the device hands back to the host, and a learner = bcd model."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
LINE = r"pred_write=device: (\d+) rows in (\d+) units formatted on the device, (\d+) rows in (\d+) units on the host"


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _difacto(built, *args, env=None, data=DATA, timeout=300):
    size = [] if any(a.startswith("batch_size=") for a in args) else ["batch_size=10"]
    return subprocess.run([os.path.join(built, "difacto"), "data_in=" + data, "V_dim=4"] + size + list(args),
                          capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: refused in Init, before the device is touched
# ---------------------------------------------------------------------------------------------------------------------
def test_other_value_is_fatal(built):
    r = _difacto(built, "task=predict", "model_in=none", "pred_out=none", "pred_write=gpu")
    assert r.returncode != 0 and "pred_write=gpu" in r.stderr and "host (the default) and device" in r.stderr, r.stderr[-2000:]


def test_training_is_refused(built):
    r = _difacto(built, "task=train", "pred_write=device")
    assert r.returncode != 0 and "pred_write=device with task=train" in r.stderr and "nothing is predicted" in r.stderr, r.stderr[-2000:]
    assert "use task=predict, or leave pred_write out" in r.stderr


def test_a_rank_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = _difacto(built, "task=predict", "model_in=none", "pred_out=none", "pred_write=device", env=env)
    assert r.returncode != 0 and "pred_write=device with a sharded store" in r.stderr and "DMLC_ROLE" in r.stderr, r.stderr[-2000:]
    assert "run one process, or leave pred_write out" in r.stderr


def test_unit_of_no_rows_is_refused(built):
    r = _difacto(built, "task=predict", "model_in=none", "pred_out=none", "pred_write=device", "pred_unit_rows=0")
    assert r.returncode != 0 and "pred_unit_rows=0" in r.stderr and "1 row or more" in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
# (l1 = 0: every feature the training saw has a weight)
TRAIN = ["max_num_epochs=3", "num_jobs_per_epoch=2", "V_threshold=2", "l1=0", "lr=.05", "stop_rel_objv=0", "stop_val_auc=-1e30"]


@pytest.fixture(scope="module")
def model(built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pred_write_cli") / "model")
    r = _difacto(built, "model_out=" + path, *TRAIN)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def _predict(built, model, out, *extra, data=DATA):
    r = _difacto(built, "task=predict", "learner=sgd", "model_in=" + model, "pred_out=" + out, *extra, data=data)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr, open(out, "rb").read()


def _counts(log):
    """the jobs' log lines summed: (rows on the device, units, rows on the host, units)"""
    found = re.findall(LINE, log)
    assert found, "no pred_write=device line: " + log[-3000:]
    return tuple(sum(int(f[k]) for f in found) for k in range(4)), len(found)


# pred_prob, batch_size, num_jobs_per_epoch, pred_unit_rows (None: the default), units (None: not pinned)
CASES = [(0, 10, 1, 7, 10), (1, 37, 3, None, 3), (0, 37, 1, 100, 1), (1, 10, 3, 7, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("prob,batch,jobs,unit,units", CASES)
def test_same_bytes(built, model, tmp_path, prob, batch, jobs, unit, units):
    common = ["pred_prob=%d" % prob, "batch_size=%d" % batch, "num_jobs_per_epoch=%d" % jobs]
    hlog, host = _predict(built, model, str(tmp_path / "host"), "pred_write=host", *common)
    dlog, dev = _predict(built, model, str(tmp_path / "dev"), "pred_write=device", *common,
                         *(["pred_unit_rows=%d" % unit] if unit else []))
    assert "pred_write=device:" not in hlog
    (drows, dunits, hrows, hunits), lines = _counts(dlog)
    print(re.findall(LINE, dlog))
    assert lines == jobs, "one line per job"
    assert (drows, hrows, hunits) == (100, 0, 0)
    if units is not None:
        assert dunits == units
    assert host.count(b"\n") == 100 and len(set(host.split())) > 50
    if prob:
        assert all(0.0 < float(x) < 1.0 for x in host.split())
    assert dev == host


@pytest.mark.gpu
def test_beside_exact_metrics(built, model, tmp_path):
    hlog, host = _predict(built, model, str(tmp_path / "host"), "pred_write=host", "exact_metrics=1", "num_jobs_per_epoch=3")
    dlog, dev = _predict(built, model, str(tmp_path / "dev"), "pred_write=device", "exact_metrics=1", "num_jobs_per_epoch=3")
    whole = [re.findall(r"whole file: (.*)$", log, re.M) for log in (hlog, dlog)]
    assert len(whole[0]) == 1 and whole[0] == whole[1] and "rows=100 " in whole[0][0], (whole, dlog[-2000:])
    assert _counts(dlog)[0] == (100, 3, 0, 0)
    assert dev == host


@pytest.mark.gpu
def test_tiny_predictions_fall_back_to_the_host(built, model, tmp_path):
    """a unit that holds a value the device does not format is written by the host's fprintf, the others by the device"""
    rows = [l for l in open(DATA) if l.split()]
    freq = collections.Counter(tok.split(":")[0] for l in rows for tok in l.split()[1:])
    ids = [i for i, _ in freq.most_common(10)]
    data = str(tmp_path / "tiny.libsvm")
    with open(data, "w") as f:
        f.writelines(rows[:40])
        for k in range(60):
            f.write("1 %s:1e-30\n" % ids[k % len(ids)])
    common = ["num_jobs_per_epoch=1", "batch_size=10", "pred_unit_rows=10"]
    _, host = _predict(built, model, str(tmp_path / "host"), "pred_write=host", *common, data=data)
    vals = [float(x) for x in host.split()]
    assert len(vals) == 100 and all(0.0 < abs(v) < 5e-20 for v in vals[40:]), vals[40:]
    dlog, dev = _predict(built, model, str(tmp_path / "dev"), "pred_write=device", *common, data=data)
    assert _counts(dlog) == ((40, 4, 60, 6), 1)
    assert dev == host


@pytest.mark.gpu
def test_predict_of_a_bcd_model(built, tmp_path):
    """task = predict learner = bcd is scored by the SGD learner's prediction path: the key works there too"""
    m = str(tmp_path / "m")
    exe = os.path.join(built, "difacto")
    r = subprocess.run([exe, "learner=bcd", "data_in=" + DATA, "max_num_epochs=2", "l1=.1", "lr=.8", "block_ratio=1",
                        "tail_feature_filter=0", "model_out=" + m], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for how in ("host", "device"):
        pred = str(tmp_path / how)
        r = subprocess.run([exe, "task=predict", "learner=bcd", "data_in=" + DATA, "batch_size=30", "model_in=" + m, "pred_out=" + pred,
                            "pred_write=" + how], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        out[how] = (r.stderr, open(pred, "rb").read())
    assert _counts(out["device"][0])[0][0] == 100 and _counts(out["device"][0])[0][2] == 0
    assert out["host"][1].count(b"\n") == 100 and len(set(out["host"][1].split())) > 20
    assert out["device"][1] == out["host"][1]
