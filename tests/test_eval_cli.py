"""exact_metrics = 1 of the command line (host/sgd_learner.cc): validation epochs and task = predict report the exact AUC,
logloss and accuracy of the whole set in one more log line (the device evaluator, csrc/dfh_eval.hip).  No GPU: what Init
refuses before the device is touched.  GPU: the `whole file:` line of a prediction against the oracle of tests/eval_ref.py
applied to pred_out and the file's labels, one `Validation (whole set)` line per epoch, nothing new with the key absent."""
import os
import re
import subprocess

import numpy as np
import pytest

import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
FIELDS = r"rows=(\d+) pos=(\d+) neg=(\d+) nan=(\d+) auc2=(\d+) auc=(\S+) logloss=(\S+) accuracy=(\S+)$"


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _difacto(built, *args, env=None, timeout=300):
    return subprocess.run([os.path.join(built, "difacto"), "data_in=" + DATA, "batch_size=10", "V_dim=4"] + list(args),
                          capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: refused in Init, before the device is touched
# ---------------------------------------------------------------------------------------------------------------------
def test_other_value_is_fatal(built):
    for v in ("2", "-1"):
        r = _difacto(built, "data_val=" + DATA, "exact_metrics=" + v)
        assert r.returncode != 0 and "exact_metrics=" + v in r.stderr and "0 (off, the default) and 1" in r.stderr, r.stderr[-2000:]


def test_a_rank_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = _difacto(built, "data_val=" + DATA, "exact_metrics=1", env=env)
    assert r.returncode != 0 and "exact_metrics=1 with a sharded store" in r.stderr and "DMLC_ROLE" in r.stderr, r.stderr[-2000:]
    assert "run one process, or leave exact_metrics out" in r.stderr


def test_literal_path_is_refused(built):
    r = _difacto(built, "data_val=" + DATA, "exact_metrics=1", "device_path=literal")
    assert r.returncode != 0 and "exact_metrics=1 with device_path=literal" in r.stderr, r.stderr[-2000:]
    assert "device_path=fused, or leave exact_metrics out" in r.stderr


def test_training_without_validation_data_is_refused(built):
    r = _difacto(built, "exact_metrics=1")
    assert r.returncode != 0 and "exact_metrics=1 with task=train and no data_val" in r.stderr, r.stderr[-2000:]
    assert "data_val=<file>, or leave exact_metrics out" in r.stderr


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
# (a model that ranks some pairs wrong and ties others: measured, the whole-set AUC of the last epoch is 0.80)
TRAIN = ["max_num_epochs=3", "num_jobs_per_epoch=2", "V_threshold=2", "l1=2", "lr=.05", "stop_rel_objv=0", "stop_val_auc=-1e30"]


@pytest.fixture(scope="module")
def model(built, tmp_path_factory):
    """three epochs with validation and exact_metrics = 1: (the log, the model)"""
    path = str(tmp_path_factory.mktemp("eval_cli") / "model")
    r = _difacto(built, "data_val=" + DATA, "exact_metrics=1", "model_out=" + path, *TRAIN)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr, path


def _labels():
    return np.array([float(l.split()[0]) for l in open(DATA) if l.split()], np.float32)


def _parse(line):
    m = re.search(FIELDS, line)
    assert m, line
    return [int(x) for x in m.groups()[:5]] + list(m.groups()[5:])


@pytest.mark.gpu
def test_predict_reports_the_whole_file(built, model, tmp_path):
    _, path = model
    out = {}
    for tag, extra in (("with", ["exact_metrics=1"]), ("without", []), ("zero", ["exact_metrics=0"])):
        pred = str(tmp_path / ("pred_" + tag))
        r = _difacto(built, "task=predict", "learner=sgd", "model_in=" + path, "pred_out=" + pred, "num_jobs_per_epoch=3", *extra)
        assert r.returncode == 0, r.stderr[-3000:]
        out[tag] = (r.stderr, open(pred, "rb").read())
    for tag in ("without", "zero"):
        assert "whole file:" not in out[tag][0] and "whole set" not in out[tag][0]
        assert out[tag][1] == out["with"][1], "pred_out does not depend on the key"
    log = out["with"][0]
    lines = [l for l in log.splitlines() if "whole file: " in l]
    assert len(lines) == 1, log[-3000:]
    assert len(re.findall(r"against their labels", log)) == 1, "the existing line stays"
    rows, pos, neg, nan, auc2, auc, logloss, acc = _parse(lines[0])
    pred = np.loadtxt(str(tmp_path / "pred_with"), dtype=np.float64).astype(np.float32)   # %.9g round-trips float32
    label = _labels()
    assert np.unique(pred).size > 10
    want = R.oracle(label, pred)
    print(lines[0], want)
    assert (rows, pos, neg, nan, auc2) == (want.n, want.n_pos, want.n_neg, want.n_nan, want.auc2) and rows == 100 and nan == 0
    assert float(auc) == want.auc2 / (2.0 * want.n_pos * want.n_neg) and auc == "%.17g" % float(auc)
    assert float(acc) == want.correct / 100
    assert abs(float(logloss) * 100 - want.objv) <= (100 + 16) * 2.0 ** -52 * want.sum_abs + 2.0 ** -52 * want.objv   # (+ the division)


@pytest.mark.gpu
def test_one_validation_line_per_epoch(model):
    log, _ = model
    lines = [l for l in log.splitlines() if " - Validation (whole set): " in l]
    epochs = len(re.findall(r" - Validation: ", log))
    assert epochs == 3 and len(lines) == epochs, log[-3000:]
    label = _labels()
    for l in lines:
        rows, pos, neg, nan, auc2, auc, logloss, acc = _parse(l)
        assert (rows, pos, neg, nan) == (100, int((label > 0).sum()), int((label <= 0).sum()), 0)
        assert 0 <= auc2 <= 2 * pos * neg and float(auc) == auc2 / (2.0 * pos * neg)
        assert 0 < float(logloss) < 10 and 0 <= float(acc) <= 1
    assert "whole file:" not in log


@pytest.mark.gpu
def test_key_absent_changes_no_line(built, model, tmp_path):
    """the same training without the key: every Training / Validation line as with it, no whole-set line"""
    log, _ = model
    r = _difacto(built, "data_val=" + DATA, "model_out=" + str(tmp_path / "m"), *TRAIN)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "whole set" not in r.stderr and "whole file" not in r.stderr
    pick = lambda s: re.findall(r" - (Training: .*|Validation: .*)$", s, re.M)   # noqa: E731
    assert len(pick(r.stderr)) == 6 and pick(r.stderr) == pick(log)


@pytest.mark.gpu
def test_predict_of_a_bcd_model_reports_the_whole_file(built, tmp_path):
    """task = predict learner = bcd is scored by the SGD learner: it gets the line too"""
    m, pred = str(tmp_path / "m"), str(tmp_path / "p")
    exe = os.path.join(built, "difacto")
    r = subprocess.run([exe, "learner=bcd", "data_in=" + DATA, "max_num_epochs=2", "l1=.1", "lr=.8", "block_ratio=1",
                        "tail_feature_filter=0", "model_out=" + m], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "task=predict", "learner=bcd", "data_in=" + DATA, "batch_size=30", "model_in=" + m, "pred_out=" + pred,
                        "exact_metrics=1"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stderr.splitlines() if "whole file: " in l]
    assert len(lines) == 1, r.stderr[-3000:]
    rows, pos, neg, nan, auc2, auc, logloss, acc = _parse(lines[0])
    want = R.oracle(_labels(), np.loadtxt(pred, dtype=np.float64).astype(np.float32))
    print(lines[0], want)
    assert (rows, pos, neg, nan, auc2) == (want.n, want.n_pos, want.n_neg, want.n_nan, want.auc2) and rows == 100
    assert float(auc) == want.auc2 / (2.0 * want.n_pos * want.n_neg) and float(acc) == want.correct / 100
