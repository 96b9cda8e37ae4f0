"""learner = lbfgs with l1 > 0 (orthant-wise L-BFGS) through the command line on tests/golden/rcv1_100.libsvm: the example
conf against the float64 optimum of a FISTA solver run inside the test (objective and support), the l1 = 0 log, the run
that stops at epoch 0 because every |g| is below l1, an FM run with mixed lens, and the parameter's range.

The final objective is evaluated in float64 on the weights the run saved (model_out), so the comparison with F* carries no
printing error; the printed value is checked against that within the six digits the log prints."""
import os
import re
import subprocess

import numpy as np
import pytest

import owlqn_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
CONF = os.path.join(ROOT, "example", "rcv1_lbfgs_l1.conf")
GAP_BOUND = 1e-4 if O.FP32_GAP_MEASURED is None else min(1e-4, 10 * O.FP32_GAP_MEASURED)


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def problem():
    """the float64 solution of the example conf: (ids, X, y, w*, F*, g*)"""
    ids, X, y = O.read_libsvm(DATA)
    w, F, g = O.fista(X, y, 0.1, 0.1, tol=1e-14)
    return ids, X, y, w, F, g


def test_float64_solution(problem):
    """the solver's own answer: F*, the support size and the coordinates the support rule leaves unjudged"""
    ids, X, y, w, F, g = problem
    assert abs(F - O.F_STAR_RCV1) <= 1e-11 * F, F
    assert X.shape == (100, 2775) and np.count_nonzero(w) == 279
    res = np.where(w != 0, g + 0.1 * np.sign(w), np.maximum(np.abs(g) - 0.1, 0))
    assert np.abs(res).max() <= 1e-12, "optimality of w*"
    judged = (np.abs(w) >= 2e-3) | (0.1 - np.abs(g) >= 5e-4)
    assert (~judged).sum() == 6
    assert abs(np.abs(O.logistic(X, y, np.zeros(X.shape[1]), 1.0)[1]).max() - 0.88) < 5e-3


def _cli(built, *args, ok=True):
    r = subprocess.run([os.path.join(built, "difacto")] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def _lines(log):
    return [l.split("] ", 1)[-1] for l in log.splitlines()]


def _accepted(log):
    """(the objective the first line search starts from, the objective each epoch's line search ends with)"""
    out, last = [], None
    start = re.search(r"start linesearch with objv = (\S+),", log)
    for line in log.splitlines():
        m = re.search(r" - alpha = \S+, objv = (\S+), <p,g> = ", line)
        if m:
            last = float(m.group(1))
        if "sufficient decrease is satisfied" in line or "wolfe condition is satisifed" in line or \
                "reach the maximal number of linesearch steps" in line:
            out.append(last)
    return (float(start.group(1)) if start else None), out


def _model(path, V_dim=0):
    """the saved model by raw feature id: {id: w}, and V rows where the key has one"""
    from difacto_amd import capi
    ctx = capi.Context(0)
    t = capi.Table(ctx, 1 << 16, V_dim=V_dim)
    try:
        t.load(path)
        e = t.export()
    finally:
        t.close()
        ctx.close()
    ids = [capi.reverse_bytes(int(k)) for k in e["keys"]]
    V = e["V"][:, :V_dim] if V_dim else None
    return ids, e["scal"][:, 1].astype(np.float64), e["has_V"] != 0, V


@pytest.mark.gpu
def test_example_conf_reaches_the_float64_optimum(built, problem, tmp_path):
    ids, X, y, ws, Fs, gs = problem
    model = str(tmp_path / "m")
    log = _cli(built, "argfile=" + CONF, "model_out=" + model).stderr
    assert "Unrecognized" not in log and log.count("c2 is unused") == 1
    f0, acc = _accepted(log)
    assert abs(f0 - 100 * np.log(2)) < 1e-3 and 1 <= len(acc) <= 30
    seq = [f0] + acc
    assert all(b <= a for a, b in zip(seq, seq[1:])), "the logged objective never increases: %s" % seq
    mids, mw, _, _ = _model(model)
    assert set(mids) <= {int(i) for i in ids}        # the file drops entries with w == 0 and no V
    w = np.zeros(len(ids))
    w[np.searchsorted(ids, np.array(mids, np.uint64))] = mw
    f, _ = O.logistic(X, y, w, 0.1)
    F = f + 0.1 * np.abs(w).sum()
    gap = (F - Fs) / Fs
    print("\nrcv1_lbfgs_l1.conf: %d epochs, F = %.12f, F* = %.12f, relative gap %.3e (bound %.3e); nnz(w) = %d of %d" % (
        len(acc), F, Fs, gap, GAP_BOUND, np.count_nonzero(w), len(w)))
    assert abs(acc[-1] - F) <= 1e-5 * F, "the printed objective %r against F of the saved weights %r" % (acc[-1], F)
    assert -1e-12 <= gap <= GAP_BOUND, gap
    big = np.abs(ws) >= 2e-3
    zero = 0.1 - np.abs(gs) >= 5e-4
    assert (~big & ~zero).sum() <= 8
    assert (np.sign(w[big]) == np.sign(ws[big])).all(), "every coordinate with |w*| >= 2e-3 is non-zero with the same sign"
    assert not w[zero].any(), "%d coordinates with l1 - |g*| >= 5e-4 are not zero" % np.count_nonzero(w[zero])
    nnz = [int(v) for v in re.findall(r" - nnz\(w\) = (\d+)", log)]
    assert len(nnz) == len(acc) and nnz[-1] == np.count_nonzero(w)


@pytest.mark.gpu
def test_l1_zero_prints_the_plain_run(built):
    args = ["learner=lbfgs", "data_in=" + DATA, "V_dim=0", "tail_feature_filter=0", "max_num_epochs=4"]
    a = _lines(_cli(built, *args).stderr)
    b = _lines(_cli(built, *args, "l1=0").stderr)
    assert a == b and any("wolfe condition" in l for l in a) and not any("nnz(w)" in l for l in a)


@pytest.mark.gpu
def test_every_gradient_below_l1_stops_at_epoch_zero(built, tmp_path):
    """l1 = 1 > max |g(0)| = 0.88: the pseudo-gradient is zero at w = 0"""
    model = str(tmp_path / "m")
    # the keys of the example conf with l1 = l2 = 1 (a key of an argfile wins over the command line's)
    log = _cli(built, "learner=lbfgs", "data_in=" + DATA, "V_dim=0", "tail_feature_filter=0", "max_num_epochs=30", "l1=1", "l2=1",
               "model_out=" + model).stderr
    assert "nan" not in log.lower()
    assert len(re.findall(r"Epoch \d+:", log)) == 1 and "Epoch 0:" in log
    m = re.search(r"pseudo-gradient is zero: objv = (\S+),", log)
    # 100 log 2 as a float32 printed with eight digits: within two float32 ulps at 64 .. 128 (2 x 2^-17)
    assert m and abs(float(m.group(1)) - 69.314718) <= 2 * 2.0 ** -17, log[-2000:]
    assert " - alpha = " not in log and "Training is done" in log
    _, w, _, _ = _model(model)
    assert not w.any()                               # the file drops entries with w == 0 and no V: it may be empty


@pytest.mark.gpu
def test_fm_with_mixed_lens(built, tmp_path):
    args = ["learner=lbfgs", "data_in=" + DATA, "V_dim=5", "V_threshold=2", "tail_feature_filter=0", "max_num_epochs=10"]
    m0, m1 = str(tmp_path / "m0"), str(tmp_path / "m1")
    _cli(built, *args, "model_out=" + m0)
    log = _cli(built, *args, "l1=.05", "model_out=" + m1).stderr
    f0, acc = _accepted(log)
    seq = [f0] + acc
    assert len(acc) >= 2 and all(b <= a for a, b in zip(seq, seq[1:])), seq
    _, w0, has0, _ = _model(m0, 5)
    _, w1, has1, V1 = _model(m1, 5)
    assert 0 < has0.sum() < len(has0) and has1.any(), "mixed lens (the file drops entries with w == 0 and no V)"
    assert 0 < np.count_nonzero(w1) < np.count_nonzero(w0), (np.count_nonzero(w1), np.count_nonzero(w0))
    alive = has1 & (w1 != 0)
    assert alive.any() and V1[alive].all(axis=None), "V of the surviving keys is non-zero"
    assert np.isfinite(V1).all() and V1[has1 & (w1 == 0)].any(), "l1 does not touch V"


def test_negative_l1_is_refused(built):
    r = _cli(built, "learner=lbfgs", "data_in=" + DATA, "V_dim=0", "l1=-1", ok=False)
    assert r.returncode != 0 and "l1" in r.stderr and "Training is done" not in r.stderr
