"""learner = bcd end to end: the reference's BCDLearner tests (tests/cpp/bcd_learner_test.cc) through
Learner::Create("bcd") (build/difacto_bcd_tests), chunking against the numpy restatement (tests/bcd_ref.py), the command
line, the refusals and model_out."""
import os
import re
import subprocess

import numpy as np
import pytest

import bcd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def test_bcd_binaries_build(built):
    assert os.path.exists(os.path.join(built, "difacto_bcd_tests"))


def test_sharded_store_is_refused(built):
    env = dict(os.environ, DMLC_NUM_WORKER="2")
    r = subprocess.run([os.path.join(built, "difacto"), "learner=bcd", "data_in=" + DATA], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode != 0 and "learner = bcd runs in one process on one GPU" in r.stderr


def test_predict_task_points_to_sgd(built):
    r = subprocess.run([os.path.join(built, "difacto"), "task=predict", "learner=bcd", "data_in=" + DATA],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "task=predict learner=sgd model_in=" in r.stderr


def _run_tests_binary(built, chunk=None):
    args = [os.path.join(built, "difacto_bcd_tests"), DATA] + ([str(chunk)] if chunk else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    objv, chunks = {}, {}
    for case, ep, v in re.findall(r"^(\S+) epoch (\d+) objv (\S+)$", r.stdout, re.M):
        objv.setdefault(case, []).append(float(v))
    for case, rows in re.findall(r"^(\S+) chunks ([\d ]+)$", r.stdout, re.M):
        chunks[case] = [int(x) for x in rows.split()]
    return r, objv, chunks


@pytest.mark.gpu
def test_reference_tests_through_the_learner(built):
    """DiagNewton within 1e-5 per epoch, Convergence for ratios .4, 1 and 10 within 1e-3 of 15.884923"""
    r, objv, chunks = _run_tests_binary(built)
    assert sorted(objv) == ["Convergence_.4", "Convergence_1", "Convergence_10", "DiagNewton"]
    assert len(objv["DiagNewton"]) == 10 and all(len(objv["Convergence_" + k]) == 50 for k in (".4", "1", "10"))
    assert chunks["DiagNewton"] == [100]
    assert "partitioning feature into 1 blocks" in r.stderr and "partitioning feature into 881 blocks" in r.stderr


@pytest.mark.gpu
def test_chunked_trajectories_follow_the_restatement(built):
    """the data in >= 4 chunks: every epoch of the four cases against the restatement on the same chunks (statistics,
    partition and the shuffle stream included)"""
    _, objv, chunks = _run_tests_binary(built, 40000)
    rows = chunks["DiagNewton"]
    assert len(rows) >= 4 and sum(rows) == 100, rows
    d = R.read_libsvm(DATA)
    parts = R.split_rows(*d, rows)
    stream = R.RefRand()
    want = R.BCD(parts, l1=.1, lr=.05, block_ratio=.001, tail_feature_filter=0).run(10, stream)
    assert np.allclose(objv["DiagNewton"], want, rtol=1e-5, atol=0)
    for ratio, name in ((.4, "Convergence_.4"), (1, "Convergence_1"), (10, "Convergence_10")):
        want = R.BCD(parts, l1=.1, lr=.8, block_ratio=ratio, tail_feature_filter=0).run(50, stream)
        assert np.allclose(objv[name], want, rtol=1e-4, atol=0), name
        assert abs(objv[name][-1] - 15.884923) / objv[name][-1] < 1e-3


def _cli(built, *args, timeout=600):
    r = subprocess.run([os.path.join(built, "difacto")] + list(args), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.mark.gpu
def test_cli_example_conf(built):
    log = _cli(built, "argfile=" + os.path.join(ROOT, "example", "rcv1_bcd.conf"))
    assert "Unrecognized" not in log
    epochs = re.findall(r"epoch: (\d+), objv: \S+, auc: \S+, acc: \S+", log)
    assert [int(e) for e in epochs] == list(range(10))
    assert "loaded 100 examples" in log and "partitioning feature into 89 blocks" in log


@pytest.mark.gpu
def test_model_out_scores_with_sgd_predict(built, tmp_path):
    """the saved w scored by task=predict learner=sgd against the learner's own final predictions"""
    from difacto_amd import capi
    model, pred = str(tmp_path / "m"), str(tmp_path / "p")
    args = dict(l1=.1, lr=.8, block_ratio=1, tail_feature_filter=0)
    _cli(built, "learner=bcd", "data_in=" + DATA, "max_num_epochs=5", "model_out=" + model,
         *["%s=%s" % kv for kv in args.items()])
    r = subprocess.run([os.path.join(built, "difacto"), "task=predict", "learner=sgd", "data_in=" + DATA, "V_dim=0",
                        "batch_size=100", "model_in=" + model, "pred_out=" + pred], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.loadtxt(pred, dtype=np.float64)
    # the same run through the C ABI: the learner's final predictions
    d = R.read_libsvm(DATA)
    ranges = R.partition_feature(0, R.block_counts(R.fea_group_stats([(d[0], d[1])], 0), 1))
    ctx = capi.Context(0)
    o = capi.Bcd(ctx)
    try:
        o.add_chunk(*d)
        o.build(ranges, tail_feature_filter=0, l1=.1, lr=.8)
        order, stream = list(range(len(ranges))), R.RefRand()
        for _ in range(5):
            stream.shuffle(order)
            o.epoch(order)
        want = o.get_pred(0).astype(np.float64)
        assert np.count_nonzero(o.get_model()["w"]) > 10
    finally:
        o.close()
        ctx.close()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
