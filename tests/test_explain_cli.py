"""explain_out of task = predict (host/sgd_learner.cc over csrc/dfh_explain.hip): one line per data row, "<inter>" and
"\\t<id_i>:<id_j>:<c>" per pair, against float64 from task = dump of the same model and the libsvm file, with the bound of
test_explain.py; pred_out keeps its bytes with and without the key under both pred_write values; what Init refuses."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
K, KDIM = 10, 4
COMMON = ["data_in=" + DATA, "V_dim=%d" % KDIM, "batch_size=10", "num_jobs_per_epoch=2", "V_threshold=0", "l1=0"]


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build", "difacto")


def run(built, *args, env=None):
    return subprocess.run([built] + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)


@pytest.fixture(scope="module")
def model(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("explain_cli")
    path, dump = str(d / "model"), str(d / "dump.txt")
    r = run(built, "model_out=" + path, "max_num_epochs=3", "lr=.05", "stop_rel_objv=0", "stop_val_auc=-1e30", *COMMON)
    assert r.returncode == 0, r.stderr[-3000:]
    r = run(built, "task=dump", "model_in=" + path, "dump_out=" + dump)
    assert r.returncode == 0, r.stderr[-3000:]
    tok = [line.split("\t") for line in open(dump)]
    return path, {int(t[0]): np.array(t[2:], np.float64) for t in tok if len(t) > 2}   # printed id -> V, the entries that have it


def test_explain_out_of_a_trained_model(built, model, tmp_path):
    path, V = model
    pred, expl = {}, {}
    for write in ("host", "device"):
        for with_key in (0, 1):
            p, x = str(tmp_path / ("pred_%s_%d" % (write, with_key))), str(tmp_path / ("expl_" + write))
            r = run(built, "task=predict", "model_in=" + path, "pred_out=" + p, "pred_write=" + write, "pred_unit_rows=25",
                    *(["explain_out=" + x, "explain_topk=%d" % K] if with_key else []), *COMMON)
            assert r.returncode == 0, r.stderr[-3000:]
            pred[write, with_key] = open(p, "rb").read()
        expl[write] = open(x).read()
    assert len(set(pred.values())) == 1 and pred["host", 0].count(b"\n") == 100 and expl["host"] == expl["device"]
    lines, rows = expl["host"].split("\n")[:-1], [row.split() for row in open(DATA)]
    assert len(lines) == len(rows) == 100
    m, g = KDIM + 3, lambda n: n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    for line, row in zip(lines, rows):
        feats = [t.split(":") for t in row[1:] if int(t.split(":")[0]) in V]
        ids, xs = [int(i) for i, _ in feats], np.array([np.float32(x) for _, x in feats], np.float64)
        Vr = np.array([V[i] for i in ids]).reshape(len(ids), KDIM)
        assert len(set(ids)) == len(ids)
        C, B = np.outer(xs, xs) * (Vr @ Vr.T), np.outer(np.abs(xs), np.abs(xs)) * (np.abs(Vr) @ np.abs(Vr).T)
        i, j = np.triu_indices(len(ids), 1)
        c64, mag, tok = C[i, j], B[i, j], line.split("\t")
        got = [t.split(":") for t in tok[1:]]
        assert len(got) == min(K, c64.size)
        at = {(ids[a], ids[b]): t for t, (a, b) in enumerate(zip(i, j))}
        t = np.array([at[int(a), int(b)] for a, b, _ in got], np.int64)
        c = np.array([float(v) for _, _, v in got], np.float64)
        assert np.unique(t).size == t.size and (np.abs(c - c64[t]) <= g(m) * mag[t]).all()
        assert (np.diff(np.abs(c)) <= 0).all()
        rest = np.setdiff1d(np.arange(c64.size), t)
        if rest.size:
            assert (np.abs(c64[rest]) <= np.abs(c[-1]) + g(m) * mag[rest]).all()
        assert abs(float(tok[0]) - c64.sum()) <= g(c64.size + m) * mag.sum() and c64.size > K


@pytest.mark.parametrize("args,env,words", [
    (["task=train", "explain_out=x"], {}, ["explain_out with task=train", "use task=predict"]),
    (["task=predict", "model_in=none", "pred_out=none", "explain_out=x"], {"DMLC_ROLE": "worker", "DMLC_NUM_WORKER": "2", "DIFACTO_RANK": "0"},
     ["explain_out with a sharded store", "run one process"]),
    (["task=predict", "model_in=none", "pred_out=none", "explain_out=x", "device_path=literal"], {}, ["explain_out with device_path=literal"]),
    (["task=predict", "model_in=none", "pred_out=none", "explain_out=x", "learner=lbfgs"], {}, ["explain_out with learner=lbfgs", "only learner=sgd"]),
    (["task=predict", "model_in=none", "pred_out=none", "explain_out=x", "V_dim=0"], {}, ["explain_out with V_dim=0", "no interaction pairs"]),
])
def test_refused_before_the_device_is_touched(built, tmp_path, args, env, words):
    env = dict(os.environ, DIFACTO_COMM="file", DIFACTO_RENDEZVOUS=str(tmp_path), DIFACTO_DEVICE="0", **env) if env else None
    extra = [a for a in COMMON if not (a.startswith("V_dim") and any(x.startswith("V_dim") for x in args))]
    r = run(built, *args, *extra, env=env)
    assert r.returncode != 0 and all(w in r.stderr for w in words), r.stderr[-2000:]
