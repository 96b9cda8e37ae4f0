"""recommend_out of task = predict (host/sgd_learner.cc over csrc/dfh_recommend.hip): one line per data row, "<item>:<logit>"
joined by tabs, equal to capi.Recommend on the same model file, catalogue and rows (which tests/test_recommend.py holds against
float64); pred_out keeps its bytes with and without the keys under both pred_write values; what is refused."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
K, KDIM, M = 10, 4, 37
COMMON = ["data_in=" + DATA, "V_dim=%d" % KDIM, "batch_size=10", "num_jobs_per_epoch=2", "V_threshold=0", "l1=0"]


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build", "difacto")


def run(built, *args, env=None):
    return subprocess.run([built] + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)


def libsvm(path):
    """-> offset, ids, x"""
    rows = [[t.split(":") for t in line.split()[1:]] for line in open(path)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return off, np.array([int(i) for r in rows for i, _ in r], np.uint64), np.array([np.float32(x) for r in rows for _, x in r], np.float32)


def test_recommend_out_of_a_trained_model(built, tmp_path):
    model, items = str(tmp_path / "model"), str(tmp_path / "items.libsvm")
    r = run(built, "model_out=" + model, "max_num_epochs=3", "lr=.05", "stop_rel_objv=0", "stop_val_auc=-1e30", *COMMON)
    assert r.returncode == 0, r.stderr[-3000:]
    _, ids, _ = libsvm(DATA)
    rng, pool = np.random.default_rng(3), np.unique(ids)
    with open(items, "w") as f:   # M items of 0 .. 5 of the data's ids with dyadic values; item 5 repeats item 4
        lines = ["1 " + " ".join("%d:%g" % (i, x) for i, x in zip(np.sort(rng.choice(pool, n, replace=False)), rng.integers(1, 9, n) / 4))
                 for n in rng.integers(0, 6, M)]
        lines[5] = lines[4]
        f.write("\n".join(lines) + "\n")
    pred, rec = {}, {}
    for write in ("host", "device"):
        for with_key in (0, 1):
            p, x = str(tmp_path / ("pred_%s_%d" % (write, with_key))), str(tmp_path / ("rec_" + write))
            r = run(built, "task=predict", "model_in=" + model, "pred_out=" + p, "pred_write=" + write, "pred_unit_rows=25",
                    *(["items_in=" + items, "recommend_out=" + x, "recommend_topk=%d" % K] if with_key else []), *COMMON)
            assert r.returncode == 0, r.stderr[-3000:]
            pred[write, with_key] = open(p, "rb").read()
        rec[write] = open(x).read()
    assert len(set(pred.values())) == 1 and pred["host", 0].count(b"\n") == 100 and rec["host"] == rec["device"]
    lines = rec["host"].split("\n")[:-1]
    assert len(lines) == 100
    # the same through the C ABI: the model file in a table, the catalogue as one batch, the data as one batch
    from difacto_amd import capi
    ctx = capi.Context(0)
    tb = capi.Table(ctx, 1 << 16, V_dim=KDIM, V_threshold=0, l1=0.0)
    assert tb.load(model)[0] > 0
    want, b = capi.Recommend(ctx, K), capi.Batch(ctx, 128, 1 << 14)
    for path, call in ((items, want.add_items), (DATA, want.append_batch)):
        off, fid, x = libsvm(path)
        b.load_host(off, fid, x, np.ones(len(off) - 1, np.float32))
        b.localize()
        b.lookup(tb)
        b.sgd_step(tb, is_train=False)
        call(b, tb)
    got = want.read()
    assert want.item_count() == M and got["nonfinite"] == 0
    for q, line in enumerate(lines):
        tok = [t.split(":") for t in line.split("\t")]
        assert len(tok) == got["n"][q] == K
        assert [int(i) for i, _ in tok] == list(got["items"][q]) and [np.float32(v) for _, v in tok] == list(got["logits"][q]), q
    for o in (want, b, tb, ctx):
        o.close()


PRED = ["task=predict", "model_in=none", "pred_out=none"]


@pytest.mark.parametrize("args,env,words", [
    (["task=train", "recommend_out=x", "items_in=y"], {}, ["with task=train", "use task=predict"]),
    (PRED + ["recommend_out=x", "items_in=y"], {"DMLC_ROLE": "worker", "DMLC_NUM_WORKER": "2", "DIFACTO_RANK": "0"},
     ["recommend_out with a sharded store", "run one process"]),
    (PRED + ["recommend_out=x", "items_in=y", "device_path=literal"], {}, ["recommend_out with device_path=literal"]),
    (PRED + ["recommend_out=x", "items_in=y", "learner=lbfgs"], {}, ["with learner=lbfgs", "only learner=sgd"]),
    (PRED + ["recommend_out=x", "items_in=y", "recommend_topk=33"], {}, ["recommend_topk=33", "between 1 and 32"]),
    (PRED + ["recommend_out=x", "items_in=y", "recommend_topk=0"], {}, ["recommend_topk=0", "between 1 and 32"]),
    (PRED + ["recommend_out=x"], {}, ["recommend_out without items_in"]),
    (PRED + ["items_in=y"], {}, ["items_in without recommend_out"]),
])
def test_refused_before_the_device_is_touched(built, tmp_path, args, env, words):
    env = dict(os.environ, DIFACTO_COMM="file", DIFACTO_RENDEZVOUS=str(tmp_path), DIFACTO_DEVICE="0", **env) if env else None
    r = run(built, *args, *COMMON, env=env)
    assert r.returncode != 0 and all(w in r.stderr for w in words), r.stderr[-2000:]
