"""pairs_out of task = dump (host/model_dump.h): a second file, one line "<id>\\t<id_1>:<s_1>\\t ..." per entry with V.  No GPU:
what Init refuses before the device is touched.  GPU: a trained model's lists against float64 with V read back from the
dump_out text of the same run (%.9g round-trips a float: the dump is its own reference), the same bytes for two unit sizes,
and dump_out byte for byte what it is without pairs_out."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dump_pairs import check_lists   # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _difacto(built, *args):
    return subprocess.run([os.path.join(built, "difacto")] + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("arg,words", [("pairs_topk=0", ("pairs_topk=0", "1 to 32 partners")), ("pairs_topk=33", ("pairs_topk=33", "1 to 32 partners")),
                                       ("pairs_by=other", ("pairs_by=other is not one of abs", "and pos"))])
def test_refused_in_init(built, arg, words):
    r = _difacto(built, "task=dump", "model_in=none", "dump_out=none", "pairs_out=none", arg)
    assert r.returncode != 0 and all(w in r.stderr for w in words), r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("by", ["abs", "pos"])
def test_pairs_of_a_trained_model(built, tmp_path, by):
    model, K = str(tmp_path / "model"), 7
    r = _difacto(built, "data_in=" + DATA, "model_out=" + model, "V_dim=4", "batch_size=10", "max_num_epochs=3", "num_jobs_per_epoch=2",
                 "V_threshold=0", "l1=0", "lr=.05", "stop_rel_objv=0", "stop_val_auc=-1e30")
    assert r.returncode == 0, r.stderr[-3000:]
    files = {}
    for name, extra in (("plain", []), ("a", ["pairs_out=" + str(tmp_path / "a.pairs")]), ("b", ["pairs_out=" + str(tmp_path / "b.pairs"), "dump_unit_rows=37"])):
        r = _difacto(built, "task=dump", "model_in=" + model, "dump_out=" + str(tmp_path / name), "pairs_topk=%d" % K, "pairs_by=" + by, *extra)
        assert r.returncode == 0 and "not finite" not in r.stderr, r.stderr[-3000:]
        files[name] = open(tmp_path / name, "rb").read()
    assert files["plain"] == files["a"] == files["b"]
    text = open(tmp_path / "a.pairs", "rb").read()
    assert text == open(tmp_path / "b.pairs", "rb").read() and not os.path.exists(str(tmp_path / "a.pairs") + ".tmp")
    # the model, from the dump of the same run
    rows = [l.split(b"\t") for l in files["a"].split(b"\n")[:-1]]
    ids = np.array([int(t[0]) for t in rows], np.uint64)
    has = np.array([len(t) == 6 for t in rows], np.int32)
    V = np.array([[float(x) for x in t[2:]] if len(t) == 6 else [0.0] * 4 for t in rows], np.float64).astype(np.float32)
    assert has.sum() > 50
    lines = [l.split(b"\t") for l in text.split(b"\n")[:-1]]
    assert [int(t[0]) for t in lines] == [int(i) for i in ids[has == 1]], "one line per entry with V, in the dump's order"
    got = dict(ids=np.zeros((len(ids), K), np.uint64), scores=np.zeros((len(ids), K), np.float32), n=np.zeros(len(ids), np.uint32))
    for e, t in zip(np.flatnonzero(has), lines):
        got["n"][e] = len(t) - 1
        got["ids"][e, :len(t) - 1] = [int(p.split(b":")[0]) for p in t[1:]]
        got["scores"][e, :len(t) - 1] = [float(p.split(b":")[1]) for p in t[1:]]
    assert check_lists(ids, has, V, got, 0, K, by == "pos") == has.sum()
