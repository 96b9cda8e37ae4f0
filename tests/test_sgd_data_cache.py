"""data_cache = hbm of learner = sgd: the parsed rows of every data part stay in HBM after the epoch that read them.

No GPU: the key's values and the combinations Init refuses.  GPU: the command line with and without the cache (same
Training / Validation lines, same model, later epochs served from the cache), build/difacto_sgd_cache_tests (epochs whose
file is gone), and dfh_batch_prepare_cached against dfh_batch_prepare_rows through the C ABI."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
EPOCHS = 3


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _difacto(built, *args, env=None, timeout=600, data=DATA):
    return subprocess.run([os.path.join(built, "difacto"), "data_in=" + data, "batch_size=25", "V_dim=4"] + list(args),
                          capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


def test_binaries_build(built):
    assert os.path.exists(os.path.join(built, "difacto_sgd_cache_tests"))


def test_unknown_cache_value_is_fatal(built):
    r = _difacto(built, "data_cache=disk")
    assert r.returncode != 0 and "data_cache=disk" in r.stderr and "hbm" in r.stderr and "off" in r.stderr, r.stderr[-2000:]


def test_literal_path_is_refused(built):
    r = _difacto(built, "data_cache=hbm", "device_path=literal")
    assert r.returncode != 0 and "data_cache=hbm with device_path=literal" in r.stderr, r.stderr[-2000:]


def test_predict_is_refused(built):
    r = _difacto(built, "data_cache=hbm", "task=predict", "model_in=/nonexistent", "pred_out=/dev/null")
    assert r.returncode != 0 and "data_cache=hbm with task=predict" in r.stderr, r.stderr[-2000:]


def test_sharded_store_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = _difacto(built, "data_cache=hbm", env=env)
    assert r.returncode != 0 and "data_cache=hbm with a sharded store" in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def _criteo_file(path, rows=300, seed=7):
    """criteo text: label, 13 integer fields, 26 fields of 8 hex characters; some fields empty"""
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for _ in range(rows):
            ints = ["" if rng.random() < 0.2 else str(int(rng.integers(0, 50))) for _ in range(13)]
            cats = ["" if rng.random() < 0.15 else "%08x" % int(rng.integers(0, 40)) for _ in range(26)]
            f.write("\t".join([str(int(rng.random() < 0.3))] + ints + cats) + "\n")
    return path


def _train(built, tmp_path, tag, extra, cache, data=DATA):
    model = str(tmp_path / ("model_" + tag))
    args = ["max_num_epochs=%d" % EPOCHS, "num_jobs_per_epoch=2", "V_threshold=2", "l1=.1", "lr=.1", "stop_rel_objv=0",
            "stop_val_auc=-1e30", "model_out=" + model] + list(extra) + list(cache)
    r = _difacto(built, *args, data=data)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = re.findall(r" - (Training: .*|Validation: .*)$", r.stderr, re.M)
    return r.stderr, lines, model


def _model(path):
    from difacto_amd import capi
    ctx = capi.Context(0)
    tb = capi.Table(ctx, 1 << 14, V_dim=4)
    tb.load(path)
    e = tb.export()
    o = np.argsort(e["keys"])
    out = {k: np.array(e[k][o]) for k in ("keys", "scal", "has_V", "V")}
    tb.close()
    ctx.close()
    return out


def _same_model(a, b):
    for k in ("keys", "scal", "has_V", "V"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


CONFIGS = {
    "shuffle": ["shuffle=2"],
    "neg_sampling": ["shuffle=2", "neg_sampling=0.5"],
    "in_order": ["shuffle=0"],
    "validation": ["shuffle=2", "data_val=" + DATA],
}


def _check_cached_run(built, tmp_path, extra, jobs_per_epoch, data=DATA):
    plain_log, plain, m0 = _train(built, tmp_path, "plain", extra, [], data)
    log, cached, m1 = _train(built, tmp_path, "cached", extra, ["data_cache=hbm"], data)
    assert len(plain) == EPOCHS * (jobs_per_epoch // 2) and plain == cached, "\n".join(plain + ["--"] + cached)
    assert "HBM cache" not in plain_log and "cached" not in plain_log
    _same_model(_model(m0), _model(m1))
    # epoch 0 parses and keeps, every later job is served from the cache
    assert len(re.findall(r"rows parsed from \S+, cached \d+ MB", log)) == jobs_per_epoch, log[-3000:]
    assert len(re.findall(r"rows from the HBM cache", log)) == jobs_per_epoch * (EPOCHS - 1), log[-3000:]
    assert "WARNING" not in log or "does not fit" not in log
    return log


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cli_results_do_not_depend_on_the_cache(built, tmp_path, name):
    """Training / Validation lines string for string, model_out bit for bit, later epochs from the cache"""
    extra = CONFIGS[name]
    _check_cached_run(built, tmp_path, extra, 4 if name == "validation" else 2)


@pytest.mark.gpu
def test_cli_criteo_text(built, tmp_path):
    data = _criteo_file(str(tmp_path / "criteo.txt"))
    log = _check_cached_run(built, tmp_path, ["shuffle=2", "data_format=criteo"], 2, data)
    assert data in log


@pytest.mark.gpu
def test_cli_budget_too_small_streams_every_epoch(built, tmp_path):
    """data_cache_max_gb below one buffer's size: same results, one warning per part, nothing served from the cache"""
    extra = ["shuffle=2"]
    _, plain, m0 = _train(built, tmp_path, "plain", extra, [])
    log, cached, m1 = _train(built, tmp_path, "tight", extra, ["data_cache=hbm", "data_cache_max_gb=1e-6"])
    assert len(plain) == EPOCHS and plain == cached
    _same_model(_model(m0), _model(m1))
    warnings = re.findall(r"part (\d) of 2 \(training\): does not fit the HBM cache: its \d+ rows need (\d+) bytes", log)
    assert sorted(w[0] for w in warnings) == ["0", "1"] and all(int(w[1]) > 1073 for w in warnings), log[-3000:]
    assert "from the HBM cache" not in log
    assert len(re.findall(r"not cached", log)) == 2 * EPOCHS


@pytest.mark.gpu
def test_epochs_run_without_their_file(built):
    """build/difacto_sgd_cache_tests: the data file is unlinked after epoch 0; epochs 1 and 2 complete with the uncached
    run's losses"""
    r = subprocess.run([os.path.join(built, "difacto_sgd_cache_tests"), DATA], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    for case in ("Shuffled", "Sampled", "InOrder", "Validated"):
        assert case + " ok (3 uncached, 3 cached epochs)" in r.stdout, r.stdout[-3000:]
        assert len(re.findall(r"^%s cached epoch \d loss" % case, r.stdout, re.M)) == 3


# ---------------------------------------------------------------------------------------------------------------------
# dfh_batch_prepare_cached against dfh_batch_prepare_rows (a subprocess of its own, under its own time limit)
# ---------------------------------------------------------------------------------------------------------------------
KERNEL_SCRIPT = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %(root)r)
    from difacto_amd import capi

    def random_batch(rng, nrows, nfeat_space, max_nnz_row, binary=False):
        """a ragged random CSR batch with raw u64 ids, empty rows among them"""
        lens = rng.integers(0, max_nnz_row + 1, size=nrows)
        off = np.zeros(nrows + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        nnz = int(off[-1])
        idx = rng.integers(0, nfeat_space, size=nnz, dtype=np.uint64)
        val = None if binary else rng.normal(size=nnz).astype(np.float32)
        lab = np.where(rng.random(nrows) < 0.4, 1.0, -1.0).astype(np.float32)
        return dict(offset=off, index=idx, value=val, label=lab)

    def minibatch(bufs_host, segments):
        off, lab = [0], []
        for g, rows in segments:
            hb = bufs_host[g]
            for r in rows:
                off.append(off[-1] + int(hb["offset"][r + 1]) - int(hb["offset"][r]))
                lab.append(hb["label"][r])
        return np.array(off, np.uint64), np.array(lab, np.float32)

    def run(case, bufs_host, plans, max_rows, max_nnz):
        ctx = capi.Context(0)
        ctx.set_pipeline(1)
        kw = dict(l1=0.02, l2=0.01, lr=0.3, V_lr=0.05, V_l2=0.02, V_threshold=0, V_init_scale=0.2, seed=5)
        rbs = []
        for hb in bufs_host:
            rb = capi.RowBuf(ctx, len(hb["label"]), max(int(hb["offset"][-1]), 1))
            rb.load_host(hb["offset"], hb["index"], hb["value"])
            rb.set_labels(hb["label"])
            rbs.append(rb)
        results = []
        for cached in (False, True):
            tb = capi.Table(ctx, 1 << 20, V_dim=8, init_mode=capi.INIT_HASH, **kw)
            bt = capi.Batch(ctx, max_rows, max_nnz)
            out = []
            for step, segments in enumerate(plans * 2):   # (the second round: stored splitters, the count pass gathers)
                segs = [(rbs[g], rows) for g, rows in segments]
                off, lab = minibatch(bufs_host, segments)
                if cached:
                    bt.prepare_cached(tb, segs)
                else:
                    bt.prepare_rows(tb, off, lab, segs)
                d_off, d_lab = bt.get_rows()
                assert np.array_equal(d_off, off.astype(np.uint32)) and d_lab.tobytes() == lab.tobytes(), (case, cached, step)
                loc = bt.get_localized()
                bt.sgd_step(tb, is_train=True, push_cnt=step < len(plans))
                out.append((d_off, d_lab, loc["feaids"], loc["index"], loc["feacnt"], bt.pred()))
            e = tb.export()
            o = np.argsort(e["keys"])
            results.append((out, [np.array(e[k][o]) for k in ("keys", "scal", "has_V", "V")]))
            bt.close()
            tb.close()
        (a, ma), (b, mb) = results
        for step, (x, y) in enumerate(zip(a, b)):
            for u, v in zip(x, y):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), (case, step)
        for u, v in zip(ma, mb):
            assert u.tobytes() == v.tobytes(), case
        for rb in rbs:
            rb.close()
        ctx.close()
        print(case, "ok:", len(a), "minibatches identical")

    rng = np.random.default_rng(43)
    if sys.argv[1] == "small":
        # with values, without, with again; empty rows; one and two buffers per minibatch; repeated rows; a single row;
        # a buffer read through in order; more rows than one block of the describing kernel (256)
        bufs = [random_batch(rng, 900, 700, 30), random_batch(rng, 500, 700, 12, binary=True), random_batch(rng, 300, 700, 40)]
        plans = [[(0, rng.permutation(900)[:200])], [(0, rng.permutation(900)[:120]), (2, rng.permutation(300)[:90])],
                 [(1, rng.permutation(500)[:150])], [(1, rng.permutation(500)[:60]), (0, np.array([5, 5, 7, 5]))],
                 [(2, np.arange(300))], [(0, np.array([17]))], [(0, rng.permutation(900)[:257]), (1, rng.permutation(500)[:143])],
                 [(1, rng.permutation(500)[:400])]]
        run("small", bufs, plans, 400, 400 * 40)
    else:
        # C3 size: 10 000 rows x 39 ids out of two 100 000-row buffers
        bufs = []
        for _ in range(2):
            n = 100000
            b = dict(offset=(np.arange(n + 1) * 39).astype(np.uint64), index=rng.integers(0, 300000, size=n * 39, dtype=np.uint64) << np.uint64(12),
                     value=None, label=np.where(rng.random(n) < 0.25, 1.0, 0.0).astype(np.float32))
            bufs.append(b)
        plans = [[(0, rng.permutation(100000)[:10000])], [(0, rng.permutation(100000)[:6000]), (1, rng.permutation(100000)[:4000])],
                 [(1, rng.permutation(100000)[:10000])]]
        run("c3", bufs, plans, 10000, 10000 * 48)
''')


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["small", "c3"])
def test_prepare_cached_matches_prepare_rows(built, tmp_path, size):
    """the same minibatches prepared from the host's offsets and labels and from the row numbers alone: the device's offsets
    and labels, get_localized(), the step's predictions and the model after the steps, bit for bit"""
    script = tmp_path / "prepare_cached.py"
    script.write_text(KERNEL_SCRIPT % dict(root=ROOT))
    r = subprocess.run([sys.executable, str(script), size], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and size + " ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
