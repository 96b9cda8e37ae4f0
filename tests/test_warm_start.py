"""model_in for learner = bcd and learner = lbfgs (dfh_bcd_set_model, dfh_lbfgs_set_model: a model given by key joined onto
the learner's own key order on the device, BCD's predictions rebuilt from w) and task = predict with those learners."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bcd_ref as R  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
f32 = np.float32
MIXED = ["V_dim=4", "V_threshold=2", "tail_feature_filter=2"]
BCD_ARGS = ["l1=.1", "lr=.8", "block_ratio=1", "tail_feature_filter=0"]   # test_bcd_learner.py's Convergence_1 case


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def ctx():
    from difacto_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ BCD, the C ABI
# keys in ReverseBytes space (raw id = reverse_bytes(key)); four blocks: [1, 120) ordinary keys, [120, 200) no key at all,
# [200, 330) with key 200 in every row of every chunk, [330, 400) ordinary keys
RANGES = [(1, 120), (120, 200), (200, 330), (330, 400)]
RARE = [5, 17, 118, 210, 329, 340]       # in one or two training rows: filtered by tail_feature_filter = 2
VAL_ONLY = [60, 390]                     # in the validation chunk only: never in the model
L1, LR, TAIL = .1, .8, 2


def _chunk(rng, nrows, binary, rare=(), extra=()):
    pool = np.array([k for k in list(range(1, 120)) + list(range(201, 330)) + list(range(330, 400))
                     if k not in RARE and k not in VAL_ONLY])
    rows = []
    for r in range(nrows):
        ks = [200] + list(rng.choice(pool, 11, replace=False))
        for k, where in rare:
            if r in where:
                ks.append(k)
        for k in extra:
            if r % 7 == 3:
                ks.append(k)
        rows.append(rng.permutation(ks))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    keys = np.concatenate(rows).astype(np.uint64)
    val = None if binary else rng.normal(size=len(keys)).astype(np.float32)
    lab = (rng.random(nrows) < .4).astype(np.float32)
    return off, R.reverse_bytes_np(keys), val, lab


@pytest.fixture(scope="module")
def job():
    """two training chunks (193 rows with values, 64 without) and a validation chunk of 50 rows; the input model; the
    expected w and the float32 restatement of the predictions, computed once"""
    rng = np.random.default_rng(7)
    train = [_chunk(rng, 193, False, rare=[(5, (3,)), (17, (8, 100)), (210, (0, 192)), (340, (77,))]),
             _chunk(rng, 64, True, rare=[(118, (63,)), (329, (0, 1))])]
    val = [_chunk(rng, 50, False, rare=[(5, (2,))], extra=VAL_ONLY)]
    ref = R.bcd_with_ranges(train, val, RANGES, l1=L1, lr=LR, tail_feature_filter=TAIL)
    mk = ref.keys.astype(np.int64)
    assert 280 <= len(mk) <= 320 and not set(RARE) & set(mk) and not set(VAL_ONLY) & set(mk) and 200 in mk
    assert [pe - pb > 0 for pb, pe in ref.pos] == [True, False, True, True]
    # the input: ~70 % of the model's keys, the filtered keys, keys never seen; w positive, negative, 0 and -0
    take = mk[rng.random(len(mk)) < .7]
    take = np.union1d(take, [200])
    never = np.array([130, 150, 199, 1000, 2 ** 40 + 3], np.int64)
    in_keys = np.concatenate([take, RARE, VAL_ONLY, never]).astype(np.uint64)
    in_w = rng.normal(size=len(in_keys)).astype(np.float32)
    in_w[rng.random(len(in_w)) < .15] = 0
    in_w[1] = f32(-0.0)
    o = rng.permutation(len(in_keys))
    in_keys, in_w = in_keys[o], in_w[o]
    want_w = np.zeros(len(mk), np.float32)
    pos = np.searchsorted(ref.keys, in_keys)
    hit = (pos < len(mk)) & (ref.keys[np.minimum(pos, len(mk) - 1)] == in_keys)
    want_w[pos[hit]] = in_w[hit]
    assert hit.sum() == len(take) and (want_w > 0).any() and (want_w < 0).any() and (want_w[np.searchsorted(mk, take)] == 0).any()
    return dict(train=train, val=val, ref=ref, in_keys=in_keys, in_w=in_w, want_w=want_w, matched=int(hit.sum()),
                want_pred=[_restate_pred(ref, c, want_w) for c in ref.tr + list(ref.va)])


def _restate_pred(ref, c, w):
    """the definition in include/difacto_hip.h: per row a sequential float32 sum over the surviving entries whose key lies
    in a block, in ascending model position, entries with w == 0 skipped; x = 1 in a chunk without values"""
    in_blk = np.zeros(len(ref.keys), bool)
    for pb, pe in ref.pos:
        in_blk[pb:pe] = True
    out = np.zeros(c.n, np.float32)
    for r in range(c.n):
        e = np.flatnonzero((c.row == r) & (c.gk >= 0))
        e = e[in_blk[c.gk[e]]]
        e = e[np.argsort(c.gk[e], kind="stable")]
        acc = f32(0)
        for i in e:
            wi = w[c.gk[i]]
            if wi == 0:
                continue
            acc = f32(acc + (wi if c.val is None else f32(wi * c.val[i])))
        out[r] = acc
    return out


def _device(ctx, job):
    from difacto_amd import capi
    o = R.make_device(capi, ctx, job["train"], RANGES, l1=L1, lr=LR, tail=TAIL, val=job["val"])
    assert np.array_equal(o.get_model()["keys"], job["ref"].keys)
    return o


@pytest.mark.gpu
def test_bcd_set_model_w_and_predictions(ctx, job):
    o = _device(ctx, job)
    try:
        assert o.set_model(job["in_keys"], job["in_w"]) == job["matched"]
        m = o.get_model()
        assert R.same_bits(m["w"], job["want_w"])
        assert np.all(m["delta"] == 1) and np.all(m["dw"] == 0) and not np.signbit(m["dw"]).any()
        preds = R.device_preds(o, job["ref"])
        assert [len(p) for p in preds] == [193, 64, 50]
        for i, (p, want) in enumerate(zip(preds, job["want_pred"])):
            assert np.count_nonzero(want) > len(want) // 2
            assert R.same_bits(p, want), "chunk %d: %d rows differ" % (i, np.count_nonzero(p != want))
    finally:
        o.close()


@pytest.mark.gpu
def test_bcd_set_model_empty_input_leaves_the_built_state(ctx, job):
    o = _device(ctx, job)
    try:
        before, pb = o.get_model(), R.device_preds(o, job["ref"])
        assert o.set_model(np.zeros(0, np.uint64), np.zeros(0, np.float32)) == 0
        after, pa = o.get_model(), R.device_preds(o, job["ref"])
        for n in ("w", "delta", "dw"):
            assert R.same_bits(before[n], after[n])
        assert all(R.same_bits(a, b) and not a.any() for a, b in zip(pa, pb))
    finally:
        o.close()


@pytest.mark.gpu
def test_bcd_set_model_refusals(ctx, job):
    from difacto_amd import capi
    o = _device(ctx, job)
    try:
        k, w = job["in_keys"], job["in_w"]
        with pytest.raises(capi.DfhError, match="not unique"):
            o.set_model(np.r_[k, k[5:6]], np.r_[w, w[5:6]])
        bad = w.copy()
        bad[3] = np.inf
        with pytest.raises(capi.DfhError, match="non-finite"):
            o.set_model(k, bad)
        o.step(0)
        with pytest.raises(capi.DfhError, match="step has run"):
            o.set_model(k, w)
    finally:
        o.close()
    o = capi.Bcd(ctx)
    try:
        o.add_chunk(*job["train"][0])
        with pytest.raises(capi.DfhError, match="not built"):
            o.set_model(job["in_keys"], job["in_w"])
    finally:
        o.close()


@pytest.mark.gpu
def test_bcd_step_after_set_model(ctx, job):
    """block 0 right after set_model against numpy on the restated predictions: g, h within 1e-6 of the sum of |terms|
    (test_bcd_kernels.py's criterion for a cold step), w, delta w and every chunk's pred afterwards bit for bit"""
    o = _device(ctx, job)
    try:
        o.set_model(job["in_keys"], job["in_w"])
        ref = R.bcd_with_ranges(job["train"], job["val"], RANGES, l1=L1, lr=LR, tail_feature_filter=TAIL)   # this test's own
        chunks = ref.tr + list(ref.va)
        for c, p in zip(chunks, job["want_pred"]):
            c.pred = p.copy()
        ref.w, ref.delta, ref.dw = job["want_w"].copy(), np.ones_like(job["want_w"]), np.zeros_like(job["want_w"])
        g_want, h_want, g_mag, h_mag = ref.grad(0, mag=True)
        g, h, _ = o.step(0, grad=True)
        print("max |g - g_want| / sum|terms| = %.3g, h: %.3g" % (np.max(np.abs(g - g_want) / np.maximum(g_mag, 1e-300)),
                                                                np.max(np.abs(h - h_want) / np.maximum(h_mag, 1e-300))))
        assert np.all(np.abs(g - g_want) <= 1e-6 * g_mag) and np.all(np.abs(h - h_want) <= 1e-6 * h_mag)
        pb, pe = ref.pos[0]
        w, d, dw = R.update_weight(g.astype(np.float32), h.astype(np.float32), ref.w[pb:pe], ref.delta[pb:pe], L1, LR)
        m = o.get_model()
        assert R.same_bits(m["w"][pb:pe], w) and R.same_bits(m["dw"][pb:pe], dw) and R.same_bits(m["delta"][pb:pe], d)
        assert R.same_bits(m["w"][pe:], ref.w[pe:]) and np.count_nonzero(dw) > 10
        ref.w, ref.delta, ref.dw = m["w"].copy(), m["delta"].copy(), m["dw"].copy()
        ref.update_pred(0)
        for i, (c, p) in enumerate(zip(chunks, R.device_preds(o, ref))):
            assert R.same_bits(p, c.pred), "pred of chunk %d (training first) not bit-identical" % i
    finally:
        o.close()


@pytest.mark.gpu
def test_bcd_set_model_is_repeatable(ctx, job):
    a, b = _device(ctx, job), _device(ctx, job)
    try:
        a.set_model(job["in_keys"], job["in_w"])
        b.set_model(job["in_keys"], job["in_w"])
        for p, q in zip(R.device_preds(a, job["ref"]), R.device_preds(b, job["ref"])):
            assert p.tobytes() == q.tobytes()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ the command line
def _difacto(built, *args, env=None):
    return subprocess.run([os.path.join(built, "difacto")] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT,
                          env=env)


def _ok(built, *args):
    r = _difacto(built, *args)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _bcd_objv(log):
    return [float(v) for v in re.findall(r"epoch: \d+, objv: (\S+),", log)]


def _export(ctx, path, k):
    from difacto_amd import capi
    t = capi.Table(ctx, 1 << 16, V_dim=k)
    t.load(path)
    e = t.export()
    t.close()
    return e


@pytest.fixture(scope="module")
def bcd_runs(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("bcd")
    a = _ok(built, "learner=bcd", "data_in=" + DATA, "max_num_epochs=10", "model_out=" + str(d / "a"), *BCD_ARGS)
    b = _ok(built, "learner=bcd", "data_in=" + DATA, "max_num_epochs=1", "model_in=" + str(d / "a"), *BCD_ARGS)
    return dict(dir=d, a=a, b=b, model=str(d / "a"))


@pytest.mark.gpu
def test_bcd_cli_warm_start(built, ctx, bcd_runs):
    oa, ob = _bcd_objv(bcd_runs["a"]), _bcd_objv(bcd_runs["b"])
    assert len(oa) == 10 and len(ob) == 1
    m = re.search(r"model loaded from (\S+): (\d+) of (\d+) keys matched (\d+) model keys", bcd_runs["b"])
    assert m and m.group(1) == bcd_runs["model"] and 0 < int(m.group(2)) <= int(m.group(3)) and int(m.group(2)) <= int(m.group(4))
    assert "model loaded from" not in bcd_runs["a"]
    # the restatement started from A's saved w: its predictions rebuilt block after block, then one epoch on a fresh
    # shuffle stream, as the new process runs it
    e = _export(ctx, bcd_runs["model"], 0)
    ref = R.BCD([R.read_libsvm(DATA)], l1=.1, lr=.8, block_ratio=1, tail_feature_filter=0)
    pos = np.searchsorted(ref.keys, e["keys"])
    assert np.array_equal(ref.keys[pos], e["keys"]) and int(m.group(2)) == len(pos)
    ref.w[pos] = e["scal"][:, 1]
    ref.dw = ref.w.copy()
    for b in range(len(ref.ranges)):
        ref.update_pred(b)
    ref.dw[:] = 0
    want = ref.run(1, R.RefRand())[0] / 100
    print("B epoch 0 objv %r, restatement %r, A epoch 0 %r" % (ob[0], want, oa[0]))
    # rtol 1e-4: test_bcd_learner.py's tolerance for these arguments; + half a unit of the 6 digits the log prints
    assert abs(ob[0] - want) <= 1e-4 * abs(want) + 5e-6 * abs(ob[0])
    assert ob[0] < oa[0]


@pytest.mark.gpu
def test_bcd_cli_missing_model_is_fatal(built, tmp_path):
    missing = str(tmp_path / "no_such_model")
    r = _difacto(built, "learner=bcd", "data_in=" + DATA, "max_num_epochs=1", "model_in=" + missing, *BCD_ARGS)
    assert r.returncode != 0 and missing in r.stderr


def _accepted(log):
    out, last = [], None
    for line in log.splitlines():
        m = re.search(r" - alpha = \S+, objv = (\S+), <p,g> = ", line)
        if m:
            last = float(m.group(1))
        if "wolfe condition is satisifed" in line or "reach the maximal number of linesearch steps" in line:
            out.append(last)
    return out


def _starts(log):
    return [float(v) for v in re.findall(r"start linesearch with objv = (\S+),", log)]


def _lines(log):
    return [l.split("] ", 1)[-1] for l in log.splitlines() if "objv" in l]


@pytest.fixture(scope="module")
def lbfgs_runs(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("lbfgs")
    args = ["learner=lbfgs", "data_in=" + DATA] + MIXED
    a = _ok(built, *args, "max_num_epochs=6", "model_out=" + str(d / "m"))
    b = _ok(built, *args, "max_num_epochs=1", "model_in=" + str(d / "m"))
    return dict(dir=d, a=a, b=b, model=str(d / "m"))


@pytest.mark.gpu
def test_lbfgs_cli_warm_start(lbfgs_runs):
    a, b = lbfgs_runs["a"], lbfgs_runs["b"]
    last, first_a, first_b = _accepted(a)[-1], _starts(a)[0], _starts(b)[0]
    print("A first %r, A last accepted %r, B first %r" % (first_a, last, first_b))
    assert abs(first_b - last) <= 1e-5 * abs(last)
    assert first_b < first_a
    m = re.search(r"model loaded from \S+: (\d+) of (\d+) keys matched (\d+) model keys", b)
    assert m and int(m.group(1)) > 0 and "model loaded from" not in a


def _run_ranks(built, world, args, rv):
    """one process per rank on the one GPU over the file transport (the launcher of tests/test_lbfgs_sharded.py)"""
    os.makedirs(rv)
    procs = []
    for r in range(world):
        env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER=str(world), DIFACTO_RANK=str(r), DIFACTO_DEVICE="0",
                   DIFACTO_COMM="file", DIFACTO_RENDEZVOUS=rv)
        procs.append(subprocess.Popen([os.path.join(built, "difacto"), "learner=lbfgs"] + list(args), stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env))
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


@pytest.mark.gpu
def test_lbfgs_cli_warm_start_on_two_ranks(built, lbfgs_runs):
    d = lbfgs_runs["dir"]
    args = ["data_in=" + DATA] + MIXED
    want = _accepted(lbfgs_runs["b"])
    # a world-2 run A writes <m2>.part-0, .part-1 and the manifest
    _run_ranks(built, 2, args + ["max_num_epochs=6", "model_out=" + str(d / "m2")], str(d / "rv_a"))
    assert os.path.exists(str(d / "m2.parts")) and not os.path.exists(str(d / "m2"))
    for tag, model in (("file", lbfgs_runs["model"]), ("parts", str(d / "m2"))):
        logs = _run_ranks(built, 2, args + ["max_num_epochs=1", "model_in=" + model], str(d / ("rv_" + tag)))
        assert _lines(logs[1]) == _lines(logs[0]), tag
        got = _accepted(logs[0])
        assert len(got) == len(want) >= 1
        np.testing.assert_allclose(got, want, rtol=1e-4)
        np.testing.assert_allclose(_starts(logs[0]), _starts(lbfgs_runs["b"]), rtol=1e-4)
        assert all(re.search(r"model loaded from \S+: [1-9]\d* of", l) for l in logs)


@pytest.mark.gpu
def test_predict_with_the_learner_that_trained(built, bcd_runs, lbfgs_runs, tmp_path):
    for learner, model, k in (("bcd", bcd_runs["model"], 0), ("lbfgs", lbfgs_runs["model"], 4)):
        p1, p2 = str(tmp_path / (learner + ".p1")), str(tmp_path / (learner + ".p2"))
        common = ["task=predict", "data_in=" + DATA, "data_val=" + DATA, "batch_size=100", "model_in=" + model]
        _ok(built, "learner=" + learner, "pred_out=" + p1, *(common + (["V_dim=4"] if k else [])))
        _ok(built, "learner=sgd", "V_dim=%d" % k, "pred_out=" + p2, *common)
        a, b = open(p1, "rb").read(), open(p2, "rb").read()
        assert len(a.splitlines()) == 100 and a == b, learner
        assert np.abs(np.loadtxt(p1)).max() > .05
    r = _difacto(built, "task=predict", "learner=bcd", "V_dim=3", "data_in=" + DATA, "batch_size=100",
                 "model_in=" + bcd_runs["model"], "pred_out=" + str(tmp_path / "p3"))
    assert r.returncode != 0 and "V_dim" in r.stderr


# ------------------------------------------------------------------------------------------------ L-BFGS, the C ABI
INIT = dict(tail_feature_filter=2, V_init_scale=.01, l2=.1, V_l2=.01)
K = 4
# V_threshold = 2 is the command-line tests' configuration: with tail_feature_filter = 2 a surviving key has count > 2 and
# so every key carries V.  V_threshold = 5 on the same rows gives the model with both kinds of keys (count 3 .. 5: no V).
V_THRESHOLDS = [2, 5]


def _lbfgs(ctx, vth):
    """the rcv1 rows in two chunks"""
    from difacto_amd import capi
    off, idx, val, lab = R.read_libsvm(DATA)
    o = capi.Lbfgs(ctx, K, 5)
    for r0, r1 in ((0, 47), (47, 100)):
        s = off[r0:r1 + 1]
        o.add_chunk(s - s[0], idx[int(s[0]):int(s[-1])], val[int(s[0]):int(s[-1])], lab[r0:r1])
    o.init_model(V_threshold=vth, **INIT)
    return o


def _ragged(keys, lens, w, pos, order):
    """the entries `order` of a flat model as (keys, lens, vals) of dfh_lbfgs_set_model"""
    vals = np.concatenate([w[pos[i]:pos[i] + lens[i]] for i in order]) if len(order) else np.zeros(0, np.float32)
    return keys[order], lens[order], vals.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("vth", V_THRESHOLDS)
def test_lbfgs_set_model_equals_set_weights(ctx, vth):
    x, y = _lbfgs(ctx, vth), _lbfgs(ctx, vth)
    try:
        m = x.get_model()
        lens, n = m["lens"], len(m["w"])
        assert np.any(lens == 1 + K) and n == lens.sum() and np.any(lens == 1) == (vth == 5)
        pos = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rng = np.random.default_rng(3)
        w = rng.normal(size=n).astype(np.float32) * f32(.1)
        assert x.set_model(*_ragged(m["keys"], lens, w, pos, rng.permutation(len(lens)))) == len(lens)
        y.set_weights(w)
        assert R.same_bits(x.get_model()["w"], w) and R.same_bits(y.get_model()["w"], w)
        gx, gy = x.calc_grad(), y.calc_grad()
        assert np.array([gx], np.float32).tobytes() == np.array([gy], np.float32).tobytes() and gx[0] > 0
    finally:
        x.close()
        y.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vth", V_THRESHOLDS)
def test_lbfgs_set_model_partial_input(ctx, vth):
    """vth = 5: every case; vth = 2: the model has no key without V, the other cases"""
    x, y = _lbfgs(ctx, vth), _lbfgs(ctx, vth)
    try:
        m = x.get_model()
        keys, lens, w0 = m["keys"], m["lens"], m["w"].copy()
        pos = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rng = np.random.default_rng(5)
        withV, noV = np.flatnonzero(lens > 1), np.flatnonzero(lens == 1)
        plain = np.r_[withV[::3], noV[::3]]                # given as the model holds them
        short, long_ = withV[1::3][:9], noV[1::3][:9]      # lens = 1 for a key with V; V for a key without
        unseen = np.setdiff1d(np.array([1, 2, 3, 2 ** 63 + 11, 2 ** 64 - 1], np.uint64), keys)
        in_keys, in_lens, in_vals, want = [], [], [], w0.copy()
        for i in np.r_[plain, short, long_]:
            l = 1 if i in short else 1 + K if i in long_ else int(lens[i])
            v = rng.normal(size=l).astype(np.float32)
            in_keys.append(keys[i]); in_lens.append(l); in_vals.append(v)
            c = min(l, int(lens[i]))                       # V only where both sides carry one
            want[pos[i]:pos[i] + c] = v[:c]
        for j, key in enumerate(unseen):
            l = 1 + K * (j % 2)
            in_keys.append(key); in_lens.append(l); in_vals.append(rng.normal(size=l).astype(np.float32))
        o = rng.permutation(len(in_keys))
        in_keys = np.array(in_keys, np.uint64)[o]
        in_lens = np.array(in_lens, np.int32)[o]
        in_vals = np.concatenate([in_vals[i] for i in o])
        assert len(short) and (len(long_) > 0) == (vth == 5) and len(unseen) >= 3
        assert x.set_model(in_keys, in_lens, in_vals) == len(plain) + len(short) + len(long_)
        y.set_weights(want)
        got = x.get_model()["w"]
        assert R.same_bits(got, want)
        # the V of a key given with lens = 1 keeps its initial value
        assert all(R.same_bits(got[pos[i] + 1:pos[i + 1]], w0[pos[i] + 1:pos[i + 1]]) and w0[pos[i] + 1] != 0 for i in short)
        gx, gy = x.calc_grad(), y.calc_grad()
        assert np.array([gx], np.float32).tobytes() == np.array([gy], np.float32).tobytes()
    finally:
        x.close()
        y.close()


@pytest.mark.gpu
def test_lbfgs_set_model_refusals(ctx):
    from difacto_amd import capi
    x = _lbfgs(ctx, 5)
    try:
        m = x.get_model()
        k2 = np.r_[m["keys"][:4], m["keys"][2:3]]
        with pytest.raises(capi.DfhError, match="not unique"):
            x.set_model(k2, np.ones(5, np.int32), np.zeros(5, np.float32))
        with pytest.raises(capi.DfhError, match="lens"):
            x.set_model(m["keys"][:1], np.array([2], np.int32), np.zeros(2, np.float32))
        assert x.owned_range() == (0, 0)
        x.calc_grad()
        with pytest.raises(capi.DfhError, match="gradient pass has run"):
            x.set_model(m["keys"][:1], np.ones(1, np.int32), np.zeros(1, np.float32))
    finally:
        x.close()
