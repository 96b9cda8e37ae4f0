"""The device feed at sizes where every minibatch is a first call of its size class or a single tile: the gather launch
(k_gather_rows_staged) and k_loc_describe's block bases are the code under test, then — on a second pass over the same
objects, with stored splitters — the count pass's own gather.  Four ways to feed one minibatch must agree bit for bit:
dfh_batch_load_host + dfh_localize, dfh_batch_gather_rows + dfh_localize, dfh_batch_prepare_rows, dfh_batch_prepare_cached."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(l1=0.02, l2=0.01, lr=0.3, V_lr=0.05, V_l2=0.02, V_threshold=0, V_init_scale=0.2, seed=5)
PATHS = ("load_host", "gather_rows", "prepare_rows", "prepare_cached")
MAX_ROWS, MAX_NNZ = 64, 64 * 12


def _buffer(rng, lens, binary):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(off[-1])
    return dict(offset=off, index=rng.integers(1, 2000, size=nnz).astype(np.uint64),
                value=None if binary else rng.uniform(0.1, 2.0, size=nnz).astype(np.float32),
                label=rng.choice(np.array([-1.0, 1.0], np.float32), size=len(lens)))


@pytest.fixture(scope="module")
def feed():
    """one context; three row buffers of 64 / 48 / 40 rows with 0..12 ids per row below 2 000 (they share keys): one with
    values, one binary, one with values and runs of empty rows; all three carry their labels"""
    from difacto_amd import capi
    capi.lib()
    rng = np.random.default_rng(47)
    lens2 = rng.integers(0, 13, size=40)
    lens2[5:15] = 0
    lens2[25:32] = 0
    host = [_buffer(rng, rng.integers(0, 13, size=64), False), _buffer(rng, rng.integers(0, 13, size=48), True),
            _buffer(rng, lens2, False)]
    ctx = capi.Context(0)
    rbs = []
    for hb in host:
        rb = capi.RowBuf(ctx, len(hb["label"]), max(int(hb["offset"][-1]), 1))
        rb.load_host(hb["offset"], hb["index"], hb["value"])
        rb.set_labels(hb["label"])
        rbs.append(rb)
    plans = dict(
        a=[(0, rng.permutation(64)[:20]), (1, rng.permutation(48)[:15])],                  # 20 + 15 rows from two buffers
        b=[(0, np.array([3, 9, 9, 17, 9, 2, 9, 40]))],                                     # a row four times
        c=[(2, np.array([5, 14, 7, 7, 25, 31, 30]))],                                      # empty rows only: nnz == 0
        d=[(0, rng.permutation(64)[:9]), (2, np.zeros(0, np.int64)), (1, rng.permutation(48)[:11])])  # an empty segment
    yield dict(capi=capi, ctx=ctx, host=host, rbs=rbs, plans=plans)
    for rb in rbs:
        rb.close()
    ctx.close()


def _host_minibatch(host, segments):
    off, idx, val, lab = [0], [np.zeros(0, np.uint64)], [np.zeros(0, np.float32)], []
    anyv = any(host[g]["value"] is not None for g, _ in segments)
    for g, rows in segments:
        hb = host[g]
        for r in rows:
            lo, hi = int(hb["offset"][r]), int(hb["offset"][r + 1])
            idx.append(hb["index"][lo:hi])
            val.append(hb["value"][lo:hi] if hb["value"] is not None else np.ones(hi - lo, np.float32))
            lab.append(hb["label"][r])
            off.append(off[-1] + hi - lo)
    return dict(offset=np.array(off, np.uint64), index=np.concatenate(idx),
                value=np.concatenate(val).astype(np.float32) if anyv else None, label=np.array(lab, np.float32))


def _feed(path, f, bt, tb, segments):
    mb = _host_minibatch(f["host"], segments)
    segs = [(f["rbs"][g], rows) for g, rows in segments]
    if path == "load_host":
        bt.load_host(mb["offset"], mb["index"], mb["value"], mb["label"])
        bt.localize()
    elif path == "gather_rows":
        bt.gather_rows(mb["offset"], mb["label"], segs)
        bt.localize()
    elif path == "prepare_rows":
        bt.prepare_rows(tb, mb["offset"], mb["label"], segs)
    else:
        bt.prepare_cached(tb, segs)
    return mb


def _same_minibatch(bt, want_bt, nnz):
    (o0, l0), (o1, l1) = want_bt.get_rows(), bt.get_rows()
    assert np.array_equal(o0, o1) and np.array_equal(l0, l1)
    if nnz == 0:
        assert bt.shape() == want_bt.shape()
        return
    g0, g1 = want_bt.get_localized(), bt.get_localized()
    for k in ("feaids", "index", "feacnt"):
        assert np.array_equal(g0[k], g1[k]), k


def test_four_paths_agree_on_the_fall_back_shapes(feed):
    capi, ctx = feed["capi"], feed["ctx"]
    tbs = [capi.Table(ctx, 1 << 12, V_dim=8, init_mode=capi.INIT_HASH, **KW) for _ in PATHS]
    bts = [capi.Batch(ctx, MAX_ROWS, MAX_NNZ) for _ in PATHS]
    keys = set()
    for rnd in range(2):   # the second pass has stored splitters: the count pass gathers where it can
        for name in "abcd":
            segments = feed["plans"][name]
            for path, bt, tb in zip(PATHS, bts, tbs):
                mb = _feed(path, feed, bt, tb, segments)
            nnz = int(mb["offset"][-1])
            assert (nnz == 0) == (name == "c")
            assert np.array_equal(bts[0].get_rows()[0], mb["offset"].astype(np.uint32))
            for bt in bts[1:]:
                _same_minibatch(bt, bts[0], nnz)
            if nnz == 0:
                continue
            keys.update(bts[0].get_localized()["feaids"].tolist())
            for bt, tb in zip(bts, tbs):
                bt.sgd_step(tb, is_train=True, push_cnt=rnd == 0)
            preds = [bt.pred() for bt in bts]
            for p in preds[1:]:
                assert np.array_equal(preds[0], p), (rnd, name)
    pulled = [tb.pull(np.array(sorted(keys), np.uint64)) for tb in tbs]
    for v, l in pulled[1:]:
        assert np.array_equal(pulled[0][0], v) and np.array_equal(pulled[0][1], l)
    for o in bts + tbs:
        o.close()


def test_a_refused_call_leaves_the_object_usable(feed):
    """the refusals that come after the argument checks — behind the phase's begin, in the middle of the staging writes —
    leave a batch object that takes the next minibatch as if nothing had happened"""
    capi, ctx, rbs = feed["capi"], feed["ctx"], feed["rbs"]
    plan = feed["plans"]["a"]
    mb = _host_minibatch(feed["host"], plan)
    segs = [(rbs[g], rows) for g, rows in plan]
    bare = capi.RowBuf(ctx, 8, 8)   # uploaded, never given labels
    bare.load_host(np.arange(9, dtype=np.uint64), np.arange(8, dtype=np.uint64) + 1)

    def stepped(path, bt):
        tb = capi.Table(ctx, 1 << 12, V_dim=8, init_mode=capi.INIT_HASH, **KW)
        _feed(path, feed, bt, tb, plan)
        rows, loc = bt.get_rows(), bt.get_localized()
        bt.sgd_step(tb, is_train=True, push_cnt=True)
        bt.sgd_step(tb, is_train=True)   # (a fresh model predicts zero: the second step's predictions carry the values)
        out = (rows, loc, bt.pred(), tb.pull(loc["feaids"]))
        tb.close()
        return out

    ref_bt = capi.Batch(ctx, MAX_ROWS, MAX_NNZ)
    want = stepped("load_host", ref_bt)
    ref_bt.close()

    beyond = [(rbs[0], np.array([1, 64, 2])), (rbs[1], plan[1][1])]
    off_beyond = np.concatenate([[0], np.cumsum(np.ones(3 + len(plan[1][1]), np.uint64))]).astype(np.uint64)
    down = mb["offset"].copy()
    k = 1 + int(np.argmax(down >= 1))   # the row after the first one that starts at or beyond 1 now starts one short of it
    assert k < len(down) - 1
    down[k] = down[k - 1] - 1
    assert down[k] < down[k - 1] and down[-1] == mb["offset"][-1]
    cases = [
        ("prepare_rows", lambda bt, tb: bt.prepare_rows(tb, off_beyond, np.ones(len(off_beyond) - 1, np.float32), beyond),
         "dfh_batch_prepare_rows: row number beyond the buffer"),
        ("prepare_rows", lambda bt, tb: bt.prepare_rows(tb, np.append(mb["offset"], mb["offset"][-1]), np.append(mb["label"], 1.0), segs),
         "dfh_batch_prepare_rows: the segments must hold nrows rows"),
        ("prepare_cached", lambda bt, tb: bt.prepare_cached(tb, [(rbs[0], plan[0][1]), (bare, np.array([0, 1]))]),
         "dfh_batch_prepare_cached: a row buffer without labels"),
        ("gather_rows", lambda bt, tb: bt.gather_rows(down, mb["label"], segs), "dfh_batch_gather_rows: offsets must not decrease"),
    ]
    for path, call, message in cases:
        bt = capi.Batch(ctx, MAX_ROWS, MAX_NNZ)
        tb = capi.Table(ctx, 1 << 12, V_dim=8, init_mode=capi.INIT_HASH, **KW)
        with pytest.raises(capi.DfhError) as e:
            call(bt, tb)
        assert message in str(e.value)
        tb.close()
        rows, loc, pred, pulled = stepped(path, bt)
        assert np.array_equal(rows[0], want[0][0]) and np.array_equal(rows[1], want[0][1]), message
        for key in ("feaids", "index", "feacnt"):
            assert np.array_equal(loc[key], want[1][key]), (message, key)
        assert np.array_equal(pred, want[2]), message
        assert np.array_equal(pulled[0], want[3][0]) and np.array_equal(pulled[1], want[3][1]), message
        bt.close()
    bare.close()


def test_rowbuf_load_host_equals_load_host_slices(feed):
    """one buffer uploaded whole and as three slices, the middle one without a value array beside two with: the same ids, ones
    for the middle slice's values (seen through the Localizer's outputs and a step: the library has no getter for a
    minibatch's raw arrays); a buffer without any values has none after either call"""
    capi, ctx = feed["capi"], feed["ctx"]
    hb = feed["host"][0]
    off, idx, val, lab = hb["offset"], hb["index"], hb["value"], hb["label"]
    cut = [0, int(off[20]), int(off[45]), int(off[64])]   # slices at row borders
    assert cut[0] < cut[1] < cut[2] < cut[3]
    val_mid_ones = val.copy()
    val_mid_ones[cut[1]:cut[2]] = 1.0
    assert not np.array_equal(val_mid_ones, val)

    def stepped(feed_it):
        tb = capi.Table(ctx, 1 << 12, V_dim=8, init_mode=capi.INIT_HASH, **KW)
        bt = capi.Batch(ctx, MAX_ROWS, MAX_NNZ)
        feed_it(bt, tb)
        loc = bt.get_localized()
        bt.sgd_step(tb, is_train=True, push_cnt=True)
        bt.sgd_step(tb, is_train=True)   # (a fresh model predicts zero: the second step's predictions carry the values)
        out = (loc, bt.pred(), tb.pull(loc["feaids"]))
        bt.close()
        tb.close()
        return out

    def same(got, want):
        for key in ("feaids", "index", "feacnt"):
            assert np.array_equal(got[0][key], want[0][key]), key
        assert np.array_equal(got[1], want[1])
        assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1])

    def host(value):
        def feed_it(bt, tb):
            bt.load_host(off, idx, value, lab)
            bt.localize()
        return stepped(feed_it)

    def device(rb):
        return stepped(lambda bt, tb: bt.prepare_rows(tb, off, lab, [(rb, np.arange(64))]))

    def uploaded(values):
        whole, sliced = capi.RowBuf(ctx, 64, len(idx)), capi.RowBuf(ctx, 64, len(idx))
        whole.load_host(off, idx, values[0])
        sliced.load_host_slices(off, [(idx[cut[g]:cut[g + 1]], values[1][g]) for g in range(3)])
        return whole, sliced

    whole, sliced = uploaded((val, [val[cut[0]:cut[1]], None, val[cut[2]:cut[3]]]))
    want_whole, want_sliced = host(val), host(val_mid_ones)
    assert not np.array_equal(want_whole[1], want_sliced[1])   # the step sees the difference
    same(device(whole), want_whole)
    same(device(sliced), want_sliced)
    whole.close()
    sliced.close()
    whole, sliced = uploaded((None, [None, None, None]))
    want = host(None)
    same(device(whole), want)
    same(device(sliced), want)
    whole.close()
    sliced.close()
