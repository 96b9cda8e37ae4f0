"""The whole-set evaluator (csrc/dfh_eval.hip) through capi.Eval: exact AUC (auc2 = 2 x pairs ranked right + tied pairs, an
integer), correct rows and the fp64 logloss sum of everything appended, against the numpy / Python-integer oracle of
tests/eval_ref.py.  Integer fields must be equal; objv within (n + 16) 2^-52 of the sum of the terms' magnitudes.

A tile of the ranking kernels is 2 048 sorted rows (256 threads x 8).  The small sizes (7 .. 8 193 rows, and sets of up to
240 000 rows = 118 tiles) sit on and around one thread's rows, one tile and several tiles, and their tie-heavy cases make
every tie group span every tile boundary.  k_eval_scan, k_eval_reduce and k_eval_final are single blocks that take 256 tiles
per trip, so the cases from 524 287 rows on (the last section; up to 1 048 581 rows = 513 tiles, a third trip) sit on and
around 256 tiles: the carries between trips, a tie group and a head record that cross from one trip into a later one, and
tiles wholly behind the ranked rows."""
import numpy as np
import pytest

import eval_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def run(dev, label, pred, hint=0):
    capi, ctx = dev
    e = capi.Eval(ctx, hint)
    try:
        e.append_host(label, pred)
        return e.finish()
    finally:
        e.close()


def labels01(rng, n, p=0.4):
    return np.where(rng.random(n) < p, 1.0, 0.0).astype(np.float32)


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_empty(dev):
    capi, ctx = dev
    e = capi.Eval(ctx)
    r = e.finish()
    assert R.fields(r) == (0, 0, 0, 0, 0, 0, np.float64(0).tobytes())
    e.append_host(np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert R.fields(e.finish()) == R.fields(r)
    e.close()


@pytest.mark.parametrize("lab,s", [(1.0, 0.5), (0.0, 0.5), (1.0, -2.0), (0.0, 0.0), (1.0, float("nan"))])
def test_one_row(dev, lab, s):
    label, pred = np.array([lab], np.float32), np.array([s], np.float32)
    r = run(dev, label, pred)
    R.check(r, R.oracle(label, pred))
    assert r.auc2 == 0


@pytest.mark.parametrize("sp,sq,auc2", [(1.0, -1.0, 2), (0.25, 0.25, 1), (-1.0, 1.0, 0)])
def test_two_rows(dev, sp, sq, auc2):
    for order in (0, 1):
        label = np.array([1, 0] if order == 0 else [0, 1], np.float32)
        pred = np.array([sp, sq] if order == 0 else [sq, sp], np.float32)
        r = run(dev, label, pred)
        R.check(r, R.oracle(label, pred))
        assert r.auc2 == auc2


@pytest.mark.parametrize("lab", [0.0, 1.0])
def test_one_class_only(dev, lab):
    rng = np.random.default_rng(1)
    pred = rng.normal(size=5000).astype(np.float32)
    label = np.full(5000, lab, np.float32)
    r = run(dev, label, pred)
    R.check(r, R.oracle(label, pred))
    assert r.auc2 == 0 and (r.n_pos == 0 or r.n_neg == 0)


def test_all_tied(dev):
    rng = np.random.default_rng(2)
    label = np.zeros(10000, np.float32)
    label[rng.permutation(10000)[:3000]] = 1
    pred = np.full(10000, 0.75, np.float32)
    r = run(dev, label, pred)
    R.check(r, R.oracle(label, pred))
    assert r.auc2 == 3000 * 7000


def test_three_distinct_scores(dev):
    rng = np.random.default_rng(3)
    n = 50000
    pred = rng.choice(np.array([-1.5, 0.0, 2.0], np.float32), size=n)
    label = labels01(rng, n)
    R.check(run(dev, label, pred), R.oracle(label, pred))


def test_distinct_scores(dev):
    rng = np.random.default_rng(4)
    n = 50000
    pred = (rng.permutation(n).astype(np.float32) - n / 2) / 4096   # exact in float32, all different
    assert np.unique(pred).size == n
    label = (rng.random(n) < 1 / (1 + np.exp(-pred))).astype(np.float32)
    R.check(run(dev, label, pred), R.oracle(label, pred))


@pytest.mark.parametrize("n", [7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193])
def test_rounded_scores(dev, n):
    rng = np.random.default_rng(n)
    pred = (np.round(rng.normal(size=n) * 64) / 64).astype(np.float32)
    label = labels01(rng, n)
    R.check(run(dev, label, pred), R.oracle(label, pred), "n = %d" % n)


SPECIAL = dict(
    inf=[np.inf, -np.inf],
    zeros=[0.0, -0.0],
    denormals=[1e-45, -1e-45, 1e-40, -1e-40, 0.0],
    flt_max=[np.finfo(np.float32).max, -np.finfo(np.float32).max],
)


@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_special_values(dev, name):
    rng = np.random.default_rng(5)
    base = np.array(SPECIAL[name], np.float32)
    pred = np.concatenate([base, base, rng.normal(size=40).astype(np.float32), base, base])   # each value with both labels, twice
    k = base.size
    label = np.concatenate([np.ones(k), np.zeros(k), labels01(rng, 40), np.zeros(k), np.ones(k)]).astype(np.float32)
    want = R.oracle(label, pred)
    r = run(dev, label, pred)
    R.check(r, want, name)
    if name == "inf":
        assert r.objv == np.inf


def test_negative_zero_ties_with_zero(dev):
    pred = np.array([0.0, -0.0, -0.0, 0.0], np.float32)
    label = np.array([1, 0, 1, 0], np.float32)
    r = run(dev, label, pred)
    R.check(r, R.oracle(label, pred))
    assert r.auc2 == 4 and r.correct == 2   # 2 x 2 tied pairs; s <= 0 is right for the negatives only


def test_nan_predictions_of_both_signs(dev):
    rng = np.random.default_rng(6)
    nans = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF])
    pred = np.concatenate([nans, rng.normal(size=3000).astype(np.float32), nans, np.array([np.inf, -np.inf], np.float32)])
    label = labels01(rng, pred.size)
    label[:6] = [1, 0, 1, 0, 1, 0]
    perm = rng.permutation(pred.size)
    pred, label = pred[perm], label[perm]
    want = R.oracle(label, pred)
    assert want.n_nan == 12
    R.check(run(dev, label, pred), want)
    # NaN predictions only
    r = run(dev, np.array([1, 0, 1], np.float32), nans[:3])
    assert (r.n, r.n_pos, r.n_neg, r.n_nan, r.auc2, r.correct, r.objv) == (3, 0, 0, 3, 0, 0, 0.0)


def test_label_values(dev):
    rng = np.random.default_rng(7)
    n = 6000
    label = rng.choice(np.array([-1, 0, -0.0, 0.5, 1, 2, np.nan], np.float32), size=n)
    pred = (np.round(rng.normal(size=n) * 16) / 16).astype(np.float32)
    want = R.oracle(label, pred)
    assert want.n_pos == int(np.isin(label, [0.5, 1, 2]).sum())
    R.check(run(dev, label, pred), want)


def test_objv_is_inf_only_on_the_wrong_side(dev):
    pred = np.array([np.inf, -np.inf, 1.0, -1.0], np.float32)
    right = np.array([1, 0, 1, 0], np.float32)
    r = run(dev, right, pred)
    R.check(r, R.oracle(right, pred))
    assert np.isfinite(r.objv)
    for wrong in ([0, 0, 1, 0], [1, 1, 1, 0]):
        label = np.array(wrong, np.float32)
        r = run(dev, label, pred)
        R.check(r, R.oracle(label, pred))
        assert r.objv == np.inf


def test_same_bits_however_the_rows_are_appended(dev):
    capi, ctx = dev
    rng = np.random.default_rng(8)
    n = 20000
    pred = (np.round(rng.normal(size=n) * 256) / 256).astype(np.float32)
    pred[rng.integers(0, n, 50)] = np.nan
    label = labels01(rng, n)
    want = R.oracle(label, pred)
    at_once = run(dev, label, pred)
    R.check(at_once, want)
    # 300 uneven pieces, the first allocation one row: the arrays grow many times and keep their content
    cuts = np.sort(rng.choice(np.arange(1, n), size=299, replace=False))
    e = capi.Eval(ctx, 1)
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]])):
        e.append_host(label[a:b], pred[a:b])
    pieces = e.finish()
    assert R.fields(e.finish()) == R.fields(pieces), "two finish calls without an append"
    e.close()
    # row by row for the first 300 rows, the rest at once
    e = capi.Eval(ctx, 1)
    for i in range(300):
        e.append_host(label[i:i + 1], pred[i:i + 1])
    e.append_host(label[300:], pred[300:])
    rows = e.finish()
    e.close()
    assert R.fields(pieces) == R.fields(at_once) and R.fields(rows) == R.fields(at_once)
    assert R.fields(run(dev, label, pred)) == R.fields(at_once), "a second run"


def test_finish_keeps_the_rows_and_reset_empties(dev):
    capi, ctx = dev
    rng = np.random.default_rng(9)
    pred = rng.normal(size=7000).astype(np.float32)
    label = labels01(rng, 7000)
    e = capi.Eval(ctx, 16)
    e.append_host(label[:3000], pred[:3000])
    R.check(e.finish(), R.oracle(label[:3000], pred[:3000]))
    e.append_host(label[3000:], pred[3000:])   # append after finish accumulates
    R.check(e.finish(), R.oracle(label, pred))
    e.reset()
    assert R.fields(e.finish())[:6] == (0, 0, 0, 0, 0, 0)
    e.append_host(label[:100], pred[:100])
    R.check(e.finish(), R.oracle(label[:100], pred[:100]))
    e.close()


def test_append_batch(dev, rcv1):
    """the batch's own predictions and labels, queued behind its step: equal to append_host of dfh_batch_get_pred and the
    labels; two batches appended back to back with no host wait in between"""
    capi, ctx = dev
    off, idx, val, lab = (rcv1[k] for k in ("offset", "index", "value", "label"))
    tb = capi.Table(ctx, 1 << 14, V_dim=4, init_mode=capi.INIT_HASH, V_threshold=0, V_init_scale=0.3, lr=0.5, l1=0.0, seed=3)

    def part(a, b):
        o = off[a:b + 1]
        return (o - o[0]).astype(np.uint64), idx[int(o[0]):int(o[-1])], val[int(o[0]):int(o[-1])], lab[a:b]

    warm = capi.Batch(ctx, 128, 1 << 15)
    warm.load_host(*part(0, 100))
    warm.localize()
    for _ in range(3):   # a model whose predictions differ from row to row
        warm.sgd_step(tb, is_train=True, push_cnt=False)
    b1, b2 = capi.Batch(ctx, 128, 1 << 15), capi.Batch(ctx, 128, 1 << 15)
    e = capi.Eval(ctx, 8)
    b1.load_host(*part(0, 64))
    b1.localize()
    b1.sgd_step(tb, is_train=False)
    e.append_batch(b1)
    p1 = b1.pred()
    assert np.unique(p1).size > 8
    one = e.finish()
    R.check(one, R.oracle(lab[:64], p1))
    assert R.fields(one) == R.fields(run(dev, lab[:64], p1))
    # two batches, nothing waits between the steps and the appends
    e.reset()
    b2.load_host(*part(64, 100))
    b2.localize()
    b1.sgd_step(tb, is_train=False)
    e.append_batch(b1)
    b2.sgd_step(tb, is_train=False)
    e.append_batch(b2)
    two = e.finish()
    p2 = b2.pred()
    both = np.concatenate([b1.pred(), p2])
    assert np.array_equal(both[:64], p1)
    R.check(two, R.oracle(lab, both))
    assert R.fields(two) == R.fields(run(dev, lab, both))
    for o in (e, b1, b2, warm, tb):
        o.close()


def test_append_batch_with_pipelined_preparation(rcv1):
    """the learner's loop: preparation streams on, three batch objects in rotation, load -> localize -> step -> append with
    no host wait.  The next load into an object runs on a preparation stream and may overwrite its labels as soon as the
    object's `free` event has passed, so the append has to move that event behind its copies: every minibatch carries the
    same rows under labels of its own (a different share of positives each), and the evaluator must hold exactly those"""
    from difacto_amd import capi
    off, idx, val = (np.tile(rcv1[k], 1) for k in ("offset", "index", "value"))
    reps = 40   # 4 000 rows per minibatch: a step takes longer than the host needs to queue the next one
    nnz = int(off[-1])
    off = np.concatenate([[0], (off[1:][None, :] + (np.arange(reps) * nnz)[:, None]).ravel()]).astype(np.uint64)
    idx, val = np.tile(idx, reps), np.tile(val, reps)
    nrows, steps = off.size - 1, 60
    rng = np.random.default_rng(11)
    labels = [np.where(rng.random(nrows) < (i + 1) / (steps + 1), 1.0, -1.0).astype(np.float32) for i in range(steps)]
    ctx = capi.Context(0)
    ctx.set_pipeline(True)
    tb = capi.Table(ctx, 1 << 15, V_dim=4, init_mode=capi.INIT_HASH, V_threshold=0, V_init_scale=0.3, lr=0.5, l1=0.0, seed=3)
    bs = [capi.Batch(ctx, nrows, idx.size) for _ in range(3)]
    bs[0].load_host(off, idx, val, labels[0])
    bs[0].localize()
    for _ in range(3):
        bs[0].sgd_step(tb, is_train=True, push_cnt=False)
    bs[0].sgd_step(tb, is_train=False)
    pred = bs[0].pred()   # the model no longer changes: every minibatch below has these predictions
    assert np.unique(pred).size > 8
    e = capi.Eval(ctx, 1000)
    for i in range(steps):
        b = bs[i % 3]
        b.load_host(off, idx, val, labels[i])
        b.localize()
        b.sgd_step(tb, is_train=False)
        e.append_batch(b)
    got = e.finish()
    want = R.oracle(np.concatenate(labels), np.tile(pred, steps))
    R.check(got, want)
    assert np.array_equal(bs[(steps - 1) % 3].pred(), pred)
    for o in [e] + bs + [tb]:
        o.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ beyond 256 tiles
# k_eval_scan, k_eval_reduce and k_eval_final are single blocks that take 256 tiles per trip: from C + 1 rows on there is a
# second trip, fed by the carries run_neg and run_head and by the p >= 256 stride of the two reductions.
T = 2048
C = 256 * T


def shuffled(rng, label, pred):
    perm = rng.permutation(pred.size)
    return np.ascontiguousarray(label[perm], np.float32), np.ascontiguousarray(pred[perm], np.float32)


def distinct_sorted(n):
    """n different scores in ascending order, exact in float32"""
    assert n < 1 << 24
    return ((np.arange(n) - n // 2) / 4096).astype(np.float32)


_BIG = {}


def big_rounded(n):
    if n not in _BIG:
        rng = np.random.default_rng(n)
        pred = (np.round(rng.normal(size=n) * 64) / 64).astype(np.float32)
        _BIG[n] = (labels01(rng, n), pred)
    return _BIG[n]


@pytest.mark.parametrize("n", [C - 1, C, C + 1, C + T + 1, 2 * C + 5])
def test_rounded_scores_beyond_one_trip(dev, n):
    """256 tiles less a row, 256 tiles, the first row of a second trip, a whole tile and a row of it, and a third trip"""
    label, pred = big_rounded(n)
    assert -(-n // T) == {C - 1: 256, C: 256, C + 1: 257, C + T + 1: 258, 2 * C + 5: 513}[n]
    R.check(run(dev, label, pred), R.oracle(label, pred), "n = %d" % n)


def test_all_tied_beyond_one_trip(dev):
    """one group: the only head is row 0, every tile's partial is 0 and the whole of auc2 is k_eval_final's last group"""
    n = C + T + 1
    label = labels01(np.random.default_rng(21), n)
    pred = np.full(n, -0.5, np.float32)
    r = run(dev, label, pred)
    R.check(r, R.oracle(label, pred))
    assert r.auc2 == r.n_pos * r.n_neg and r.n_pos > 0 and r.n_neg > 0


@pytest.mark.parametrize("at", [C - 1, C, C + 1])
def test_two_values_switching_at_the_trip_boundary(dev, at):
    """the second group's head is sorted row `at`: the last row of the first trip, the first row of the second (no head
    record in front of it but run_head's), and its second row"""
    n = C + T + 1
    rng = np.random.default_rng(22 + at)
    pred = np.where(np.arange(n) < at, -1.0, 1.0).astype(np.float32)
    label, pred = shuffled(rng, labels01(rng, n), pred)
    assert int((pred < 0).sum()) == at
    R.check(run(dev, label, pred), R.oracle(label, pred), "switch at %d" % at)


def test_a_tie_group_from_tile_250_to_tile_300(dev):
    """different scores, one group of equal ones from inside tile 250 to inside tile 300, different scores again: the tiles
    256 .. 299 of the second trip hold no head and take the first trip's last one, and the group that ends in tile 300
    reads a head 50 tiles back"""
    n = 301 * T + 9
    lo, hi = 250 * T + 100, 300 * T + 57
    pred = distinct_sorted(n)
    pred[lo:hi] = pred[lo]
    assert lo // T == 250 and (hi - 1) // T == 300 and hi // T == 300 and np.unique(pred).size == n - (hi - lo) + 1
    assert pred[lo - 1] < pred[lo] == pred[hi - 1] < pred[hi]
    rng = np.random.default_rng(23)
    label, pred = shuffled(rng, labels01(rng, n), pred)
    R.check(run(dev, label, pred), R.oracle(label, pred))


def test_distinct_scores_beyond_one_trip(dev):
    """every row is a head"""
    rng = np.random.default_rng(24)
    n = C + T + 1
    pred = (rng.permutation(n).astype(np.float32) - n / 2) / 4096   # exact in float32, all different
    assert np.unique(pred).size == n
    label = (rng.random(n) < 1 / (1 + np.exp(-pred / 16))).astype(np.float32)
    R.check(run(dev, label, pred), R.oracle(label, pred))


@pytest.mark.parametrize("negatives_below", [True, False])
def test_separated_classes_beyond_one_trip(dev, negatives_below):
    """the lower class fills the first trip and seven rows more, so the upper class lies wholly in later trips: with the
    negatives below, every NP of a positive's group comes through run_neg"""
    n = C + T + 1
    n_low = C + 7
    rng = np.random.default_rng(25)
    mag = np.abs(np.round(rng.normal(size=n) * 64) / 64)
    pred = np.where(np.arange(n) < n_low, -1.0 - mag, 1.0 + mag).astype(np.float32)
    label = ((np.arange(n) >= n_low) == negatives_below).astype(np.float32)
    label, pred = shuffled(rng, label, pred)
    r = run(dev, label, pred)
    R.check(r, R.oracle(label, pred))
    n_pos = n - n_low if negatives_below else n_low
    assert (r.n_pos, r.n_neg) == (n_pos, n - n_pos)
    assert r.auc2 == (2 * n_pos * (n - n_pos) if negatives_below else 0)


def test_nan_tail_of_more_than_three_tiles(dev):
    """m = n - n_nan is three rows past 256 tiles: tile 256 holds three ranked rows and the last three tiles none"""
    n = C + 4 * T
    n_nan = 4 * T - 3
    rng = np.random.default_rng(26)
    pred = (np.round(rng.normal(size=n) * 64) / 64).astype(np.float32)
    nans = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF])
    pred[rng.choice(n, size=n_nan, replace=False)] = nans[rng.integers(0, 4, n_nan)]
    label = labels01(rng, n)
    want = R.oracle(label, pred)
    assert want.n_nan == n_nan and n - n_nan == C + 3 and -(-n // T) - -(-(n - n_nan) // T) == 3
    R.check(run(dev, label, pred), want)


def test_same_bits_in_seven_pieces_beyond_two_trips(dev):
    """2C + 5 rows at once and in 7 uneven pieces from a capacity hint of 1: the arrays grow by doubling under the pieces"""
    capi, ctx = dev
    n = 2 * C + 5
    label, pred = big_rounded(n)
    at_once = run(dev, label, pred)
    cuts = [0, 1, 3, T + 1, C - 1, C + 2, 2 * C - 77, n]
    e = capi.Eval(ctx, 1)
    for a, b in zip(cuts[:-1], cuts[1:]):
        e.append_host(label[a:b], pred[a:b])
    pieces = e.finish()
    e.close()
    R.check(pieces, R.oracle(label, pred))
    assert R.fields(pieces) == R.fields(at_once)


def test_too_many_rows_are_refused_by_the_argument(dev):
    capi, ctx = dev
    e = capi.Eval(ctx)
    rc = capi.lib().dfh_eval_append_host(e.h, None, None, 2 ** 32 - 16)   # nothing is read or allocated
    assert rc == 1 and b"2^32 - 16" in capi.lib().dfh_last_error()
    assert R.fields(e.finish())[:6] == (0, 0, 0, 0, 0, 0)
    e.close()
    with pytest.raises(capi.DfhError) as err:
        capi.Eval(ctx, 2 ** 32 - 16)
    assert err.value.code == 1
