"""exact_metrics by group (csrc/dfh_eval_groups.hip) through capi.Eval: every group's integers exactly, objv per group by the
criterion of tests/eval_ref.py, gauc_num against a Fraction.  T = 2 048 rows is the tile of the segmented pass (GV_TILE = 256
threads x 8 rows); the shapes put group and tie borders on, before and behind tile borders.  The reference is eval_ref.oracle
applied to each group's rows alone."""
import fractions

import numpy as np
import pytest

import eval_ref as R

pytestmark = pytest.mark.gpu
T = 2048
U64 = 2 ** 64 - 1
ERR_ARG, ERR_STATE = 1, 4   # DFH_ERR_ARG, DFH_ERR_STATE (include/difacto_hip.h)


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import build, capi as m
    build.build_hip()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def summary(s):
    return (s.n_groups, s.n_mixed, s.rows_mixed, s.n_nogroup, np.float64(s.gauc_num).tobytes())


def refused(capi, code, call, *args):
    with pytest.raises(capi.DfhError) as err:
        call(*args)
    assert err.value.code == code


def run(capi, ctx, label, pred, gid, has=None, cut=None):
    """-> (summary fields, the records, dfh_eval_finish's fields) of the rows appended `cut` at a time (None: at once)"""
    e = capi.Eval(ctx)
    e.group_by_slot(0)
    n = len(label)
    for a in range(0, n, cut or max(n, 1)):
        b = min(n, a + (cut or n))
        e.append_host_groups(label[a:b], pred[a:b], gid[a:b], None if has is None else has[a:b])
    s = e.finish_groups()
    rec = e.read_groups(0, s.n_groups)
    whole = e.finish()
    e.close()
    return summary(s), rec, whole


def check(label, pred, gid, has, got, what):
    (n_groups, n_mixed, rows_mixed, n_nogroup, gauc_bits), rec, _ = got
    has = np.ones(len(label), bool) if has is None else np.asarray(has, bool)
    ids = sorted(set(int(g) for g in gid[has]))
    assert [int(g) for g in rec["gid"]] == ids and n_groups == len(ids) and n_nogroup == int((~has).sum()), what
    num, rows, mixed = fractions.Fraction(0), 0, 0
    for i, g in enumerate(ids):
        sel = has & (gid == np.uint64(g))
        want = R.oracle(label[sel], pred[sel])
        r = R.Want(*[int(rec[f][i]) for f in ("n", "n_pos")], int(rec["n"][i] - rec["n_pos"][i] - rec["n_nan"][i]),
                   *[int(rec[f][i]) for f in ("n_nan", "auc2", "correct")], float(rec["objv"][i]), None)
        assert tuple(r[:6]) == tuple(want[:6]), (what, g, r, want)
        if np.isinf(want.objv):
            assert r.objv == want.objv, (what, g)
        else:
            assert abs(r.objv - want.objv) <= (want.n + 16) * 2.0 ** -52 * want.sum_abs, (what, g, r.objv, want.objv)
        if want.n_pos and want.n_neg:
            num += fractions.Fraction((want.n_pos + want.n_neg) * want.auc2, 2 * want.n_pos * want.n_neg)
            rows += want.n_pos + want.n_neg
            mixed += 1
    gauc = float(np.frombuffer(gauc_bits, np.float64)[0])
    print("%s: groups, mixed, rows_mixed, nogroup %s gauc_num %.17g want %.17g" % (what, got[0][:4], gauc, float(num)))
    assert (n_mixed, rows_mixed) == (mixed, rows), what
    assert abs(fractions.Fraction(gauc) - num) <= num * (len(ids) + 4) * fractions.Fraction(1, 2 ** 53), (what, gauc, float(num))


def rows_of(sizes, seed, values=None):
    """groups of the given sizes with ascending ids (so group i's rows follow group i - 1's in the sorted order), shuffled"""
    rng = np.random.default_rng(seed)
    gid = np.repeat(np.arange(len(sizes), dtype=np.uint64) * np.uint64(977) + np.uint64(3), sizes)
    n = gid.size
    pred = (rng.choice(values, n) if values is not None else np.round(rng.normal(size=n), 1)).astype(np.float32)
    label = (rng.random(n) < 1 / (1 + np.exp(-pred))).astype(np.float32)
    p = rng.permutation(n)
    return label[p], pred[p], gid[p]


def sizes_upto(n, rng, top):
    out = []
    while sum(out) < n:
        out.append(min(int(rng.integers(1, top)), n - sum(out)))
    return out


SHAPES = {
    "one group": [3 * T + 5],
    "every row its own": [1] * (T + 1),
    "sizes 1, 2, 3, ...": list(range(1, 111)) + [3 * T + 5 - 110 * 111 // 2],
    "border on a tile border": [T - 3, 3, T, 5],
    "one group over three tiles": [100, 2 * T + 500, 50],
}
SHAPES.update({"n = %d" % n: sizes_upto(n, np.random.default_rng(n), 40) for n in (1, T - 1, T, T + 1, 3 * T + 5)})


@pytest.mark.parametrize("values", [None, (-1.5, 0.25, 2.0)], ids=["scores", "three values"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_exact_fields(capi, ctx, shape, values):
    """three values: equal scores sit on both sides of most group borders, and tie groups cross the tile borders inside a group"""
    label, pred, gid = rows_of(SHAPES[shape], 7, values)
    got = run(capi, ctx, label, pred, gid)
    check(label, pred, gid, None, got, shape)
    if shape == "one group":
        rec, whole = got[1], got[2]
        assert [int(rec[f][0]) for f in ("n", "n_pos", "n_nan", "auc2", "correct")] == [whole.n, whole.n_pos, whole.n_nan, whole.auc2,
                                                                                          whole.correct]
    if shape == "every row its own":
        assert got[0][1:3] == (0, 0) and got[0][4] == np.float64(0).tobytes()


def special_rows():
    """NaN predictions in several groups and one all-NaN group, -0.0 against +0.0, the ids 0 and 2^64 - 1 beside rows without a
    group whose id fields hold those very values"""
    rng = np.random.default_rng(11)
    n = T + 700
    gid = rng.choice(np.array([0, 1, 4096, 2 ** 63, U64 - 1, U64], np.uint64), n)
    pred = rng.choice(np.array([-0.0, 0.0, np.nan, 1.0, -1.0, np.inf, -np.inf], np.float32), n)
    label = rng.integers(0, 2, n).astype(np.float32)
    pred[gid == np.uint64(4096)] = np.nan
    has = rng.random(n) < 0.8
    has[:2] = False
    gid[0], gid[1] = 0, U64
    return label, pred, gid, has.astype(np.uint8)


def test_nan_signed_zero_and_extreme_ids(capi, ctx):
    label, pred, gid, has = special_rows()
    got = run(capi, ctx, label, pred, gid, has)
    check(label, pred, gid, has, got, "special")
    rec = got[1]
    i = [int(g) for g in rec["gid"]].index(4096)
    assert rec["n"][i] == rec["n_nan"][i] > 0 and rec["auc2"][i] == 0 and rec["objv"][i] == 0
    assert int(rec["gid"][0]) == 0 and int(rec["gid"][-1]) == U64


def test_appends_and_the_whole_set(capi, ctx):
    """the same bits in every field however the rows were cut into appends; dfh_eval_finish as with grouping off"""
    label, pred, gid, has = special_rows()
    l2, p2, g2 = rows_of(sizes_upto(2 * T + 9 - len(label), np.random.default_rng(5), 300), 5)
    label, pred, gid = np.concatenate([label, l2]), np.concatenate([pred, p2]), np.concatenate([gid, g2 + np.uint64(7)])
    has = np.concatenate([has, np.ones(len(l2), np.uint8)])
    bits = lambda got: (got[0], [got[1][f].tobytes() for f in capi.Eval.GROUP_FIELDS], R.fields(got[2]))   # noqa: E731
    once = run(capi, ctx, label, pred, gid, has)
    check(label, pred, gid, has, once, "appends")
    for cut in (1, 7, T + 1):
        assert bits(run(capi, ctx, label, pred, gid, has, cut)) == bits(once), cut
    e = capi.Eval(ctx)
    e.append_host(label, pred)
    assert R.fields(e.finish()) == R.fields(once[2])
    e.close()


@pytest.mark.parametrize("slot", [0, 4095])
def test_groups_of_a_stepped_batch(capi, ctx, slot):
    """rows whose slot feature stands first, last, twice (the first wins) and nowhere; 70 rows of 1 .. 20 positions: more than one
    block of 32 rows, more than one round of a lane group's 8 lanes"""
    rng = np.random.default_rng(slot + 1)
    other = lambda k: (rng.integers(1, 2 ** 51, k).astype(np.uint64) << np.uint64(12)) | np.uint64(17 if slot != 17 else 18)   # noqa: E731
    user = lambda: (np.uint64(rng.integers(1, 6)) << np.uint64(50)) | np.uint64(slot)   # noqa: E731
    rows = []
    for r in range(70):
        ids = list(other(r % 20 + 1))
        for at in ((0,), (-1,), (len(ids) // 2, -1), ())[r % 4]:
            ids[at] = user()
        rows.append(ids)
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    idx = np.array([i for r in rows for i in r], np.uint64)
    lab = rng.integers(0, 2, len(rows)).astype(np.float32)
    tb = capi.Table(ctx, 1 << 12, V_dim=4, init_mode=capi.INIT_HASH, l1=0.01, l2=0.0, lr=0.1, V_lr=0.05, V_l2=0.01, V_threshold=0,
                    V_init_scale=0.5, seed=1)
    bt = capi.Batch(ctx, len(rows), idx.size)
    e = capi.Eval(ctx)
    e.group_by_slot(slot)
    bt.load_host(off, idx, None, lab)
    bt.localize()
    refused(capi, ERR_STATE, e.append_batch, bt)   # not stepped since its load
    bt.sgd_step(tb, is_train=False, push_cnt=False)
    e.append_batch(bt)
    e.append_batch(bt)   # (the same rows once more, behind the first ones: every count doubles)
    s = e.finish_groups()
    got = (summary(s), e.read_groups(0, s.n_groups), None)
    loc, pred = bt.get_localized(), bt.pred()
    ids = np.array([capi.reverse_bytes(loc["feaids"][j]) for j in loc["index"]], np.uint64)
    gid, has = np.zeros(len(rows), np.uint64), np.zeros(len(rows), np.uint8)
    for r in range(len(rows)):
        hit = [int(i) for i in ids[int(off[r]):int(off[r + 1])] if int(i) & 4095 == slot]
        assert hit == [int(i) for i in rows[r] if int(i) & 4095 == slot]
        if hit:
            gid[r], has[r] = hit[0], 1
    assert 0 < has.sum() < len(rows)
    check(np.tile(lab, 2), np.tile(pred, 2), np.tile(gid, 2), np.tile(has, 2), got, "batch, slot %d" % slot)
    for o in (e, bt, tb):
        o.close()


def test_refusals(capi, ctx):
    e = capi.Eval(ctx)
    one, gid = np.ones(1, np.float32), np.ones(1, np.uint64)
    refused(capi, ERR_ARG, e.group_by_slot, -2)
    refused(capi, ERR_ARG, e.group_by_slot, 4096)
    refused(capi, ERR_STATE, e.append_host_groups, one, one, gid)   # grouping is off
    e.append_host(one, one)
    refused(capi, ERR_STATE, e.group_by_slot, 3)                    # not empty
    e.reset()
    e.group_by_slot(3)
    refused(capi, ERR_STATE, e.append_host, one, one)               # these rows would have no groups
    e.append_host_groups(one, one, gid)
    e.reset()   # keeps the slot
    e.append_host_groups(one, one, gid)
    assert e.finish_groups().n_groups == 1
    refused(capi, ERR_ARG, e.read_groups, 1, 1)
    e.close()
