"""The minibatch AUC, every counted pair: pair counting (auc_pairs_block as k_auc_pairs and as a role of k_update_fused,
k_auc_finalize) up to 32 768 rows and the radix form (k_auc_keys, rocPRIM's stable sort, k_auc_area) beyond, against the
integer oracle of tests/auc_ref.py.  Every case keeps one class at 16 rows or fewer, so that one miscounted pair moves the
float the device returns by several ulp (auc_ref.visible), and every comparison is ==.

Sizes: 255 .. 257 around a row tile, 1 023 .. 1 025 around a column tile, 16 384 the last size with one column tile per unit
and 16 385 the first with a second trip of the tile loop, 17 409 = 17 x 1 024 + 1 (18 tiles: two units of a row tile take two
tiles, the last tile holds one row), 32 767 and 32 768 the largest; 32 769, 33 793 = 33 x 1 024 + 1 and 65 537 for the block
that walks the sorted rows 1 024 at a time with a carry.

NaN predictions are out of scope: the reference sorts with a comparator that is no strict weak ordering once a NaN is
present (bin_class_metric.h:43), so their place is unspecified there."""
import numpy as np
import pytest

import auc_ref as A

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the oracle itself, CPU
def area_by_pairs(label, pred):
    n, cnt = len(pred), 0
    for j in range(n):
        if not label[j] > 0:
            continue
        for i in range(n):
            if not label[i] > 0 and (pred[j] < pred[i] or (pred[j] == pred[i] and j < i)):
                cnt += 1
    return cnt


@pytest.mark.parametrize("n", [1, 2, 3, 17, 100, 300])
def test_area_against_the_double_loop(n):
    rng = np.random.default_rng(n)
    for rep in range(3):
        pred = (np.round(rng.normal(size=n) * 3) / 4).astype(np.float32)   # some ten values; -0.0 among them
        pred[rng.random(n) < 0.1] = -0.0
        lab = rng.choice(np.array([-1, 0, 1, 2], np.float32), size=n)
        assert A.area(lab, pred) == area_by_pairs(lab, pred)
    both = np.array([0.0, -0.0, -0.0, 0.0], np.float32)
    assert A.area([1, 0, 1, 0], both) == 3 and A.area([0, 1, 0, 1], both) == 1


def test_float_of_an_area():
    assert A.auc_times_n_f32(0, 0, 5) == 1.0 and A.auc_times_n_f32(0, 5, 5) == 1.0
    assert A.auc_times_n_f32(6, 2, 5) == 5.0 and A.auc_times_n_f32(0, 2, 5) == 5.0   # the fold
    assert A.auc_times_n_f32(3, 2, 5) == 2.5 and A.auc_times_n_f32(4, 2, 5) == np.float32(4 / 6 * 5)


def test_visible_against_brute_force():
    """where visible holds, neighbouring areas on one side of the fold give different floats — over the whole range for small
    n, on a sample of areas (the ends, the fold, random ones) for the sizes the tests use"""
    for n in (2, 3, 5, 64, 255):
        for tp in range(1, min(n, 17)):
            if A.visible(tp, n):
                f = [A.auc_times_n_f32(a, tp, n) for a in range((tp * (n - tp) + 1) // 2, tp * (n - tp) + 1)]
                assert all(x < y for x, y in zip(f, f[1:])), (tp, n)
    rng = np.random.default_rng(0)
    for n in A.PAIR_SIZES + A.RADIX_SIZES + (70000,):
        for tp in (1, 2, 15, 16, n - 16, n - 1):
            assert A.visible(tp, n), (tp, n)
            tot = tp * (n - tp)
            sample = set(int(a) for a in rng.integers(0, tot, 200)) | {0, 1, tot - 1, tot // 2 - 2, tot // 2 + 1}
            for a in sample:
                if a + 1 <= tot // 2 - 1 or a >= (tot + 1) // 2:   # both of a, a + 1 below the fold, or both at or above it
                    assert A.auc_times_n_f32(a, tp, n) != A.auc_times_n_f32(a + 1, tp, n), (a, tp, n)
    assert not A.visible(3000, 10000) and not A.visible(0, 10) and not A.visible(10, 10)


def minority_rows(case):
    pos = case.label > 0
    return np.flatnonzero(pos if pos.sum() * 2 < pos.size else ~pos)


def claims_hold(case):
    """the minority class is the rows the case names, at most 16, and one pair shows in the float"""
    assert case.label.size == case.pred.size and case.label.dtype == case.pred.dtype == np.float32
    assert sorted(case.rows) == list(minority_rows(case)) and 0 < len(case.rows) <= A.MAX_MINORITY, case.name
    A.expect(case.label, case.pred)


@pytest.mark.parametrize("n", A.PAIR_SIZES)
def test_designed_cases_of_pair_counting(n):
    for pos in (True, False):
        one = A.one_row_cases(n, pos)
        assert len(one) == 4 * len(A.probe_rows(n))
        for layout in A.LAYOUTS:
            got = [c.rows[-1] for c in one if c.name.endswith(layout)]
            assert got == A.probe_rows(n) and got[-1] == n - 1
        for c in one:
            claims_hold(c)
            assert len(c.rows) == 1 or (c.rows[0] == 1 and n >= 32767 and c.rows[1] in (16383, 16384)), c.name
            s = A.scores(n, c.name.split()[-1])
            assert np.array_equal(c.pred, s) and np.unique(s).size == (1 if c.name.endswith("tied") else n)
        # tie by index: one positive at row j of equal scores is in front of the n - 1 - j negatives behind it
        for j in A.probe_rows(n):
            assert A.area(A.labels(n, [j], True), A.scores(n, "tied")) == n - 1 - j
            assert A.area(A.labels(n, [j], False), A.scores(n, "tied")) == j
        seams = A.seam_cases(n, pos)
        covered = set()
        for c in seams:
            claims_hold(c)
            assert np.array_equal(c.pred * 8, np.round(c.pred * 8)) and np.unique(c.pred).size < 80
            covered |= set(c.rows)
        assert covered == {r for s in range(256, n, 256) for r in (s - 1, s)}
        assert len(seams) == (((n - 1) // 256) + 7) // 8
        sp = A.special_case(n, pos)
        claims_hold(sp)
        for v in A.SPECIAL:   # every special score under both labels (the bits: -0.0 is not +0.0 here)
            at = np.flatnonzero(sp.pred.view(np.uint32) == v.view(np.uint32))
            assert len(set(at) & set(sp.rows)) == 1 and len(set(at) - set(sp.rows)) >= 2, v
        # a zero of either sign in one class has zeros of the other sign, in the other class, on both sides of it
        zeros = np.flatnonzero(sp.pred == 0)
        for r in (r for r in sp.rows if sp.pred[r] == 0):
            other = [z for z in zeros if z not in sp.rows and np.signbit(sp.pred[z]) != np.signbit(sp.pred[r])]
            assert min(other) < r < max(other)
    # the tile loop: a unit takes a second trip from 16 385 rows on; at 17 409 two units of sixteen do, and the last tile holds one row
    tiles = -(-n // A.TILE_COLS)
    assert (tiles > A.COL_SPLIT) == (n > 16384)
    if n == 17409:
        assert tiles == 18 and tiles - A.COL_SPLIT == 2 and n - 17 * A.TILE_COLS == 1


@pytest.mark.parametrize("n", A.RADIX_SIZES)
def test_designed_cases_of_the_radix_form(n):
    assert n > A.PAIRS_MAX_N
    for pos in (True, False):
        one = A.one_sorted_cases(n, pos)
        assert len(one) == 4 * 5
        for c in one:
            claims_hold(c)
            r = int(c.name.split("sorted position ")[1].split()[0])
            order = np.lexsort((np.arange(n), c.pred))
            assert order[r] == c.rows[-1] and r in (1023, 1024, 1025, 32768, n - 1)
            assert len(c.rows) == 1 or (n == 65537 and r == 32768 and c.rows[0] == 1), c.name
        covered = set()
        for c in A.sorted_seam_cases(n, pos):
            claims_hold(c)
            order = np.lexsort((np.arange(n), c.pred))
            where = np.empty(n, np.int64)
            where[order] = np.arange(n)
            covered |= set(int(w) for w in where[c.rows])
        assert covered == {r for s in range(1024, n, 1024) for r in (s - 1, s)}
    b = A.boundary_case()
    claims_hold(b)
    assert b.label.size == A.PAIRS_MAX_N + 1 and b.label[-1] > 0
    assert A.expect(b.label[:-1], b.pred[:-1]) != A.expect(b.label, b.pred)


# ------------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def run_direct(ctx, cases):
    """every case through dfh_auc_times_n; all the figures are printed, then every one must be equal"""
    bad = []
    for c in cases:
        want = A.expect(c.label, c.pred)
        got = np.float32(ctx.auc_times_n(c.label, c.pred))
        print("%s: got %.9g want %.9g" % (c.name, got, want))
        if got != want:
            bad.append((c.name, float(got), float(want)))
    assert not bad, bad
    assert cases


@gpu
@pytest.mark.parametrize("minority_pos", [True, False], ids=["one_positive", "one_negative"])
@pytest.mark.parametrize("n", A.PAIR_SIZES)
def test_pairs_one_row_against_the_rest(ctx, n, minority_pos):
    """one positive among negatives: every column tile but one compacts to nothing; one negative among positives: every
    column tile is full.  At rows on both sides of the row tile, the column tile and the second trip, scores ascending,
    descending, permuted and all equal (ties by index)"""
    run_direct(ctx, A.one_row_cases(n, minority_pos))


@gpu
@pytest.mark.parametrize("minority_pos", [True, False], ids=["positives", "negatives"])
@pytest.mark.parametrize("n", [n for n in A.PAIR_SIZES if n > A.TILE_ROWS])   # 255 and 256 rows are one row tile: no seam
def test_pairs_minority_on_both_sides_of_every_seam(ctx, n, minority_pos):
    """up to 16 rows of one class on both sides of eight multiples of 256 per case, every multiple in some case, among scores
    rounded to 1/8: ties across every row-tile, column-tile and second-trip seam"""
    run_direct(ctx, A.seam_cases(n, minority_pos))


@gpu
@pytest.mark.parametrize("minority_pos", [True, False], ids=["positives", "negatives"])
@pytest.mark.parametrize("n", A.PAIR_SIZES + A.RADIX_SIZES)
def test_special_scores(ctx, n, minority_pos):
    """+-inf, +-FLT_MAX, denormals of both signs, -0.0 against +0.0, each under both labels"""
    run_direct(ctx, [A.special_case(n, minority_pos)])


@gpu
@pytest.mark.parametrize("minority_pos", [True, False], ids=["one_positive", "one_negative"])
@pytest.mark.parametrize("n", A.RADIX_SIZES)
def test_radix_one_row_against_the_rest(ctx, n, minority_pos):
    """the minority row at sorted positions 1 023, 1 024, 1 025, 32 768 and n - 1: on both sides of the block's first trip,
    and behind 32 trips' carry; all scores equal: the sort is stable, so the order is the index's"""
    run_direct(ctx, A.one_sorted_cases(n, minority_pos))


@gpu
@pytest.mark.parametrize("minority_pos", [True, False], ids=["positives", "negatives"])
@pytest.mark.parametrize("n", A.RADIX_SIZES)
def test_radix_minority_on_both_sides_of_every_seam(ctx, n, minority_pos):
    run_direct(ctx, A.sorted_seam_cases(n, minority_pos))


@gpu
def test_each_form_is_exact_at_its_side_of_the_boundary(ctx):
    """one data set of 32 769 rows (radix form) and the same without its last row (pair counting)"""
    b = A.boundary_case()
    run_direct(ctx, [b, b._replace(name=b.name + " less the last", label=b.label[:-1].copy(), pred=b.pred[:-1].copy(), rows=b.rows[:-1])])


# ------------------------------------------------------------------------------------------------------------- in a step
def step_cases(n):
    """(regime, cases): the cases of a regime share their scores, so one imported model serves them"""
    pick = lambda cases, layout: [c for c in cases if c.name.endswith(layout)]
    if n > A.PAIRS_MAX_N:
        one = {pos: A.one_sorted_cases(n, pos) for pos in (True, False)}
        seams = {pos: A.sorted_seam_cases(n, pos)[-1:] for pos in (True, False)}
    else:
        one = {pos: A.one_row_cases(n, pos) for pos in (True, False)}
        seams = {pos: A.seam_cases(n, pos)[-1:] for pos in (True, False)}
    out = [("tied", pick(one[True], "tied") + pick(one[False], "tied")),
           ("distinct", pick(one[True], "perm") + pick(one[False], "perm")),
           ("distinct", pick(one[True], "asc")[-3:] + pick(one[False], "desc")[-3:])]
    out += [("seam ties", seams[True]), ("seam ties", seams[False])]
    return out


def regime_is_there(regime, pred, case):
    n = pred.size
    if regime == "tied":
        assert np.unique(pred).size == 1
    elif regime == "distinct":
        assert np.unique(pred).size == n
    else:   # multiples of 1/8; three in four minority rows tie with rows of the other class, and some of those ties cross a row tile's seam
        assert np.array_equal(pred * 8, np.round(pred * 8))
        other = np.ones(n, bool)
        other[case.rows] = False
        tied = {r: np.flatnonzero(other & (pred == pred[r])) for r in case.rows}
        assert 4 * sum(t.size >= 2 for t in tied.values()) >= 3 * len(tied), case.name   # (scores in the far tails stand alone)
        assert any((t // A.TILE_ROWS != r // A.TILE_ROWS).any() for r, t in tied.items()), case.name


def run_steps(capi, n, is_train, auc_in_update):
    """one feature per row, key i + 1 in row i with value 1, V_dim 0: a row's score is the w of its key.  The expected float
    comes from the predictions read back and the case's labels"""
    ctx = capi.Context(0)
    ctx.set_option("auc_in_update", auc_in_update)
    kw = dict(l1=0.0, l2=0.0, lr=0.1, V_threshold=0, seed=1)
    off, idx, val = np.arange(n + 1, dtype=np.uint64), np.arange(1, n + 1, dtype=np.uint64), np.ones(n, np.float32)
    bt = capi.Batch(ctx, n, n)
    bt.set_option("compute_auc", 1)
    bad, steps, tb = [], 0, None
    for regime, cases in step_cases(n):
        for ci, c in enumerate(cases):
            bt.load_host(off, idx, val, c.label)
            bt.localize()
            fresh = regime == "tied" and ci == 0   # a fresh table: every score is 0 at its first step
            if ci == 0:
                if tb is not None:
                    tb.close()
                tb = capi.Table(ctx, 1 << 17, V_dim=0, **kw)
            if not fresh:   # the case's scores as the model (a training step moves w: imported again before every step)
                loc = bt.get_localized()
                assert loc["U"] == n
                w = np.empty(n, np.float32)
                w[loc["index"]] = c.pred   # row i holds the one occurrence of feaids[index[i]]
                scal = np.zeros((n, 4), np.float32)
                scal[:, 1] = w
                tb.import_(loc["feaids"], scal, np.zeros(n, np.int32))
            bt.sgd_step(tb, is_train=is_train, push_cnt=False)
            pred = bt.pred()
            prog = bt.progress(reset=True)
            regime_is_there(regime, pred, c)
            if not fresh:
                assert np.array_equal(pred, c.pred), c.name
            want = A.expect(c.label, pred)
            got = np.float32(prog.auc)
            print("%s [%s]: got %.9g want %.9g" % (c.name, regime, got, want))
            if got != want:
                bad.append((c.name, regime, float(got), float(want)))
            steps += 1
    for o in (bt, tb):
        o.close()
    ctx.close()
    assert not bad, bad
    assert steps >= 20


@gpu
@pytest.mark.parametrize("placement", ["train_in_update", "validation_own_launch"])
@pytest.mark.parametrize("n", A.STEP_SIZES)
def test_pairs_in_a_step(capi, n, placement):
    """dfh_sgd_step with compute_auc = 1: a training step whose AUC units are the first blocks of k_update_fused
    (auc_in_update = 1), and a validation step with auc_in_update = 0, where k_auc_pairs is a launch of its own.  One step
    feeds one float: the progress is reset after each.  (-0.0 does not survive the forward's 0 + w x: the direct call has it)"""
    if placement == "train_in_update":
        run_steps(capi, n, is_train=True, auc_in_update=1)
    else:
        run_steps(capi, n, is_train=False, auc_in_update=0)


@gpu
def test_radix_in_a_validation_step(capi):
    run_steps(capi, A.PAIRS_MAX_N + 1, is_train=False, auc_in_update=1)
