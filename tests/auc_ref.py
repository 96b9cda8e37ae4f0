"""The integer oracle of the minibatch AUC (k_auc_pairs / k_auc_finalize, the AUC role of k_update_fused, and the radix form
k_auc_keys / k_auc_area in csrc/dfh_kernels.hip), the condition under which ONE miscounted pair changes the float the device
returns, and the designed cases tests/test_auc_exact.py runs.

The device counts area = the (positive j, negative i) pairs with (pred_j, j) before (pred_i, i) — -0 equals +0, ties by
index — as an integer, then does three IEEE double operations, a = area / (tp (n - tp)), 1 - a where a < 0.5, times n, adds
the result to a zeroed double and casts to float.  auc_times_n_f32 does the same in numpy, so a test compares with ==.

One pair moves a by 1 / (tp (n - tp)) and the result by n / (tp (n - tp)); a float near n resolves np.spacing(float32(n)).
visible(tp, n) asks for 4 of those per pair, which a minority class of at most 16 rows gives for every n up to 65 537.  The
fold 1 - a maps area and tp (n - tp) - area to the same float, so a case also keeps its area more than one pair away from
half of tp (n - tp): a count off by one never lands on its own mirror image.

NaN predictions are out of scope: BinClassMetric::AUC leaves their order to std::sort's comparator, which is not a strict
weak ordering with them, and the device's key image puts them wherever their sign bit says."""
import collections

import numpy as np

TILE_ROWS, TILE_COLS = 256, 1024      # a unit of auc_pairs_block: 256 rows against column tiles of 1 024
COL_SPLIT = 16                        # column tiles are dealt to min(tiles, 16) units per row tile
PAIRS_MAX_N = 32768                   # beyond: the radix form, one block walking 1 024 sorted rows per trip
MAX_MINORITY = 16

PAIR_SIZES = (255, 256, 257, 1023, 1024, 1025, 16384, 16385, 17409, 32767, 32768)
RADIX_SIZES = (32769, 33793, 65537)
STEP_SIZES = (257, 16385, 17409, 32768)
LAYOUTS = ("asc", "desc", "perm", "tied")

Case = collections.namedtuple("Case", "name label pred rows")   # rows: the minority class's rows, as designed


def area(label, pred):
    """the (positive j, negative i) pairs with (pred_j, j) before (pred_i, i), a Python integer"""
    pred = np.asarray(pred, np.float32) + np.float32(0)   # -0.0 -> +0.0: one value
    assert not np.isnan(pred).any()
    pos = np.asarray(label, np.float32) > 0
    order = np.lexsort((np.arange(pred.size), pred))
    sp = pos[order]
    return int(np.cumsum(sp, dtype=np.int64)[~sp].sum())


def auc_times_n_f32(area, tp, n):
    """what the device turns {area, positives, n} into: three double operations, then the cast to float"""
    return np.float32(auc_times_n_f64(area, tp, n))


def auc_times_n_f64(area, tp, n):
    """the double the device adds to its accumulator (several steps between two reads: the doubles add up, then the cast)"""
    if tp in (0, n):
        return np.float64(1.0)
    a = np.float64(area) / (np.float64(tp) * np.float64(n - tp))
    return (np.float64(1.0) - a if a < 0.5 else a) * np.float64(n)


def visible(tp, n):
    """one pair moves AUC x n by at least 4 float32 ulp of n"""
    return 0 < tp < n and n / (tp * (n - tp)) >= 4 * float(np.spacing(np.float32(n)))


def expect(label, pred):
    """the float the device must return for a designed case, after the two conditions that make one pair show in it"""
    label = np.asarray(label, np.float32)
    n, tp = label.size, int((label > 0).sum())
    assert min(tp, n - tp) <= MAX_MINORITY and visible(tp, n), (tp, n)
    ar = area(label, pred)
    assert abs(2 * ar - tp * (n - tp)) > 2, "area %d of %d: within one pair of the fold" % (ar, tp * (n - tp))
    return auc_times_n_f32(ar, tp, n)


# ------------------------------------------------------------------------------------------------------ designed cases
def scores(n, layout):
    """n scores, all different (multiples of 2^-12 below 20 in magnitude: exact as w x 1 in a step too) or all equal"""
    if layout == "tied":
        return np.full(n, 0.25, np.float32)
    k = np.arange(n)
    if layout == "desc":
        k = k[::-1]
    elif layout == "perm":
        k = np.random.default_rng(1000 + n).permutation(n)
    else:
        assert layout == "asc"
    return ((k - n // 2) / 4096).astype(np.float32)


def rounded_scores(rng, n):
    """multiples of 1/8: some sixty values, so every row ties with many others"""
    return (np.round(rng.normal(size=n) * 8) / 8).astype(np.float32)


def labels(n, rows, minority_pos):
    """the rows `rows` in one class, every other row in the other (negatives are 0 under a positive minority, -1 under a
    negative one: label > 0 is the rule)"""
    lab = np.full(n, 0.0 if minority_pos else 1.0, np.float32)
    lab[np.asarray(rows, np.int64)] = 1.0 if minority_pos else -1.0
    return lab


def probe_rows(n):
    return sorted({0, 255, 256, 1023, 1024, 16383, 16384, n - 1} & set(range(n)))


def sorted_positions(n):
    return [1023, 1024, 1025, 32768, n - 1]


def one_row(n, layout, row, minority_pos):
    """one row of the minority class.  Where that single row would leave the area within a pair of the fold (a row in the
    middle of a monotone or tied layout), row 1 joins it"""
    pred = scores(n, layout)
    rows = [row]
    if abs(2 * area(labels(n, rows, minority_pos), pred) - (n - 1)) <= 2:
        assert row != 1
        rows = [1, row]
    return Case("one %s at row %d of %d, %s" % ("positive" if minority_pos else "negative", row, n, layout),
                labels(n, rows, minority_pos), pred, rows)


def one_row_cases(n, minority_pos):
    return [one_row(n, layout, row, minority_pos) for layout in LAYOUTS for row in probe_rows(n)]


def row_at_sorted_position(n, layout, r):
    order = np.lexsort((np.arange(n), scores(n, layout)))
    return int(order[r])


def one_sorted_cases(n, minority_pos):
    """the radix form walks the SORTED rows: the minority row sits at sorted position r"""
    return [one_row(n, layout, row_at_sorted_position(n, layout, r), minority_pos)._replace(
        name="one %s at sorted position %d of %d, %s" % ("positive" if minority_pos else "negative", r, n, layout))
        for layout in LAYOUTS for r in sorted_positions(n)]


def seam_chunks(n, step):
    """the multiples of `step` inside (0, n), eight to a case: both sides of a seam are two rows, sixteen in all"""
    seams = list(range(step, n, step))
    return [seams[i:i + 8] for i in range(0, len(seams), 8)]


def seam_cases(n, minority_pos):
    """pair counting: the minority class sits on both sides of every multiple of 256 (row tiles; every fourth is a column
    tile's seam, every 64th a second trip's), scores rounded to 1/8"""
    out = []
    for c, seams in enumerate(seam_chunks(n, TILE_ROWS)):
        pred = rounded_scores(np.random.default_rng(7 * n + c), n)
        rows = [r for s in seams for r in (s - 1, s)]
        out.append(Case("%s on both sides of rows %s of %d" % ("positives" if minority_pos else "negatives", seams, n),
                        labels(n, rows, minority_pos), pred, rows))
    return out


def sorted_seam_cases(n, minority_pos):
    """the radix form: the minority class on both sides of every multiple of 1 024 of the SORTED order, scores rounded to 1/8"""
    out = []
    for c, seams in enumerate(seam_chunks(n, TILE_COLS)):
        pred = rounded_scores(np.random.default_rng(11 * n + c), n)
        order = np.lexsort((np.arange(n), pred))
        rows = [int(order[r]) for s in seams for r in (s - 1, s)]
        out.append(Case("%s on both sides of sorted positions %s of %d" % ("positives" if minority_pos else "negatives", seams, n),
                        labels(n, rows, minority_pos), pred, rows))
    return out


FLT_MAX = float(np.finfo(np.float32).max)
SPECIAL = np.array([np.inf, -np.inf, FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1e-40, -1e-40, 0.0, -0.0], np.float32)


def special_case(n, minority_pos):
    """every special score once in the minority class and twice in the other, among rounded scores (which hold zeros of
    both signs themselves): thirty random rows in ascending order, taken three at a time as (other class, minority, other
    class) with one score — but a zero of the minority sits between two zeros of the OTHER sign"""
    rng = np.random.default_rng(13 * n + int(minority_pos))
    pred = rounded_scores(rng, n)
    at = np.sort(rng.choice(n, size=3 * SPECIAL.size, replace=False)).reshape(-1, 3)
    v = SPECIAL[rng.permutation(SPECIAL.size)]
    rows = [int(r) for r in at[:, 1]]
    pred[at[:, 1]] = v
    pred[at[:, 0]] = pred[at[:, 2]] = np.where(v == 0, -v, v)
    return Case("special scores among %d rows, minority %s" % (n, "positive" if minority_pos else "negative"),
                labels(n, rows, minority_pos), pred, rows)


def boundary_case():
    """32 769 rows for the radix form; without the last row, 32 768 for pair counting"""
    n = PAIRS_MAX_N + 1
    rng = np.random.default_rng(99)
    pred = rounded_scores(rng, n)
    rows = sorted(int(r) for r in rng.choice(n - 1, size=15, replace=False)) + [n - 1]   # the row cut off is a positive
    return Case("16 positives among %d rows" % n, labels(n, rows, True), pred, rows)
