"""The oracle of the whole-set evaluator (csrc/dfh_eval.hip), in numpy and Python integers, and the pass criteria the
evaluator's tests share: integer fields equal, objv within (n + 16) 2^-52 of the sum of the terms' magnitudes (the device's and
numpy's fp64 exp / log1p are each within a couple of ulp of a term, a sum of n terms adds at most n ulp of that sum)."""
import collections

import numpy as np

Want = collections.namedtuple("Want", "n n_pos n_neg n_nan auc2 correct objv sum_abs")


def oracle(label, pred):
    label = np.asarray(label, np.float32)
    pred = np.asarray(pred, np.float32)
    assert label.shape == pred.shape and label.ndim == 1
    nan = np.isnan(pred)
    s = pred[~nan]
    with np.errstate(invalid="ignore"):
        pos = label[~nan] > 0          # a NaN label is negative
    neg = np.sort(s[~pos])             # (-0.0 and +0.0 compare equal; +-inf are ordinary values)
    sp = s[pos]
    auc2 = int(np.sum(np.searchsorted(neg, sp, "left"), dtype=object)) + int(np.sum(np.searchsorted(neg, sp, "right"), dtype=object))
    correct = int(np.count_nonzero((pos & (s > 0)) | (~pos & (s <= 0))))
    m = np.where(pos, s.astype(np.float64), -s.astype(np.float64))
    with np.errstate(over="ignore"):
        terms = np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))
    objv = float(np.sum(terms)) if terms.size else 0.0
    return Want(int(pred.size), int(pos.sum()), int((~pos).sum()), int(nan.sum()), auc2, correct, objv,
                float(np.sum(np.abs(terms))) if terms.size else 0.0)


def fields(r):
    """every field of a capi.EvalResult, objv as its bits"""
    return (r.n, r.n_pos, r.n_neg, r.n_nan, r.auc2, r.correct, np.float64(r.objv).tobytes())


def check(r, want, what=""):
    got = (r.n, r.n_pos, r.n_neg, r.n_nan, r.auc2, r.correct)
    print("%s got %s objv %.17g | want %s objv %.17g" % (what, got, r.objv, tuple(want[:6]), want.objv))
    assert got == tuple(want[:6]), what
    assert r.n == r.n_pos + r.n_neg + r.n_nan
    if np.isinf(want.objv):
        assert r.objv == want.objv, what
    else:
        bound = (want.n + 16) * 2.0 ** -52 * want.sum_abs
        assert abs(r.objv - want.objv) <= bound, (what, r.objv, want.objv, bound)
