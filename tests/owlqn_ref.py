"""The yardstick of the l1 (orthant-wise L-BFGS, OWL-QN) tests of learner = lbfgs (tests/test_lbfgs_l1_kernels.py,
test_lbfgs_l1_learner.py, test_lbfgs_l1_sharded.py):

  Mirror       lbfgs_ref.Mirror with the rules of difacto_amd/csrc/dfh_owlqn.hip in float32 numpy, operation for operation:
               the pseudo-gradient, s = w - w0, the Add chain WITHOUT the x == 0 / x == 1 shortcuts, the alignment of p with
               the pseudo-gradient by strict signs, the trial w = w0 + alpha p and its projection, and the fp64 sums of
               float32 terms.  Like its base it is fed with the DEVICE's g_new, so its vectors are compared bit for bit.
  objective    F(w) = loss + r(w) + l1 |w|_1 and the smooth gradient in float64 on lbfgs_ref.Model
  fista        a float64 proximal-gradient solver (strongly convex FISTA) of the l1 + l2 logistic problem of the command-line
               tests, and read_libsvm, the dense float64 design of a small libsvm file
  sum_tol      the bound of a device scalar against the float64 sum of the mirror's float32 terms:
               2^-23 |value| + n 2^-52 sum |terms| (the float return, and the fp64 sum taken in another order)

Measured on an MI355X (FP32_GAP_MEASURED): the relative gap between F of the weights that example/rcv1_lbfgs_l1.conf saves
on the golden file (12 epochs, stopped by stop_rel_objv; F evaluated in float64) and the float64 optimum F*:
F = 50.973958198446 against F* = 50.973955492691, 5.308e-08 of F*, with the optimum's 279 of 2775 weights non-zero.  The
learner test asserts 10 x that, and never looser than 1e-4."""
import numpy as np

import lbfgs_ref as L

f32 = np.float32
FP32_GAP_MEASURED = 5.308e-8    # (F_fp32 - F*) / F*; see the docstring
F_STAR_RCV1 = 50.973955492691   # example/rcv1_lbfgs_l1.conf on tests/golden/rcv1_100.libsvm, float64 (fista below)


def sum_tol(value, n, mag):
    return 2.0 ** -23 * abs(value) + n * 2.0 ** -52 * mag


def _sum(terms):
    """float64 sum of float32 (or float64) terms -> (sum, sum |terms|)"""
    t = np.asarray(terms, np.float64)
    return float(t.sum()), float(np.abs(t).sum())


class Mirror(L.Mirror):
    def __init__(self, w, isV, l2, V_l2, m, l1):
        super().__init__(w, isV, l2, V_l2, m)
        self.isV = np.asarray(isV, bool)
        self.l1 = f32(l1)
        self.pg = self.w0 = None

    def pseudo(self, gp):
        a, b = gp + self.l1, gp - self.l1
        zero = np.where(a < 0, a, np.where(b > 0, b, f32(0)))
        pg = np.where(self.w > 0, a, np.where(self.w < 0, b, zero))
        return np.where(self.isV, gp, pg).astype(np.float32)

    def branches(self, gp):
        """which of the five pseudo-gradient branches each w element takes: 0 w > 0, 1 w < 0, 2 g' + l1 < 0, 3 g' - l1 > 0,
        4 the zero of the subdifferential; -1 on V elements"""
        a, b = gp + self.l1, gp - self.l1
        br = np.where(self.w > 0, 0, np.where(self.w < 0, 1, np.where(a < 0, 2, np.where(b > 0, 3, 4))))
        return np.where(self.isV, -1, br)

    def prepare(self, g_new):
        g_new = np.asarray(g_new, np.float32)
        gp = g_new + self.coef * self.w
        pg = self.pseudo(gp)
        self.gp_last = gp
        if self.g is None:
            self.g, self.pg = gp, pg
            return None
        if len(self.y) == self.m:
            self.y.pop(0)
        self.y.append(gp + f32(-1) * self.g)               # smooth gradients on both sides
        self.s[-1] = self.w - self.w0                      # the real displacement, always stored
        self.g, self.pg = gp, pg
        self.alpha = f32(0)
        k = len(self.y)
        assert len(self.s) == k
        out = [None] * (6 * k + 1)
        for r, a in enumerate((self.s[-1], self.y[-1], self.pg)):
            for i in range(k):
                out[i + 2 * r * k] = _sum(a * self.s[i])
                out[i + (2 * r + 1) * k] = _sum(a * self.y[i])
        out[6 * k] = _sum(self.pg * self.pg)
        return out

    def drop_last(self):
        self.s.pop()
        self.y.pop()

    def chain(self, d, every=1):
        if d is None:
            vecs, d = [self.pg], [f32(-1)]
        else:
            vecs, d = self.s + self.y + [self.pg], np.asarray(d, np.float32)
            assert len(d) == len(vecs)
        p = np.zeros_like(self.pg[::every])
        for c, v in zip(d, vecs):
            p = p + f32(c) * v[::every]                    # no shortcut: an exact 0 or 1 changes no bit
        return p

    def direction(self, d):
        """-> (<pg, p>, sum |products|) of the aligned p"""
        p = self.chain(d)
        self.clamped = float((np.abs(p) > f32(5)).mean())
        p = np.where(p > f32(5), f32(5), np.where(p < f32(-5), f32(-5), p)).astype(np.float32)
        keep = ((p > 0) & (self.pg < 0)) | ((p < 0) & (self.pg > 0))
        self.dropped = int((~keep & ~self.isV & (p != 0)).sum())
        p = np.where(self.isV | keep, p, f32(0)).astype(np.float32)
        if len(self.s) == self.m:
            self.s.pop(0)
        self.s.append(p)
        self.w0 = self.w.copy()
        self.alpha = f32(0)
        return _sum(self.pg * p)

    def line_search(self, alpha):
        """the trial from w0, projected -> the number of w elements the projection set to zero"""
        p, w0, pg = self.s[-1], self.w0, self.pg
        t = w0 + f32(alpha) * p
        pos = (w0 > 0) | (~(w0 < 0) & (pg < 0))
        neg = (w0 < 0) | (~(w0 > 0) & (pg > 0))
        keep = ((t > 0) & pos) | ((t < 0) & neg)
        self.projected = int((~keep & ~self.isV & (t != 0)).sum())
        self.w = np.where(self.isV | keep, t, f32(0)).astype(np.float32)
        self.alpha = f32(alpha)
        return self.projected

    def sums(self):
        """-> dict of (value, sum |terms|): r (with l1), armijo = sum pg (w - w0), and the counts nnz, moved"""
        c64, w64 = self.coef.astype(np.float64), self.w.astype(np.float64)
        r2 = _sum(0.5 * c64 * w64 * w64)
        r1 = _sum(np.abs(self.w[~self.isV]))
        l1 = float(self.l1)
        return dict(r=(r2[0] + l1 * r1[0], r2[1] + l1 * r1[1]),
                    armijo=_sum(self.pg * (self.w - self.w0)),
                    nnz=int(np.count_nonzero(self.w)), moved=int((self.w != self.w0).sum()))


def objective(M, w, l1):
    """F(w) = loss + r(w) + l1 sum |w| over the w elements, and the smooth gradient g + coef w, float64, on lbfgs_ref.Model"""
    loss, g = M.loss_grad(w)
    r, gr = M.reg(w)
    w = np.asarray(w, np.float64)
    return loss + r + l1 * np.abs(w[~M.isV]).sum(), g + gr


# ------------------------------------------------------------------------------------------------ the command-line problem

def read_libsvm(path):
    """-> (ids ascending [d] uint64, X [rows, d] float64 of the values as written, y in {-1, +1}).  The learner reads the
    values as float32; rounding them first moves F* of the golden file by 7.5e-10 of itself (50.973955454669), three
    orders below the tightest bound the tests may use"""
    rows, labs = [], []
    for line in open(path):
        t = line.split()
        if not t:
            continue
        labs.append(1.0 if float(t[0]) > 0 else -1.0)
        rows.append([(int(i), float(x)) for i, x in (kv.split(":") for kv in t[1:])])
    ids = np.array(sorted({i for r in rows for i, _ in r}), np.uint64)
    col = {int(i): j for j, i in enumerate(ids)}
    X = np.zeros((len(rows), len(ids)))
    for r, row in enumerate(rows):
        for i, x in row:
            X[r, col[i]] += x
    return ids, X, np.array(labs)


def logistic(X, y, w, l2):
    """-> (loss + .5 l2 |w|^2, its gradient)"""
    z = y * (X @ w)
    return np.logaddexp(0, -z).sum() + 0.5 * l2 * (w @ w), X.T @ (-y / (1.0 + np.exp(z))) + l2 * w


def fista(X, y, l1, l2, tol=1e-14, max_iter=100000):
    """min_w sum log(1 + exp(-y x w)) + .5 l2 |w|^2 + l1 |w|_1 by proximal gradient with the constant momentum of a strongly
    convex problem (mu = l2, L = sigma_max(X)^2 / 4 + l2), until an iteration moves no coordinate by more than tol
    -> (w*, F*, smooth gradient at w*)"""
    Lc = 0.25 * np.linalg.norm(X, 2) ** 2 + l2
    q = np.sqrt(l2 / Lc)
    beta = (1 - q) / (1 + q)
    w = v = np.zeros(X.shape[1])
    for _ in range(max_iter):
        _, g = logistic(X, y, v, l2)
        u = v - g / Lc
        wn = np.sign(u) * np.maximum(np.abs(u) - l1 / Lc, 0.0)
        step = np.abs(wn - w).max()
        v = wn + beta * (wn - w)
        w = wn
        if step <= tol:
            break
    else:
        raise AssertionError("fista did not converge")
    f, g = logistic(X, y, w, l2)
    return w, f + l1 * np.abs(w).sum(), g
