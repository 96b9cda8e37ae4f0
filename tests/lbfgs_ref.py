"""The yardstick of the dfh_lbfgs object's kernel-level tests (tests/test_lbfgs_state.py, test_lbfgs_gradient.py,
test_lbfgs_ring.py), in one place:

  Model     the reference's model and gradient pass in float64 over several training and validation chunks: keys =
            ReverseBytes(id) ascending, the merged float counts, RemoveTailFeatures (cnt > tail_feature_filter), lens
            (cnt > V_threshold), FMLoss::Predict / Evaluate / CalcGrad per chunk on scipy sparse designs
            (oracle.tolerance.Design) summed into the ragged layout, and the per-element tolerance of the comparison.
  Mirror    LBFGSUpdater's vector algebra in float32 with exactly the kernels' operation order (the kernels are compiled
            with fp contract(off)): PrepareCalcDirection, the s / y drop-oldest rule, CalcDirection's Add chain,
            LineSearch's step, r(w), <grad r, p>, nnz and lbfgs::Inner.  Its gradient input is the DEVICE's g_new
            (Lbfgs.vector(0)), so it carries no fp32 gradient noise and its vectors are compared bit for bit.
  designed_case / big_case   chunks built by rule; census() proves the rule on the reference's own model, on the CPU.
  draw_coefficients / ALPHAS the coefficients and line-search steps the ring test drives the object with.

The gradient pass is deterministic (no float atomics: a key occurs once per chunk, chunks run in order on one stream), so
a second pass must give the same bits.

Worst err / tol of the element-wise gradient comparison over the nine cases of tests/test_lbfgs_gradient.py, measured on
an MI355X: 0.350 (V_dim = 0, stride 4; 0.149 at the grid cap, 0.014 .. 0.145 at the other strides; GRAD_WORST_MEASURED
below; the test prints the value of its own run with -s).  No sqrt(n) of the floor had to be replaced by its strict n."""
import numpy as np

from oracle import tolerance as T

from bcd_ref import reverse_bytes_np

f32 = np.float32
GRAD_WORST_MEASURED = 0.350


# ------------------------------------------------------------------------------------------------ the model, float64

class _Chunk:
    """a chunk localized as Localizer(-1) does (keys = ReverseBytes(id) ascending) with its float64 design"""

    def __init__(self, off, ids, val, lab):
        self.off = np.asarray(off, np.int64)
        self.n = len(self.off) - 1
        self.lab = np.asarray(lab, np.float32)
        self.y = np.where(self.lab > 0, 1.0, -1.0)
        rk = reverse_bytes_np(np.asarray(ids, np.uint64))
        self.keys, self.col = np.unique(rk, return_inverse=True)
        self.U = len(self.keys)
        self.cnt = np.bincount(self.col, minlength=self.U).astype(np.float32)
        self.val = None if val is None else np.asarray(val, np.float32)
        self.D = T.Design(self.off, self.col, self.val, self.U)


class Model:
    """LBFGSUpdater::InitWeight's model of the training chunks [(offset, raw ids, value or None, label)] and the
    gradient pass over them in float64.  Nothing here comes from the device."""

    def __init__(self, train, val=(), V_dim=0, V_threshold=0, tail_feature_filter=0, l2=0.0, V_l2=0.0):
        self.k, self.l2, self.V_l2 = V_dim, l2, V_l2
        self.tr, self.va = [_Chunk(*c) for c in train], [_Chunk(*c) for c in val]
        uk, inv = np.unique(np.concatenate([c.keys for c in self.tr]), return_inverse=True)
        tot = np.zeros(len(uk), np.float32)
        np.add.at(tot, inv, np.concatenate([c.cnt for c in self.tr]))      # KVUnion of the chunks' float counts
        keep = tot > f32(tail_feature_filter) if tail_feature_filter > 0 else np.ones(len(uk), bool)
        self.keys, self.cnt = uk[keep], tot[keep]
        K = len(self.keys)
        self.hasV = (self.cnt > f32(V_threshold)) if V_dim else np.zeros(K, bool)
        self.lens = (1 + np.where(self.hasV, V_dim, 0)).astype(np.int32)
        self.pos = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.n = int(self.pos[-1])
        self.isV = np.ones(self.n, bool)
        self.isV[self.pos[:-1]] = False
        for c in self.tr + self.va:
            gp = np.searchsorted(self.keys, c.keys)
            hit = (gp < K) & (self.keys[np.minimum(gp, max(K - 1, 0))] == c.keys) if K else np.zeros(c.U, bool)
            c.map = np.where(hit, gp, -1)                  # TileBuilder::BuildColmap: -1 = not in the model

    # ---- layouts
    def split(self, w):
        """ragged -> W [K], V [K, k] (zero rows without V) in float64"""
        w = np.asarray(w, np.float64)
        W = w[self.pos[:-1]]
        V = np.zeros((len(self.keys), self.k))
        if self.k and self.hasV.any():
            V[self.hasV] = w[(self.pos[:-1][self.hasV] + 1)[:, None] + np.arange(self.k)[None, :]]
        return W, V

    def chunk_rows(self, c, W, V):
        """the chunk's packed rows as k_lb_gather builds them: w, V, has_V per chunk key, zero where map = -1"""
        m = np.maximum(c.map, 0)
        inm = c.map >= 0
        return np.where(inm, W[m], 0.0), np.where(inm[:, None], V[m], 0.0), inm & self.hasV[m]

    # ---- FMLoss
    def logits(self, w, chunks=None):
        """per chunk: float64 FMLoss::Predict (clamped iff V_dim > 0) and predict_bound's floor per row"""
        W, V = self.split(w)
        out = []
        for c in (self.tr if chunks is None else chunks):
            wc, Vc, _ = self.chunk_rows(c, W, V)
            out.append(T.predict_bound(c.D, wc, Vc))
        return out

    def grad(self, w):
        """the gradient pass at the ragged weights w -> dict:
          loss, loss_floor   sum over rows of log(1 + exp(-y f)); sum over rows of the logits' floors (|dl/df| <= 1)
          g, floor           float64 sum over the chunks of FMLoss::CalcGrad in the ragged layout; the comparison floor
          mag                sum of |terms| behind every element (0: the element must be an exact zero)
          touched            elements that some chunk's scatter adds to
          contrib            per chunk: its ragged contribution (zero where it has none)
          pred               per chunk: (float64 logits, their floors)
          raw                per chunk: (gw [U], gV [U, k]) by chunk key, the keys that are not in the model included
        floor = sum over the chunks of calcgrad_bound's floors on that chunk's float64 logits, plus two terms that
        calcgrad_bound has no slot for because it is handed the logits:
          (a) the logit's own floor carried through p = -y / (1 + exp(y f)): |dp/df| = s (1 - s) <= 1/4 (s the sigmoid), so
              |delta p| <= floor_f / 4 per row.  gw = X^T p moves by at most A^T (floor_f / 4); gV = X^T (p o XV) - V o
              (X2^T p) by at most A^T (|XV| o floor_f / 4) + |V| o X2^T (floor_f / 4)   (A = |X|, X2 = X.^2).
          (b) the chunks' contributions are added into g one after the other in float: every add rounds a partial sum
              whose magnitude is at most sum_c |contribution_c|; the roundings of the (chunks - 1) adds taken as one
              rounding of that magnitude, 2^-24 sum_c |contribution_c| (zero for an element that one chunk alone writes
              would be exact; the term keeps the sum form for every element).
        RTOL and C_SIGMA are oracle.tolerance's; no other factor appears."""
        W, V = self.split(w)
        g, floor, mag, cabs = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        touched = np.zeros(self.n, bool)
        loss, loss_floor, contrib, preds, raws = 0.0, 0.0, [], [], []
        for c in self.tr:
            wc, Vc, has = self.chunk_rows(c, W, V)
            f, ff = T.predict_bound(c.D, wc, Vc)
            preds.append((f, ff))
            loss += np.logaddexp(0, -c.y * f).sum()
            loss_floor += ff.sum()
            gw, gV, fw, fV = T.calcgrad_bound(c.D, c.lab, f, wc, Vc, has)
            raws.append((gw, gV))
            D = c.D
            qa = 0.25 * ff                                                     # (a)
            fw = fw + D.AT @ qa
            ap = np.abs(-c.y / (1.0 + np.exp(c.y * f)))
            mw = D.AT @ ap
            if self.k:
                XV = D.X @ Vc
                fV = fV + D.AT @ (np.abs(XV) * qa[:, None]) + np.abs(Vc) * (D.X2T @ qa)[:, None]
                mV = D.AT @ (np.abs(XV) * ap[:, None]) + np.abs(Vc) * (D.X2T @ ap)[:, None]
            else:
                mV = np.zeros((c.U, 0))
            inm = c.map >= 0
            sel = c.map[inm]
            full = lambda a, b: self._scatter(sel, a[inm], b[inm])   # noqa: E731
            cg = full(gw, gV)
            contrib.append(cg)
            g += cg
            cabs += np.abs(cg)
            floor += full(fw, fV)
            mag += full(mw, mV)
            t = np.zeros(len(self.keys), bool)
            t[sel] = True
            touched |= np.repeat(t, self.lens)
        floor += T.U32 * cabs                                                  # (b)
        return dict(loss=loss, loss_floor=loss_floor, g=g, floor=floor, mag=mag, touched=touched, contrib=contrib,
                    pred=preds, raw=raws)

    def _scatter(self, sel, aw, aV):
        """k_lb_scatter: chunk-key quantities (w part [u], V part [u, k]) of the keys at model positions sel -> ragged;
        a key without V takes no V part"""
        out = np.zeros(self.n)
        out[self.pos[:-1][sel]] = aw
        if self.k:
            hv = self.hasV[sel]
            out[(self.pos[:-1][sel[hv]] + 1)[:, None] + np.arange(self.k)[None, :]] = aV[hv]
        return out

    def loss_grad(self, w):
        r = self.grad(w)
        return r["loss"], r["g"]

    def reg(self, w):
        """r(w) = sum .5 coef w^2 and its gradient, float64"""
        c = np.where(self.isV, self.V_l2, self.l2)
        w = np.asarray(w, np.float64)
        return 0.5 * (c * w ** 2).sum(), c * w


def check_gradient(got, R, what="g_new"):
    """the one comparison of a device gradient with Model.grad's result R: |got - ref| <= RTOL |ref| + floor per element;
    bit-equal 0.0 where no chunk touches the element (the gradient is memset before the chunks add to it); equal to zero
    where every term is zero.  -> the worst err / tol"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == R["g"].shape, \
        "%s: %s %r against the model's %r" % (what, got.dtype, got.shape, R["g"].shape)
    un = ~R["touched"]
    assert not got[un].view(np.uint32).any(), "%s: an element no chunk touches is not 0.0" % what
    z = R["mag"] == 0
    assert not (got[z] != 0).any(), "%s: non-zero where every term is zero" % what
    return T.check(got, R["g"], R["floor"], what)


# ------------------------------------------------------------------------------------------------ the history, float32

def inner(a, b):
    """lbfgs::Inner: float32 products summed in float64 -> (sum, sum of |products|)"""
    p = a * b
    v = float(p.sum(dtype=np.float64))
    return v, float(np.abs(p, out=p).sum(dtype=np.float64))


def inner_tol(want, mag):
    """a float result of an fp64-summed product: its rounding to float plus the fp64 summation bound of
    tests/test_lbfgs_kernels.py"""
    return 2.0 ** -24 * abs(want) + 1e-10 * mag


class Mirror:
    """LBFGSUpdater (lbfgs_updater.h:86-203) in float32 numpy, operation for operation as dfh_lbfgs.hip's kernels"""

    def __init__(self, w, isV, l2, V_l2, m):
        self.w = np.array(w, np.float32)
        self.coef = np.where(isV, f32(V_l2), f32(l2)).astype(np.float32)
        self.m, self.s, self.y, self.g, self.alpha = m, [], [], None, f32(0)

    def prepare(self, g_new):
        """PrepareCalcDirection + CalcIncreB -> [(want, sum |products|)] in incr_B's order, None at epoch 0"""
        g_new = np.asarray(g_new, np.float32)
        gp = g_new + self.coef * self.w                    # AddRegularizerGrad: the product rounds, then the sum
        if self.g is None:
            self.g = gp
            return None
        if len(self.y) == self.m:
            self.y.pop(0)
        self.y.append(gp + f32(-1) * self.g)               # y = g; Add(-1, g_old, &y)
        if self.alpha != f32(1):
            self.s[-1] = self.s[-1] * self.alpha           # Times(alpha, &s.back())
        self.g = gp
        self.alpha = f32(0)
        k = len(self.y)
        assert len(self.s) == k
        out = [None] * (6 * k + 1)                         # Twoloop::CalcIncreB's order (lbfgs_twoloop.h:25-37)
        for r, a in enumerate((self.s[-1], self.y[-1], self.g)):
            for i in range(k):
                out[i + 2 * r * k] = inner(a, self.s[i])
                out[i + (2 * r + 1) * k] = inner(a, self.y[i])
        out[6 * k] = inner(self.g, self.g)
        return out

    def chain(self, d, every=1):
        """CalcDirection's Add chain before the clamp (d = None: -g); every: on each every-th element only"""
        if d is None:
            vecs, d = [self.g], [f32(-1)]
        else:
            vecs, d = self.s + self.y + [self.g], np.asarray(d, np.float32)
            assert len(d) == len(vecs)
        p = np.zeros_like(self.g[::every])
        for c, v in zip(d, vecs):
            if c == 0:
                continue
            p = p + v[::every] if c == 1 else p + f32(c) * v[::every]
        return p

    def direction(self, d):
        """CalcDirection -> (<g, p>, sum |products|); the new s goes last, the oldest leaves a full ring;
        self.clamped: the share of the direction that the clamp to +-5 changed"""
        p = self.chain(d)
        self.clamped = float((np.abs(p) > f32(5)).mean())
        p = np.where(p > f32(5), f32(5), np.where(p < f32(-5), f32(-5), p)).astype(np.float32)
        if len(self.s) == self.m:
            self.s.pop(0)
        self.s.append(p)
        self.alpha = f32(0)
        return inner(self.g, p)

    def line_search(self, alpha):
        """LineSearch's step on w (Add(alpha - alpha_, p, &w)) -> the float32 x it used"""
        x = f32(alpha) - self.alpha
        p = self.s[-1]
        if x != 0:
            self.w = self.w + p if x == 1 else self.w + x * p
        self.alpha = f32(alpha)
        return x

    def reg(self):
        """-> r(w) in float64 (.5 coef w w), (<grad r(w), p>, sum |products|) with float products, nnz(w)"""
        c64, w64 = self.coef.astype(np.float64), self.w.astype(np.float64)
        r = float((0.5 * c64 * w64 * w64).sum())
        return r, inner(self.coef * self.w, self.s[-1]), int(np.count_nonzero(self.w))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ designed data

BWD_CLASSES = (1, 2, 8, 9, 64, 65)     # both sides of k_backward_all's BWD_SMALL = 8 and BWD_MID = 64; plus one key >= 200


def per_wave(V_dim):
    """keys side by side in a wave of k_lb_gather / k_lb_scatter: 64 >> shift, 1 << shift the row stride (4 + V_dim rounded
    up to a multiple of 4) rounded up to a power of two, at most 64"""
    stride = 4 + (V_dim + 3) // 4 * 4
    shift = 0
    while (1 << shift) < stride and shift < 6:
        shift += 1
    return 64 >> shift, stride


def _csr(nrows, rows, keys, vals, order_rng):
    """entries (row, key, value) -> (offset, raw ids, values); a row's entries in shuffled order"""
    rows, keys = np.asarray(rows, np.int64), np.asarray(keys, np.int64)
    o = np.lexsort((order_rng.random(len(rows)), rows))
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))]).astype(np.uint64)
    ids = reverse_bytes_np(keys[o].astype(np.uint64))
    return off, ids, (None if vals is None else np.asarray(vals, np.float32)[o])


def _values(rng, n):
    """magnitudes in [0.25, 1], random sign: no addend is small against its neighbours"""
    return (rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


class Case:
    """train / val chunk lists with the parameters of init_model and the designed facts a test can ask for"""


def designed_case(V_dim, seed, tail=1, vth=4, pad_keys=0):
    """Three class chunks T0, T1 (binary), T2, the small chunks S* that put U on both sides of a wave and of a block of
    k_lb_gather, the chunk N none of whose keys carries V, and two validation chunks.  Keys are integers in ReverseBytes
    space (raw id = reverse_bytes(key)), so a chunk's keys lie in integer order and the model's too.

    Class chunk c: row 0 .. R - 1; one empty row in the middle and the last row empty; key HOT in every other row but the two
    clamp rows;
    own keys with 1, 2, 8, 9, 64 and 65 entries and fillers with 3 .. 6; a filler listed twice in one row; with tail >= 1
    its one-entry keys are filtered (map -1), one of them the chunk's largest key; one own three-entry key has only zero
    values (valued chunks); two rows hold nothing but one own key CLAMP_c with a large value of either sign, which the caller scales
    until the reference's logit leaves +-20 (scale_clamp_rows).  Keys ALL* lie in all three chunks, PAIR* in two.
    pad_keys: extra two-entry keys of T0 (to choose the parity of the model size)."""
    rng = np.random.default_rng(seed)
    pw, stride = per_wave(V_dim)
    pool = list(rng.permutation(np.arange(2, 4000)))        # key integers handed out in random order: classes interleave

    def new(n=1):
        return [int(pool.pop()) for _ in range(n)]

    HOT = 1
    ALL = new(4)
    PAIR = [new(3) for _ in range(3)]      # PAIR[c] lies in chunks c and (c + 1) % 3
    R = [232, 244, 236]
    C = Case()
    C.V_dim, C.tail, C.vth, C.pw, C.stride, C.seed = V_dim, tail, vth, pw, stride, seed
    C.train, C.val, C.names, C.clamp = [], [], [], []
    C.hot, C.all3, C.pair = HOT, ALL, PAIR
    C.own, C.single, C.zero_keys, C.dup = [], [], [], []
    for c in range(3):
        binary = c == 1
        nrows = R[c]
        empty = {nrows // 2, nrows - 1}
        live = np.array([r for r in range(nrows) if r not in empty])
        counts = {}
        for k_, n_ in zip(ALL, (64, 65, 8, 9)):
            counts[k_] = n_
        for k_, n_ in zip(PAIR[c], (8, 9, 2)):
            counts[k_] = n_
        for k_, n_ in zip(PAIR[(c - 1) % 3], (9, 2, 8)):
            counts[k_] = n_
        own = {}
        for n_ in BWD_CLASSES:
            for k_ in new(6 if n_ == 1 else 2):
                own[k_] = n_
        last = 4000 + c                                      # the chunk's largest key: one entry
        own[last] = 1
        for k_ in new(110 + 60 * c):
            own[k_] = int(rng.integers(3, 7))
        zk = new(1)[0]
        own[zk] = 3
        dk = new(1)[0]
        own[dk] = 4
        if c == 0:
            for k_ in new(pad_keys):
                own[k_] = 2
        ck = new(1)[0]                                       # CLAMP_c: vth + 2 ordinary entries and the two clamp rows
        own[ck] = vth + 2
        counts.update(own)
        clamp_rows = [int(live[3]), int(live[-4])]
        normal = np.array([r for r in live if r not in clamp_rows])
        rows, keys = [normal], [np.full(len(normal), HOT)]
        for k_, n_ in counts.items():
            if k_ == dk:
                r = rng.choice(normal, n_ - 1, replace=False)
                r = np.concatenate([r, r[:1]])
            else:
                r = rng.choice(normal, n_, replace=False)
            rows.append(r)
            keys.append(np.full(n_, k_))
        rows.append(np.array(clamp_rows))
        keys.append(np.full(2, ck))
        rows, keys = np.concatenate(rows), np.concatenate(keys)
        vals = None
        if not binary:
            vals = _values(rng, len(rows))
            vals[keys == zk] = 0
            vals[-2:] = [2.0, -2.0]
            C.zero_keys.append(zk)
        off, ids, v = _csr(nrows, rows, keys, vals, rng)
        lab = (rng.random(nrows) < 0.45).astype(np.float32)
        C.train.append([off, ids, v, lab])
        C.names.append("T%d" % c)
        C.own.append(own)
        C.single.append([k_ for k_, n_ in own.items() if n_ == 1])
        C.dup.append(dk)
        if not binary:
            C.clamp.append((c, ck, clamp_rows))
    # small chunks: U keys out of the shared ones (they carry V when vth < 8) and the class chunks' own, a few rows
    shared = [HOT] + ALL + [k_ for p in PAIR for k_ in p] + [k_ for o in C.own for k_, n_ in o.items() if n_ >= 8]
    C.small_U = sorted({u for u in (pw - 1, pw, pw + 1, 4 * pw + 1) if u >= 1})
    for U in C.small_U:
        ks = np.array(shared[:U] if U <= len(shared) else shared + new(U - len(shared)))
        nrows = 5
        rows = np.concatenate([rng.integers(0, nrows - 1, len(ks)), rng.integers(0, nrows - 1, len(ks))])   # last row empty
        keys = np.concatenate([ks, ks])
        off, ids, v = _csr(nrows, rows, keys, _values(rng, len(rows)), rng)
        C.train.append([off, ids, v, (rng.random(nrows) < 0.5).astype(np.float32)])
        C.names.append("S%d" % U)
    # N: keys of its own with 2 .. max(vth, 2) entries each: none carries V when vth >= 2
    ks = np.array(new(2 * pw + 3))
    per = np.array([int(rng.integers(2, max(vth, 2) + 1)) for _ in ks])
    keys = np.repeat(ks, per)
    nrows = 9
    rows = rng.integers(0, nrows - 1, len(keys))
    off, ids, v = _csr(nrows, rows, keys, _values(rng, len(rows)), rng)
    C.train.append([off, ids, v, (rng.random(nrows) < 0.5).astype(np.float32)])
    C.names.append("N")
    C.noV_chunk = len(C.train) - 1
    # validation: keys of the model and, for more than 10 % of each chunk's keys, keys no training chunk has
    known = np.array(sorted({int(k_) for c in range(3) for k_ in C.own[c]} | set(shared)))
    for vseed in range(2):
        nrows = 70 + 10 * vseed
        ks = np.concatenate([rng.choice(known, 50, replace=False), np.array(new(12)), [5000 + vseed]])
        per = rng.integers(1, 12, len(ks))
        keys = np.repeat(ks, per)
        rows = rng.integers(0, nrows - 1, len(keys))
        off, ids, v = _csr(nrows, rows, keys, None if vseed else _values(rng, len(rows)), rng)
        C.val.append([off, ids, v, (rng.random(nrows) < 0.5).astype(np.float32)])
    return C


def big_case(V_dim, U, nnz_row, seed, nval_rows=40):
    """one training chunk that names each of U keys once, nnz_row to a row (the last row takes the rest), and one small
    validation chunk; tail = 0 and vth = 0: every key carries V"""
    rng = np.random.default_rng(seed)
    pw, stride = per_wave(V_dim)
    C = Case()
    C.V_dim, C.tail, C.vth, C.pw, C.stride, C.seed = V_dim, 0, 0, pw, stride, seed
    keys = rng.permutation(np.arange(1, U + 1))
    nrows = (U + nnz_row - 1) // nnz_row + 1                 # the last row empty
    rows = np.arange(U) // nnz_row
    off, ids, v = _csr(nrows, rows, keys, _values(rng, U), rng)
    C.train = [[off, ids, v, (rng.random(nrows) < 0.5).astype(np.float32)]]
    C.names = ["BIG"]
    vk = np.concatenate([rng.choice(np.arange(1, U + 1), 300, replace=False), np.arange(U + 1, U + 41)])
    vkeys = np.repeat(vk, 2)
    vrows = rng.integers(0, nval_rows - 1, len(vkeys))
    off, ids, v = _csr(nval_rows, vrows, vkeys, _values(rng, len(vkeys)), rng)
    C.val = [[off, ids, v, (rng.random(nval_rows) < 0.5).astype(np.float32)]]
    C.clamp, C.small_U = [], []
    return C


def make_model(C, l2=0.1, V_l2=0.01):
    return Model(C.train, C.val, V_dim=C.V_dim, V_threshold=C.vth, tail_feature_filter=C.tail, l2=l2, V_l2=V_l2)


def draw_weights(C, M, seed):
    """|w| <= 0.3 and |V| <= 0.3 uniform, every seventh key's w exactly 0; a clamp key's w is 0.3, so that its rows' logits
    grow with its value at a known rate"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.3, 0.3, M.n).astype(np.float32)
    z = M.pos[:-1][::7]
    w[z] = 0
    for _, k_, _ in C.clamp:
        w[M.pos[int(np.searchsorted(M.keys, np.uint64(k_)))]] = 0.3
    return w


def _entry(chunk, row, key):
    """position of the entry (row, key) in a chunk's arrays"""
    off, ids = chunk[0].astype(np.int64), chunk[1]
    rk = reverse_bytes_np(ids[off[row]:off[row + 1]])
    j = np.flatnonzero(rk == np.uint64(key))
    assert len(j) == 1
    return int(off[row]) + int(j[0])


def scale_clamp_rows(C, w):
    """the clamp rows' large values doubled until the reference's unclamped float64 logit of each is beyond +-22 and
    further from +-20 than 10 x its floor (the reference alone decides); rebuilds and returns the model.  V_dim == 0 has no
    clamp: the values stay."""
    M = make_model(C)
    if C.V_dim == 0 or not C.clamp:
        return M
    for _ in range(12):
        f = M.logits(w)
        done = True
        for c, ck, rws in C.clamp:
            for r in rws:
                raw = abs(_raw_logit(M, c, w, r))
                if raw < 22 or raw - 20 < 10 * f[c][1][r]:
                    C.train[c][2][_entry(C.train[c], r, ck)] *= 2
                    done = False
        if done:
            return M
        M = make_model(C)
    raise AssertionError("the clamp rows did not reach +-22")


def _raw_logit(M, c, w, r):
    """the unclamped float64 logit of row r of training chunk c"""
    W, V = M.split(w)
    ch = M.tr[c]
    wc, Vc, _ = M.chunk_rows(ch, W, V)
    X, X2 = ch.D.X[r], ch.D.X2[r]
    f = (X @ wc)[0]
    if M.k:
        f += 0.5 * (((X @ Vc) ** 2).sum() - (X2 @ (Vc * Vc)).sum())
    return float(f)


def separate_labels(M, w, chunks_raw, chunks):
    """AUC must be decided by the reference alone: walking each chunk's rows in the order of their float64 logits, a row
    closer than 10 x the logit floor to its predecessor takes the predecessor's label (its label is re-drawn by rule), so
    that no positive / negative pair is that close (rows clamped to the same +-20 and empty rows included).  Changes the
    label arrays in place -> the number of rows changed"""
    changed = 0
    for raw, ch, (f, ff) in zip(chunks_raw, chunks, M.logits(w, chunks)):
        o = np.argsort(f, kind="stable")
        lab = raw[3]
        for a, b in zip(o[:-1], o[1:]):
            if f[b] - f[a] <= 10 * max(ff[a], ff[b]) and (lab[a] > 0) != (lab[b] > 0):
                lab[b] = lab[a]
                changed += 1
    return changed


def min_class_gap(f, ff, lab):
    """-> the smallest (gap / (10 x floor)) over adjacent rows of different label, in logit order (inf: none)"""
    o = np.argsort(f, kind="stable")
    best = np.inf
    for a, b in zip(o[:-1], o[1:]):
        if (lab[a] > 0) != (lab[b] > 0):
            best = min(best, (f[b] - f[a]) / (10 * max(ff[a], ff[b]) + 1e-300))
    return best


def prepare(C, wseed=0):
    """weights, clamp rows, labels -> (model, w): everything the tests compare against, before any device is touched"""
    M = make_model(C)
    w = draw_weights(C, M, wseed)
    M = scale_clamp_rows(C, w)
    separate_labels(M, w, C.train, M.tr)
    separate_labels(M, w, C.val, M.va)
    return make_model(C), w


def census(C, M, w):
    """asserts the designed facts of a designed_case on the reference's own model and logits"""
    pw = C.pw
    K = len(M.keys)
    in_chunks = np.zeros(K, int)
    for c in M.tr[:3]:
        in_chunks[c.map[c.map >= 0]] += 1
    for ci, c in enumerate(M.tr[:3]):
        occ = set(int(v) for v in c.cnt)
        assert set(BWD_CLASSES) <= occ and c.cnt.max() >= 200, (ci, sorted(occ))
        nz = np.diff(c.off)
        assert (nz == 0).sum() >= 2 and c.cnt[0] == c.cnt.max() >= (nz > 0).sum() - 2, "empty rows; HOT in the others"
        dk = int(np.searchsorted(c.keys, np.uint64(C.dup[ci])))
        per_row = np.bincount(np.repeat(np.arange(c.n), nz)[c.col == dk], minlength=c.n)
        assert per_row.max() == 2, "a row lists the same feature twice"
        if C.tail >= 1:
            f = np.flatnonzero(c.map < 0)
            assert c.map[-1] < 0 and len(f) >= 2, "filtered keys, one the chunk's last"
            if pw >= 4:
                assert ((f % pw != 0) & (f % pw != pw - 1) & (f < c.U - 1)).any(), "a filtered key inside a wave"
        else:
            assert (c.map >= 0).all()
    assert (in_chunks >= 3).any() and (in_chunks == 2).any() and (in_chunks == 1).any()
    if C.V_dim and C.vth > 0:
        assert 0 < M.hasV.sum() < K, "keys with and without V"
        n_ = M.tr[C.noV_chunk]
        assert (n_.map >= 0).any() and not M.hasV[n_.map[n_.map >= 0]].any(), "chunk N: no key carries V"
    assert [c.U for c in M.tr[3:3 + len(C.small_U)]] == C.small_U, "U on both sides of a wave and of a block"
    assert any(c.val is None for c in M.tr) and any(c.val is not None for c in M.tr)
    for c in M.va:
        assert (c.map < 0).sum() >= 0.1 * c.U and (c.map >= 0).any(), "validation keys outside the model"
    assert (w[M.pos[:-1]] == 0).any() and np.abs(w).max() <= f32(0.3)
    pr = M.logits(w)
    if C.V_dim:
        out = sum(int((np.abs(f) >= 20).sum()) for f, _ in pr)
        assert out >= 2, "rows clamped"
        for (f, ff), c in zip(pr, M.tr):
            assert (np.abs(f) < 20).sum() >= 0.9 * c.n
    for (f, ff), c in zip(pr + M.logits(w, M.va), M.tr + M.va):
        assert min_class_gap(f, ff, c.lab) > 1, "AUC order not decided by the reference alone"
        lab = c.lab > 0
        if c.n > 20:
            assert 0 < lab.sum() < c.n


# ------------------------------------------------------------------------------------------------ the ring schedule

FREE = np.array([1e-3, -0.37, 0.8125, 2.0, -1.5, 0.05, -0.004], np.float32)   # coefficients in +-[1e-3, 2]
# the line-search steps of epoch e are ALPHAS[e % 4]: x = alpha - alpha_ takes 0 (a repeated value: w must not change)
# and exactly 1 (a plain add); the last alpha of an epoch is 1 (the s store of the next PrepareCalcDirection is skipped)
# in two of four epochs
ALPHAS = ([0.25, 0.25, 1.25], [1.0], [0.5, 0.0625], [2.0, 1.0])


def draw_coefficients(mir, rng):
    """d [2k + 1] for CalcDirection: 0 or a FREE value everywhere, then one exact 0, one FREE value, one exact 1 on an s
    that stays inside the clamp by itself (max |s| <= 5; any s if there is none) and, where one exists, a -1 on another s
    with max |s| <= 1/2: y and g, whose size the test does not control, never take +-1.  The FREE entries are then scaled
    by the first factor in 1, 2^-1/2, 2^1/2, 1/2, 2, ... that puts between 2 % and 40 % of the mirror's direction beyond
    the clamp (the tests assert 1 % .. 50 % on the direction itself)"""
    k = len(mir.y)
    nd = 2 * k + 1
    free = rng.random(nd) < 0.6
    top = np.array([float(np.abs(v).max()) for v in mir.s])
    ok = np.flatnonzero(top <= 5)
    i1 = int(rng.choice(ok)) if len(ok) else int(rng.integers(0, k))
    rest = [i for i in range(nd) if i != i1]
    i0, i2 = (int(i) for i in rng.choice(rest, 2, replace=False))
    small = [i for i in np.flatnonzero(top <= 0.5) if i not in (i0, i1, i2)]
    d = np.zeros(nd, np.float32)
    free[[i0, i1]], free[i2] = False, True
    if small:
        free[small[0]] = False
        d[small[0]] = -1
    d[i1] = 1
    d[free] = rng.choice(FREE, int(free.sum()))
    every = 1 if len(mir.g) < 100000 else 16
    for j in range(80):
        t = np.float32(2.0 ** (0.5 * ((j + 1) // 2) * (-1 if j % 2 else 1)))
        dd = d.copy()
        dd[free] = d[free] * t
        frac = float((np.abs(mir.chain(dd, every)) > 5).mean())
        if 0.02 <= frac <= 0.4:
            return dd
    raise AssertionError("no scale of the free coefficients clamps between 2 %% and 40 %% of the direction (k = %d)" % k)
