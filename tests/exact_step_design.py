"""Minibatches on which one SGD step has exactly one right answer (numpy only, no GPU, no oracle).

fp32 addition is exact, in any order, when every term of a sum is a multiple of one power of two q and the sum of the absolute
values stays below 2^24 q.  A design keeps every sum of a step on such a grid:

  model      w on a 2^-4 grid, V on a 2^-3 grid in [-1, 1]; sqrt_g, z and the AdaGrad accumulators are generic (full mantissa)
  values     +-0.5, +-1, +-2 (or binary)
  slopes     only the three that any correct expf yields exactly:
               saturated  a driver key (no V, x = 1) pushes y * pred to <= -20, so p = -y / (1 + exp(-20..)) = -y
               zero       only keys with w = 0 and no V: pred = 0, p = -y / 2
               confident  (V_dim = 0 only, no clamp there) y * pred >= 128: expf overflows, p = -+0 and the term is skipped

Forward, gradient and update then have one right answer, whichever role, lane grouping, wave split or part order produced it,
and the update arithmetic (FTRL, AdaGrad, InitV, the count triggers) runs on an exactly known gradient with generic state and
generic hyper-parameters: a deviation of one ulp shows.  check() asserts these claims; it is a condition, not a tolerance.

Key classes ("cls" of the design):
  V  has V (at V_dim = 0: an ordinary key with w != 0)
  N  no V, w != 0 (the drivers are of this class)
  Z  no V, w = 0 (the only class allowed in zero rows); some have a count beyond V_threshold, so that the update initialises
     their V when w leaves zero
  C  count-push form only: no V, w != 0, the count pushed with the step takes it across V_threshold, so it gets its V at
     count-push time.  Its hashed V has 24 significant bits: two such terms no longer add exactly, so a C key occurs once and
     is the only key with V in its row (its V gradient is then (x V p) x - V (x x p) = 0 exactly)
"""
import numpy as np

V_THRESHOLD = 7000
HYPER = dict(l1=0.02, l2=0.01, lr=0.3, V_lr=0.05, V_l2=0.02, V_init_scale=0.25, V_threshold=V_THRESHOLD, seed=5)
VARIANTS = {
    "base": {},
    "l1_0": dict(l1=0.0),
    "Vl2_0": dict(V_l2=0.0),
    "beta": dict(lr_beta=0.7, V_lr_beta=1.3),
    # the penalty sum is exact too: l1 |w| is on a 2^-10 grid, 0.5 V_l2 v^2 on a 2^-12 grid (exact_progress asserts it).  l2 stays
    # 0: beside the drivers' 0.5 l2 w^2 of 2^16 and more no grid holds the other terms (l2_copy pins that term)
    "pen": dict(l1=2.0 ** -6, l2=0.0, V_l2=2.0 ** -5),
}
L2_COPY = dict(l1=2.0 ** -6, l2=2.0 ** -3, V_l2=2.0 ** -5)
L2_COPY_DRIVER = 2.0
# the smallest set that reaches every role of k_update_fused and its edges: both sides of BWD_SMALL = 8 and BWD_MID = 64, one
# and two tiles per wave, more tiles than waves, HOT_SPLIT_MIN = 4096 (4 097 = five parts, the last of one occurrence)
FULL_LENGTHS = (1, 1, 1, 1, 1, 1, 2, 2, 8, 8, 9, 9, 64, 65, 129, 257, 4096, 4097, 5121)
ROW_CAP = 8          # keys per ordinary row, the driver included
BIG_ROW = 69         # single-occurrence keys beside the driver in the one long row (the singles tile compacts)
W_DRIVER_K0 = 4096.0


def reverse_bytes(x):
    """ReverseBytes of include/difacto/base.h:39-51 (32 / 16 / 8 / 4-bit groups swapped: the nibbles reversed), on u64 arrays"""
    x = np.ascontiguousarray(x, np.uint64).byteswap()
    return ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4)) | ((x & np.uint64(0xF0F0F0F0F0F0F0F0)) >> np.uint64(4))


def _pow2_at_least(x):
    return float(2.0 ** int(np.ceil(np.log2(max(float(x), 1.0)))))


def build(lengths, V_dim, binary, push_cnt=False, variant="base", seed=0):
    """-> dict: the minibatch (offset, index = raw u64 ids, value | None, label), its localized form (keys = the ReverseBytes(id)
    in ascending order, as the Localizer leaves them and the store holds them, cidx, cnt),
    the model to import (scal [U, 4] = {fea_cnt, w, sqrt_g, z}, has_V [U], V [U, 2 V_dim] = V | acc), cls [U], the row classes
    (row_class [nrows]: 's' saturated, 'z' zero, 'c' confident) and the hyper-parameters (hyper)"""
    rng = np.random.default_rng([seed, V_dim, int(binary), int(push_cnt)])
    k = int(V_dim)
    lengths = [int(x) for x in lengths]
    n_train = max(max(lengths) + 79, 200)
    n_conf = 40 if k == 0 else 0
    n_zero = 200 if max(lengths) > 1000 else 40

    # ---- the keys: (class, length); rows are chosen below
    cls, klen = [], []
    cyc = ["V", "N", "Z", "V"]
    for i, L in enumerate(lengths):
        c = "V" if L > 9 else cyc[i % 4]
        cls.append(c)
        klen.append(L)
    named = len(cls)
    # ---- rows: lists of (key number, value)
    rows = [[] for _ in range(n_train)]
    size = np.zeros(n_train, np.int64)
    label = np.where(rng.random(n_train) < 0.5, 1.0, -1.0).astype(np.float32)
    conf = np.zeros(n_train, bool)
    conf[1:1 + n_conf] = True        # row 0 is the long row
    locked = np.zeros(n_train, bool)  # rows that take no further key with V
    locked[0] = True
    c_rows = np.arange(1 + n_conf, 4 + n_conf) if (push_cnt and k > 0) else np.zeros(0, np.int64)
    locked[c_rows] = True                # the rows of the C keys: nothing else with V enters them
    pair_row = 4 + n_conf                # a single-occurrence key alone with its driver
    locked[pair_row] = True

    def val():
        return 1.0 if binary else float(rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]))

    def place(key, L, pool):
        cand = np.flatnonzero(pool & (size < ROW_CAP - 1))
        assert len(cand) >= L, "not enough rows for a key of %d occurrences" % L
        for r in rng.choice(cand, size=L, replace=False):
            rows[r].append((key, val()))
            size[r] += 1

    open_rows = ~locked & ~conf
    one_in_conf = None
    for key in np.argsort(klen)[::-1]:      # longest first: they need the most rows
        L = klen[key]
        if k == 0 and one_in_conf is None and 2 <= L <= 9:
            # a key with ONE occurrence in a confident row
            place(key, 1, conf)
            place(key, L - 1, open_rows)
            one_in_conf = int(key)
        elif L > 64 and k == 0:
            place(key, L, ~locked)           # the long keys meet confident rows too
        else:
            place(key, L, open_rows)

    def new_key(c, L):
        cls.append(c)
        klen.append(L)
        return len(cls) - 1

    # the long row: BIG_ROW single-occurrence keys of every class
    for i in range(BIG_ROW):
        rows[0].append((new_key(["V", "Z", "N"][i % 3], 1), val()))
    rows[pair_row].append((new_key("V", 1), val()))
    # V_dim = 0: a key whose occurrences are ALL in confident rows (gw = 0 exactly; FTRL still runs)
    all_conf = None
    if k == 0:
        all_conf = new_key("V", 3)
        place(all_conf, 3, conf)
    # Z keys in training rows; some of them will leave zero in the update (lazy InitV where the count allows)
    z_keys = [new_key("Z", L) for L in (1, 1, 1, 1, 2, 2, 3, 8, 9, 12)]
    for key in z_keys:
        place(key, klen[key], open_rows)
    # count-push form: C keys, alone-with-V in their rows, beside the driver and a key without V
    for i, r in enumerate(c_rows):
        rows[r].append((new_key("C", 1), val()))
        if i:
            rows[r].append((new_key("NZ"[i % 2], 1), val()))
    # zero rows: Z keys only (no driver), rows of 1, 2 and 3 keys
    zero_pool = z_keys + [new_key("Z", 0) for _ in range(12)]
    zrows = []
    for i in range(n_zero):
        m = 1 + i % 3
        ks = rng.choice(zero_pool, size=m, replace=False)
        zrows.append([(int(q), val()) for q in ks])
        for q in ks:
            klen[q] += 1
    zrows.append([(new_key("Z", 1), val())])   # a single-occurrence key alone in its row
    zlabel = np.where(rng.random(len(zrows)) < 0.5, 1.0, -1.0).astype(np.float32)
    # drivers: w = -D for the saturated rows with y = +1 and the confident rows with y = -1, +D for the others
    d_neg, d_pos = new_key("N", 0), new_key("N", 0)
    for r in range(n_train):
        neg = (label[r] > 0) != bool(conf[r])
        d = d_neg if neg else d_pos
        rows[r].insert(int(rng.integers(0, len(rows[r]) + 1)), (d, 1.0))
        klen[d] += 1
    all_rows = rows + zrows
    labels = np.concatenate([label, zlabel])
    row_class = np.array(["c" if c else "s" for c in conf] + ["z"] * len(zrows))
    order = rng.permutation(len(all_rows))      # the classes interleaved
    order = np.concatenate([[0], order[order != 0]])   # (the long row stays first: easy to find)
    all_rows = [all_rows[i] for i in order]
    labels, row_class = labels[order], row_class[order]

    # ---- keys -> raw u64 ids
    U = len(cls)
    assert all(L > 0 for L in klen)
    raw = np.unique(rng.integers(1, 2 ** 63, size=2 * U, dtype=np.uint64))[:U]
    raw = raw[rng.permutation(U)]                # key number -> id, unrelated to class and length
    offset = np.zeros(len(all_rows) + 1, np.uint64)
    offset[1:] = np.cumsum([len(r) for r in all_rows])
    index = np.array([raw[q] for r in all_rows for q, _ in r], np.uint64)
    value = None if binary else np.array([x for r in all_rows for _, x in r], np.float32)
    # Localizer::Compact (src/data/localizer.cc:24): the store's keys are ReverseBytes(id), in ascending order
    keys, cidx, cnt = np.unique(reverse_bytes(index), return_inverse=True, return_counts=True)
    to_sorted = np.searchsorted(keys, reverse_bytes(raw))       # key number -> rank
    cls_s = np.empty(U, "U1")
    cls_s[to_sorted] = cls
    assert np.array_equal(cnt[to_sorted], klen)

    # ---- the model
    hyper = dict(HYPER, **VARIANTS[variant])
    thr = float(hyper["V_threshold"])
    w = rng.integers(-32, 33, size=U) / 16.0
    w[w == 0] = 0.0625
    w[cls_s == "Z"] = 0.0
    sqrt_g = np.abs(rng.normal(size=U)) + 0.01
    z = rng.normal(size=U) * 0.3
    has_V = ((cls_s == "V") & (k > 0)).astype(np.int32)
    V = np.zeros((U, 2 * k), np.float32)
    if k:
        V[:, :k] = rng.integers(-8, 9, size=(U, k)) / 8.0
        V[:, k:] = np.abs(rng.normal(size=(U, k))) * 0.5 + 0.01
        V[has_V == 0] = 0
    # the counts.  add = what the step's count push adds (0 without it)
    add = cnt.astype(np.float64) if push_cnt else np.zeros(U)
    fea = np.floor(rng.random(U) * 50)
    isN, isZ, isC = cls_s == "N", cls_s == "Z", cls_s == "C"
    if k == 0:
        isN = isN | (cls_s == "V")
    # N: stays at or below the threshold with this count; the first one lands exactly ON it
    n_idx = np.flatnonzero(isN)
    fea[n_idx] = thr - add[n_idx] - np.floor(rng.random(len(n_idx)) * 40)
    fea[n_idx[0]] = thr - add[n_idx[0]]
    # Z: a third beyond the threshold (their V appears if w leaves zero), one lands ON it, one on threshold + 1
    z_idx = np.flatnonzero(isZ)
    z_idx = z_idx[np.argsort(cnt[z_idx], kind="stable")]      # the two on the edge occur once: |gw| <= 2 cannot keep them at zero
    z[z_idx[:2]] = (3.0 + rng.random(2)) * np.array([1.0, -1.0])
    far = rng.random(len(z_idx)) < 0.34
    fea[z_idx[far]] = thr + 1 + np.floor(rng.random(int(far.sum())) * 30)
    fea[z_idx[0]] = thr - add[z_idx[0]]
    fea[z_idx[1]] = thr + 1 - add[z_idx[1]]
    # C: one occurrence, and the count pushed with it takes the key from the threshold to threshold + 1
    c_idx = np.flatnonzero(isC)
    fea[c_idx] = thr + 1 - add[c_idx]
    assert fea.min() >= 0
    scal = np.stack([fea, w, sqrt_g, z], 1).astype(np.float32)

    # ---- the drivers' weight: dominates every other term of every logit it sits in (check() asserts it)
    D = dict(offset=offset, index=index, value=value, label=labels.astype(np.float32), keys=keys, cidx=cidx.astype(np.uint32),
             cnt=cnt.astype(np.float32), scal=scal, has_V=has_V, V=V, cls=cls_s, row_class=row_class, hyper=hyper, V_dim=k,
             binary=bool(binary), push_cnt=bool(push_cnt), variant=variant, lengths=tuple(lengths),
             drivers=(int(to_sorted[d_neg]), int(to_sorted[d_pos])), named=to_sorted[:named].copy(),
             one_in_conf=None if one_in_conf is None else int(to_sorted[one_in_conf]),
             all_conf=None if all_conf is None else int(to_sorted[all_conf]))
    if k == 0:
        wd = W_DRIVER_K0
    else:
        # V of the C keys is not known here: bounded by V_init_scale / 2 per coordinate
        wd = _pow2_at_least(2.0 * _other_terms_bound(D) + 64.0)
    scal[D["drivers"][0], 1] = -wd
    scal[D["drivers"][1], 1] = wd
    return D


def _dense(D, pulled=None):
    """float64 w [U], V [U, k] (zero rows where a key has no V) and has [U] of the weights the step sees: `pulled` = the ragged
    (vals, lens) of Store::Pull of D["keys"], or the model of the design itself"""
    U, k = len(D["keys"]), D["V_dim"]
    if pulled is None:
        return D["scal"][:, 1].astype(np.float64), D["V"][:, :k].astype(np.float64), D["has_V"].astype(bool)
    vals, lens = pulled
    vals = np.asarray(vals, np.float64)
    if k == 0:
        assert len(vals) == U
        return vals.copy(), np.zeros((U, 0)), np.zeros(U, bool)
    lens = np.asarray(lens, np.int64)
    assert len(lens) == U and set(np.unique(lens)) <= {1, 1 + k}
    pos = np.concatenate([[0], np.cumsum(lens)[:-1]])
    w = vals[pos]
    V = np.zeros((U, k))
    has = lens > 1
    for u in np.flatnonzero(has):
        V[u] = vals[pos[u] + 1:pos[u] + 1 + k]
    return w, V, has


def _row_of(D):
    nrows = len(D["offset"]) - 1
    return np.repeat(np.arange(nrows), np.diff(D["offset"].astype(np.int64)))


def _other_terms_bound(D):
    """max over the rows of the sum of |terms| of the logit beside the driver's, 0.5 sum_d (XV_d^2 + XXVV_d) included; the V
    of a C key (not known before the count push) enters with its bound V_init_scale / 2"""
    k = D["V_dim"]
    w, V, _ = _dense(D)
    V = np.abs(V)
    V[D["cls"] == "C"] = D["hyper"]["V_init_scale"] / 2.0
    w = np.abs(w)
    w[list(D["drivers"])] = 0
    x = np.ones(len(D["cidx"])) if D["value"] is None else np.abs(D["value"].astype(np.float64))
    row = _row_of(D)
    nrows = len(D["offset"]) - 1
    s = np.bincount(row, weights=w[D["cidx"]] * x, minlength=nrows)
    if k:
        xv = np.zeros((nrows, k))
        np.add.at(xv, row, V[D["cidx"]] * x[:, None])
        xxvv = np.zeros((nrows, k))
        np.add.at(xxvv, row, (V[D["cidx"]] * x[:, None]) ** 2)
        s = s + 0.5 * (xv ** 2 + xxvv).sum(1)
    return float(s.max())


def _step(D, pulled=None):
    """the step in float64: -> dict(logit, pred, p [nrows], x [nnz], row [nnz], w, V, has, XV [nrows, k])"""
    k = D["V_dim"]
    w, V, has = _dense(D, pulled)
    x = np.ones(len(D["cidx"])) if D["value"] is None else D["value"].astype(np.float64)
    row = _row_of(D)
    nrows = len(D["offset"]) - 1
    ci = D["cidx"]
    wsum = np.bincount(row, weights=w[ci] * x, minlength=nrows)
    XV = np.zeros((nrows, k))
    logit = wsum.copy()
    if k:
        Vh = V * has[:, None]
        np.add.at(XV, row, Vh[ci] * x[:, None])
        xxvv = np.zeros((nrows, k))
        np.add.at(xxvv, row, (Vh[ci] * x[:, None]) ** 2)
        logit = wsum + 0.5 * (XV ** 2 - xxvv).sum(1)
    pred = np.clip(logit, -20.0, 20.0) if k else logit
    y = np.where(D["label"] > 0, 1.0, -1.0)
    yp = y * pred
    p = np.full(nrows, np.nan)
    p[yp <= -20.0] = -y[yp <= -20.0]
    p[pred == 0.0] = -y[pred == 0.0] / 2.0
    if k == 0:
        p[yp >= 128.0] = 0.0
    return dict(wsum=wsum, logit=logit, pred=pred, p=p, x=x, row=row, w=w, V=V, has=has, XV=XV, y=y)


def exact_pred(D, pulled=None):
    """clip(exact logit) as fp32: what every correct forward yields"""
    return _step(D, pulled)["pred"].astype(np.float32)


def exact_gradient(D, pulled=None):
    """per key gw [U] and gV [U, k] (zero where the key has no V) in fp32, computed in float64 from the weights the step
    sees (`pulled`: after a count push the oracle's pulled values; None: the design's own model)"""
    S = _step(D, pulled)
    assert not np.isnan(S["p"]).any(), "a row outside the three classes"
    U, k = len(D["keys"]), D["V_dim"]
    ci, row, x, p = D["cidx"], S["row"], S["x"], S["p"]
    gw = np.bincount(ci, weights=p[row] * x, minlength=U)
    gV = np.zeros((U, k))
    if k:
        xxp = np.bincount(ci, weights=p[row] * x * x, minlength=U)
        np.add.at(gV, ci, S["XV"][row] * (p[row] * x)[:, None])
        gV = np.where(S["has"][:, None], gV - S["V"] * xxp[:, None], 0.0)
    gw32, gV32 = gw.astype(np.float32), gV.astype(np.float32)
    assert np.array_equal(gw32.astype(np.float64), gw) and np.array_equal(gV32.astype(np.float64), gV)
    return gw32, gV32


def ragged_gradient(gw, gV, lens, V_dim):
    """[gw | gV where lens > 1] per key, the layout of Store::Push(kGradient)"""
    if V_dim == 0:
        return gw.copy()
    out = []
    for u in range(len(gw)):
        out.append(gw[u:u + 1])
        if lens[u] > 1:
            out.append(gV[u])
    return np.concatenate(out).astype(np.float32)


def _exact_sums(terms, group, ngroups, what):
    """every sum of `terms` [n] or [n, k] over the entries of one group (and one column) is exact in fp32 in any order: the
    group's terms are multiples of one power of two q and sum |terms| / q < 2^24"""
    t = np.abs(np.asarray(terms, np.float64))
    t2 = t.reshape(len(t), -1)
    g2 = np.repeat(np.asarray(group, np.int64), t2.shape[1])
    flat = t2.ravel()
    nz = flat != 0
    m, e = np.frexp(flat[nz])
    mi = np.round(m * 2.0 ** 53).astype(np.int64)      # t = mi * 2^(e - 53)
    low = mi & -mi                                      # the lowest set bit of every term
    tz = e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    qexp = np.full(ngroups, 10 ** 6, np.int64)
    np.minimum.at(qexp, g2[nz], tz)                     # the grid of every group
    tot = np.zeros((ngroups, t2.shape[1]))
    np.add.at(tot, np.asarray(group, np.int64), t2)
    steps = tot.max(1) * 2.0 ** -np.where(qexp < 10 ** 6, qexp, 0).astype(np.float64)
    assert steps.max() < 2 ** 24, "%s: up to %g grid steps in group %d" % (what, steps.max(), steps.argmax())


def check(D, pulled=None, lengths=None, nperm=20, seed=1):
    """assert the design's claims (see the module docstring) for the weights the step sees"""
    S = _step(D, pulled)
    k, U = D["V_dim"], len(D["keys"])
    ci, row, x, p, y = D["cidx"], S["row"], S["x"], S["p"], S["y"]
    nrows = len(D["offset"]) - 1
    w, V, has = S["w"], S["V"], S["has"]
    dn, dp = D["drivers"]
    # -- every row in one of the classes, and the class it was built as
    assert not np.isnan(p).any(), "a row outside the three classes"
    yp = y * S["pred"]
    cl = D["row_class"]
    assert np.all(yp[cl == "s"] <= -20) and np.all(S["pred"][cl == "z"] == 0) and np.all(yp[cl == "c"] >= 128)
    assert (cl == "s").any() and (cl == "z").any() and ((cl == "c").any() == (k == 0))
    # zero rows: only keys with w = 0 and no V
    zr = cl[row] == "z"
    assert np.all(w[ci[zr]] == 0) and not has[ci[zr]].any()
    # no key twice in a row
    assert len(np.unique(row.astype(np.int64) * U + ci)) == len(ci)
    # -- the driver dominates: |w_driver| >= 2 * sum |other terms| + 64 (no rounding in any order moves the clamp)
    isd = (ci == dn) | (ci == dp)
    assert np.array_equal(np.bincount(row[isd], minlength=nrows) > 0, cl != "z") and np.all(x[isd] == 1) and not has[[dn, dp]].any()
    assert abs(w[dn]) == abs(w[dp])
    other = np.bincount(row[~isd], weights=np.abs(w[ci[~isd]] * x[~isd]), minlength=nrows)
    if k:
        Va = np.abs(V * has[:, None])
        xva = np.zeros((nrows, k))
        np.add.at(xva, row, Va[ci] * np.abs(x)[:, None])
        xxvv = np.zeros((nrows, k))
        np.add.at(xxvv, row, (Va[ci] * x[:, None]) ** 2)
        other = other + 0.5 * (xva ** 2 + xxvv).sum(1)
    assert abs(w[dn]) >= 2 * other[cl != "z"].max() + 64
    # -- per row: wsum (compared as the logit itself at V_dim = 0, where nothing clamps it) and XV
    if k == 0:
        _exact_sums(w[ci] * x, row, nrows, "wsum")
    else:
        _exact_sums((V * has[:, None])[ci] * x[:, None], row, nrows, "XV")
    # -- per key: gw, xxp, sum (XV p) x, the product V * xxp and the difference
    tg = p[row] * x
    _exact_sums(tg, ci, U, "gw")
    gw = np.bincount(ci, weights=tg, minlength=U)
    perm_rng = np.random.default_rng(seed)
    by_key = np.argsort(ci, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=U))])
    if k:
        tx = p[row] * x * x
        _exact_sums(tx, ci, U, "xxp")
        xxp = np.bincount(ci, weights=tx, minlength=U)
        tv = S["XV"][row] * tg[:, None]
        prod = V * xxp[:, None] * has[:, None]
        assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod), "V * xxp is not exact in fp32"
        # the reference starts from -V xxp and adds the terms; the device adds the terms (in tiles, in parts) and subtracts
        # the product: both are sums of the terms and -V xxp in some order
        hv = has[ci]
        _exact_sums(np.concatenate([tv[hv], -prod[has]], 0), np.concatenate([ci[hv], np.flatnonzero(has)]), U, "gV")
    gw32, gV32 = exact_gradient(D, pulled)   # asserts that the cast to fp32 changes nothing
    # -- fp32 sums over random permutations of each key's occurrences give the same bits
    tg32 = tg.astype(np.float32)
    assert np.array_equal(tg32.astype(np.float64), tg)
    for u in range(U):
        occ = by_key[seg[u]:seg[u + 1]]
        if len(occ) < 2:
            continue
        for _ in range(nperm):
            o = perm_rng.permutation(occ)
            # (no term is -0, and x + (-x) = +0 under round-to-nearest: equal values are equal bits here)
            assert (np.cumsum(tg32[o], dtype=np.float32)[-1] + np.float32(0)).view(np.uint32) == gw32[u].view(np.uint32)
            if k and has[u]:
                s32 = np.cumsum(tv[o].astype(np.float32), axis=0, dtype=np.float32)[-1] - prod[u].astype(np.float32)
                assert np.array_equal((s32 + np.float32(0)).view(np.uint32), gV32[u].view(np.uint32))
    # -- the key lengths the test names, among the designed keys; the class edges
    cnt = np.bincount(ci, minlength=U)
    if lengths is not None:
        assert sorted(cnt[D["named"]].tolist()) == sorted(int(v) for v in lengths)
    # single-occurrence keys in rows of 1, 2 and about 70 keys
    rowlen = np.bincount(row, minlength=nrows)
    of_singles = set(rowlen[row[cnt[ci] == 1]].tolist())
    assert {1, 2} <= of_singles and max(of_singles) >= BIG_ROW, sorted(of_singles)
    if k == 0:
        u = D["all_conf"]
        assert np.all(cl[row[ci == u]] == "c") and gw[u] == 0 and w[u] != 0
        u = D["one_in_conf"]
        assert (cl[row[ci == u]] == "c").sum() == 1 and cnt[u] >= 2
    # -- the count triggers
    thr = float(D["hyper"]["V_threshold"])
    fea1 = D["scal"][:, 0].astype(np.float64) + (cnt if D["push_cnt"] else 0)
    c = D["cls"]
    Ncls = (c == "N") | ((c == "V") & (k == 0))
    assert np.all(fea1[Ncls] <= thr) and (fea1[Ncls] == thr).any()
    assert (fea1[c == "Z"] == thr).any() and (fea1[c == "Z"] == thr + 1).any() and (fea1[c == "Z"] > thr + 1).any()
    if k and D["push_cnt"]:
        cu = np.flatnonzero(c == "C")
        assert len(cu) >= 2 and np.all(cnt[cu] == 1) and np.all(fea1[cu] > thr) and (fea1[cu] == thr + 1).any()
        assert np.all(D["scal"][cu, 0] <= thr) and np.all(w[cu] != 0)
        for u in cu:   # alone-with-V in its row
            r = row[ci == u][0]
            assert has[ci[row == r]].sum() == (1 if pulled is not None else 0)
        if pulled is not None:
            assert has[cu].all()
    else:
        assert not (c == "C").any()
    if pulled is not None:
        assert np.array_equal(has, (c == "V") & (k > 0) | (c == "C"))
    return dict(gw=gw32, gV=gV32, pred=S["pred"].astype(np.float32))


# ------------------------------------------------------------------------------------------------- the step's progress sums
# dfh_batch_progress adds the blocks' double slots in double and returns (float) of each sum.  The forward's loss terms and
# the penalty terms of a "pen" design are fp32 values on one grid, so the double sums are exact in any order and the float has
# one right value — but for log1pf(1.0f), of which a correct libm may return float32(ln 2) or a neighbour, and the 24-bit V of
# the C keys: those give a set of floats derived here, never a tolerance.
LN2 = np.float32(np.log(2.0))
LOG1P_ONE = (np.nextafter(LN2, np.float32(0)), LN2, np.nextafter(LN2, np.float32(1)))
_LOSS_GRID = 24          # every loss term is a multiple of 2^-24 (asserted)


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def _pow2_or_zero(h):
    return float(np.float32(h)) == float(h) and (h == 0 or np.frexp(float(h))[0] == 0.5)


def _floats_between(lo, hi):
    """the bit patterns of every float32 in [float32(lo), float32(hi)] (positive, a handful)"""
    a, b = np.float32(lo), np.float32(hi)
    assert 0 <= a <= b
    out = {f32bits(a)}
    while a < b:
        a = np.nextafter(a, np.float32(np.inf))
        out.add(f32bits(a))
        assert len(out) <= 64
    return out


def loss_of(D, pulled=None):
    """-> (l0, l1, l2): the exact double sum of the rows' fp32 loss terms fmaxf(m, 0) + log1pf(expf(-|m|)), m = -y pred, for
    the three values a correct log1pf(1.0f) may take.  Asserts that the sum is exact in double in any order and that one row
    of a class dropped or counted twice changes the float (at V_dim = 0 not for the zero rows: the total is about 2e7, an
    ulp is 2 — their term is pinned by the V_dim > 0 designs, and the loss code does not depend on V_dim)"""
    S = _step(D, pulled)
    k, cl = D["V_dim"], D["row_class"]
    pred = S["pred"].astype(np.float32).astype(np.float64)
    assert np.array_equal(pred, S["pred"])
    m = -S["y"] * pred
    sat, zero, conf = cl == "s", cl == "z", cl == "c"
    if k:
        # m = 20 exactly; any log1pf(expf(-20)) below half an ulp of 20 leaves 20.0f
        assert np.all(m[sat] == 20.0) and 4 * np.log1p(np.exp(-20.0)) < 0.5 * float(np.spacing(np.float32(20)))
    else:
        # no clamp: expf(-m) = 0 (underflow starts near 104) and the term is m itself; confident rows: expf(-|m|) = 0 as well
        assert np.all(m[sat] >= 1024) and np.all(m[conf] <= -128)
    assert np.all(m[zero] == 0)
    fixed = np.where(sat, m, 0.0)
    scaled = fixed * 2.0 ** _LOSS_GRID
    assert np.array_equal(scaled, np.round(scaled))
    base = sum(int(v) for v in scaled)
    nz = int(zero.sum())
    out = []
    for c in LOG1P_ONE:
        ci = float(c) * 2.0 ** _LOSS_GRID
        assert ci == round(ci)
        tot = base + nz * int(ci)
        assert sum(abs(int(v)) for v in scaled) + nz * int(ci) < 2 ** 53, "the loss sum is not exact in double"
        t = tot / 2.0 ** _LOSS_GRID
        assert int(t * 2.0 ** _LOSS_GRID) == tot
        out.append(t)
        # visibility: the total with one row of a class dropped or doubled (exact in double by the same count)
        moved = [m[sat], -m[sat]]
        if k == 0:
            moved.append(-m[conf])        # a confident row taken with the other sign: |m| where 0 belongs
        else:
            moved += [np.array([float(c)]), np.array([-float(c)])]
        for d in moved:
            assert np.all((t + d).astype(np.float32) != np.float32(t)), "a row of a class does not show in the float of the loss"
    return tuple(out)


def penalty_of(D, pulled=None):
    """-> None where the hyper-parameters do not put the terms on a grid, else dict(exact, err, zero_keys): the exact sum over
    the keys of l1 |w| + 0.5 l2 w^2 + 0.5 V_l2 sum_d v_d^2 of the weights the step sees, and the bound err on what the
    device's fp32 terms may differ by.  Asserts
      every term but the V part of the C keys is a multiple of one power of two q, exact as fp32, sum |terms| / q < 2^24: the
        lanes' fp32 partials and the double sums behind them are exact in any grouping;
      C keys (hashed V of 24 bits: sum_d v_d^2 is not order-free): the key's term is off by at most (V_dim + 2) 2^-24 of
        itself, err = the sum of these is below half the smallest non-zero key term; the floats of [exact - err, exact + err]
        are accepted;
      a key's non-zero term is at least 2 ulp of the float total: one key dropped or counted twice shows"""
    h = D["hyper"]
    if not all(_pow2_or_zero(h[n]) for n in ("l1", "l2", "V_l2")) or (h["l1"] == 0 and h["l2"] == 0 and h["V_l2"] == 0):
        return None
    k = D["V_dim"]
    w, V, has = _dense(D, pulled)
    isC = (D["cls"] == "C") & has
    tw = h["l1"] * np.abs(w)
    t2 = 0.5 * h["l2"] * w * w
    tv = 0.5 * h["V_l2"] * (V * has[:, None]) ** 2
    grid = np.concatenate([tw, t2, tv[~isC].ravel()])
    assert np.array_equal(grid.astype(np.float32).astype(np.float64), grid), "a penalty term is not exact in fp32"
    _exact_sums(grid, np.zeros(len(grid), np.int64), 1, "penalty")
    term = tw + t2 + np.array([float(np.sum(r)) if not c else 0.0 for r, c in zip(tv, isC)])
    import math
    cterm = np.array([math.fsum(r) for r in tv[isC]]) if isC.any() else np.zeros(0)
    term[isC] += cterm
    exact = math.fsum(term)
    err = float(np.sum((k + 2) * 2.0 ** -24 * term[isC]))
    nzt = term[term != 0]
    ftot = np.float32(exact)
    assert len(nzt) and nzt.min() >= 2 * float(np.spacing(ftot)), "a key's penalty does not show in the float of the sum"
    assert err < 0.5 * nzt.min()
    # (a lane's fp32 partial that holds such a term beside grid terms rounds at the partial's size, not the term's: an interval
    # eight times as wide must give the same floats, so that this does not decide the outcome either)
    assert _floats_between(exact - 8 * err, exact + 8 * err) == _floats_between(exact - err, exact + err)
    return dict(exact=exact, err=err, zero_keys=int((term == 0).sum()))


def auc_of(D, pulled=None):
    """AUC x n of the step's exact logits as the device leaves it in its double accumulator"""
    import auc_ref
    pred = exact_pred(D, pulled)
    n, tp = len(pred), int((D["label"] > 0).sum())
    return auc_ref.auc_times_n_f64(auc_ref.area(D["label"], pred), tp, n)


def exact_progress(D, pulled=None, penalty=True, loss=True):
    """the one right Progress of a design's step, as doubles before the cast: dict(nrows, loss = the three candidates | None,
    penalty = dict(exact, err) | None, auc).  penalty = False: a step that counts none (the packed path)"""
    pen = dict(exact=0.0, err=0.0, zero_keys=0) if not penalty else penalty_of(D, pulled)
    return dict(nrows=len(D["label"]), loss=loss_of(D, pulled) if loss else None, penalty=pen, auc=auc_of(D, pulled) if loss else None)


def accepted(steps):
    """what dfh_batch_progress may return after the steps `steps` (exact_progress dicts) since the last reset: the doubles
    added up, then the cast.  -> dict(nrows = bits, loss = set of bits | None, penalty = set of bits | None, auc = bits | None)"""
    out = dict(nrows=f32bits(sum(s["nrows"] for s in steps)), loss=None, penalty=None, auc=None)
    if all(s["loss"] is not None for s in steps):
        out["loss"] = {f32bits(sum(s["loss"][j] for s in steps)) for j in range(3)}   # (each sum exact: far below 2^53 grid steps)
    if all(s["auc"] is not None for s in steps):
        a = 0.0
        for s in steps:       # the device's own order of additions
            a += s["auc"]
        out["auc"] = f32bits(a)
    if all(s["penalty"] is not None for s in steps):
        ex = sum(s["penalty"]["exact"] for s in steps)
        er = sum(s["penalty"]["err"] for s in steps)
        out["penalty"] = _floats_between(ex - er, ex + er)
    return out


def assert_progress(prog, want, what):
    """a capi.Progress against accepted(...): == on bit patterns, or membership in the derived set"""
    assert f32bits(prog.nrows) == want["nrows"], "%s: nrows %r" % (what, prog.nrows)
    if want["loss"] is not None:
        assert f32bits(prog.loss) in want["loss"], "%s: loss %r (%#x), accepted %s" % (
            what, prog.loss, f32bits(prog.loss), sorted("%#x" % b for b in want["loss"]))
    if want["penalty"] is not None:
        assert f32bits(prog.penalty) in want["penalty"], "%s: penalty %r (%#x), accepted %s" % (
            what, prog.penalty, f32bits(prog.penalty), sorted("%#x" % b for b in want["penalty"]))
    if want["auc"] is not None:
        assert f32bits(prog.auc) == want["auc"], "%s: AUC x n %r (%#x), expected %#x" % (what, prog.auc, f32bits(prog.auc), want["auc"])


def l2_copy(D):
    """the design with the drivers' w at +-L2_COPY_DRIVER and the hyper-parameters L2_COPY: beside drivers of 4 096 and more
    no grid holds 0.5 l2 w^2 and the other terms, here penalty_of's conditions hold with l2 != 0.  check() does not apply to
    the copy (its rows are in no class): only the penalty and nrows of its step have one right answer — the penalty depends
    on the pulled weights of the unique keys and on nothing else"""
    C = dict(D)
    C["scal"] = D["scal"].copy()
    C["scal"][D["drivers"][0], 1] = -L2_COPY_DRIVER
    C["scal"][D["drivers"][1], 1] = L2_COPY_DRIVER
    C["hyper"] = dict(D["hyper"], **L2_COPY)
    C["variant"] = D["variant"] + "+l2copy"
    return C


# ------------------------------------------------------------------------------------------------- the step after a step
# After its step a design's model is generic: full mantissas in w, V and the accumulators.  Two things still have one right
# answer on it (tests/test_second_step_exact.py): the logits of a probe of one-key rows, which show the w every key's {row, w}
# word carries, and a second training step whose gradient is exact again, which shows the header, V row and accumulators the
# update reads.
BWD_SMALL, BWD_MID = 8, 64
SECOND_LIST_LENGTHS = (2, BWD_SMALL, BWD_SMALL + 1, BWD_MID, BWD_MID + 1)


def _minibatch(D, rows, labels, binary, extra):
    """rows = lists of (key rank in D["keys"], value) -> a minibatch dict in the form build() returns, its keys a subset of
    D's: sub [U2] = their ranks in D["keys"]"""
    raw = reverse_bytes(D["keys"])       # (the nibble reversal is its own inverse)
    offset = np.zeros(len(rows) + 1, np.uint64)
    offset[1:] = np.cumsum([len(r) for r in rows])
    index = np.array([raw[u] for r in rows for u, _ in r], np.uint64)
    value = None if binary else np.array([x for r in rows for _, x in r], np.float32)
    keys, cidx, cnt = np.unique(reverse_bytes(index), return_inverse=True, return_counts=True)
    sub = np.searchsorted(D["keys"], keys)
    assert np.array_equal(D["keys"][sub], keys)
    return dict(extra, offset=offset, index=index, value=value, label=np.asarray(labels, np.float32), keys=keys,
                cidx=cidx.astype(np.uint32), cnt=cnt.astype(np.float32), sub=sub, V_dim=D["V_dim"], hyper=D["hyper"], binary=bool(binary))


def _rows_of(D):
    off = D["offset"].astype(np.int64)
    x = np.ones(len(D["cidx"])) if D["value"] is None else D["value"].astype(np.float64)
    return [[(int(D["cidx"][j]), float(x[j])) for j in range(off[i], off[i + 1])] for i in range(len(off) - 1)]


def probe(D, seed=3):
    """a minibatch of one-key rows, one row per key of D in random order, x in +-0.5, +-1, +-2 (a power of two: w x is exact)"""
    rng = np.random.default_rng([seed, D["V_dim"], len(D["keys"])])
    U = len(D["keys"])
    x = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=U)
    order = rng.permutation(U)
    labels = np.where(rng.random(U) < 0.5, 1.0, -1.0)
    P = _minibatch(D, [[(int(u), float(x[u]))] for u in order], labels, False, dict(kind="probe"))
    assert np.array_equal(P["sub"], np.arange(U)) and np.all(P["cnt"] == 1)
    P["x"], P["key_of_row"] = x, order
    return P


def probe_logits(P, model, stale_w=None):
    """-> (lo, hi) float32 [nrows]: the logits of the probe on `model` = (scal, has_V, V | acc) lie in [lo, hi]; lo == hi as
    bit patterns wherever the key has no V (every key at V_dim = 0): fl(w x), clamped to +-20 when V_dim > 0.

    A key with V: 0.5 sum_d ((x v_d)^2 - x^2 v_d^2).  Rounded operation by operation this is 0 bit for bit — x is a power of
    two, fl((x v)^2) == fl(v^2) x^2, asserted here — but the forward is compiled with contraction and takes the difference in
    one fma: each coordinate leaves x^2 (v_d^2 - fl(v_d^2)), the rounding error of the square, exactly.  Their sum is at most
    B = 0.5 x^2 sum_d |v_d^2 - fl(v_d^2)| in magnitude however it is grouped (a sum of these in fp32 gains less than 2^-20 of
    itself), so any correct forward, contracting or not, gives a float of [w x - B, w x + B]: the accepted set, derived from the
    model alone.  stale_w [U]: asserts that fl(stale_w x) is OUTSIDE the set for every key whose w differs from it — a forward
    that read the w of before the step cannot pass."""
    scal, has, V = model
    k = V.shape[1] // 2
    u = P["key_of_row"]
    x = P["x"][u]
    w = scal[u, 1].astype(np.float64)
    v = V[u, :k].astype(np.float64) * (has[u] != 0)[:, None]
    v2 = v * v                                              # exact in double (24-bit factors)
    f = np.float32
    assert np.array_equal((f(1) * (v * x[:, None]).astype(f)) ** 2, (v2.astype(f) * f(1)) * (x[:, None] ** 2).astype(f))
    B = 0.5 * x * x * np.abs(v2 - v2.astype(f).astype(np.float64)).sum(1) * (1 + 2.0 ** -19)
    wx = w * x
    assert np.array_equal(wx.astype(f).astype(np.float64), wx)
    lo, hi = (wx - B).astype(f) + f(0), (wx + B).astype(f) + f(0)      # (+0: w = 0 is skipped, the sum stays +0)
    if k:
        lo, hi = np.clip(lo, f(-20), f(20)), np.clip(hi, f(-20), f(20))
    noV = has[u] == 0
    assert np.array_equal(lo[noV].view(np.uint32), hi[noV].view(np.uint32)) and (k == 0) == bool(noV.all())
    if stale_w is not None:
        s = (np.asarray(stale_w, np.float64)[u] * x).astype(f) + f(0)
        if k:
            s = np.clip(s, f(-20), f(20))
        moved = np.asarray(stale_w, np.float32)[u].view(np.uint32) != scal[u, 1].view(np.uint32)
        seen = (s < lo) | (s > hi)
        # (behind the clamp a change of w cannot show: the drivers at V_dim > 0)
        clamped = (np.abs(lo) == 20) & (np.abs(s) == 20) if k else np.zeros(len(u), bool)
        assert np.all(seen[moved & ~clamped]), "a key's stale w would pass the probe"
        assert (moved & ~clamped).sum() >= 0.5 * len(u)
    return lo, hi


def second_minibatch(D, has_after, seed=4):
    """the minibatch of the step after D's step.  has_after [U]: which keys have V once D's step is done.

    V_dim = 0: D's own saturated and confident rows, the zero rows left out (their keys are left at zero).
    V_dim > 0: rows of {driver, one key}, every key once or twice with one |x|, so that its V gradient is
    (x V p) x - V (x^2 p) = 0 exactly whatever V holds, and 64 rows of a driver with up to five keys WITHOUT V that bring these
    to SECOND_LIST_LENGTHS occurrences: the few, mid and hot lists of the second step are not empty."""
    k = D["V_dim"]
    rng = np.random.default_rng([seed, k, int(D["binary"]), int(D["push_cnt"])])
    if k == 0:
        keep = np.flatnonzero(D["row_class"] != "z")
        rows = _rows_of(D)
        M = _minibatch(D, [rows[i] for i in keep], D["label"][keep], D["binary"], dict(kind="second", row_class=D["row_class"][keep]))
    else:
        assert not D["binary"]
        dn, dp = D["drivers"]
        rows, labels = [], []

        def add(entries):
            y = 1.0 if rng.random() < 0.5 else -1.0
            entries = list(entries)
            entries.insert(int(rng.integers(0, len(entries) + 1)), (dn if y > 0 else dp, 1.0))
            rows.append(entries)
            labels.append(y)

        others = [u for u in range(len(D["keys"])) if u not in (dn, dp)]
        for u in others:
            x = float(rng.choice([0.5, 1.0, 2.0]))
            for _ in range(1 + int(rng.random() < 0.5)):
                add([(u, x if rng.random() < 0.5 else -x)])
        nov = [u for u in others if not has_after[u]]
        listed = [int(u) for u in rng.choice(nov, size=len(SECOND_LIST_LENGTHS), replace=False)]
        have = {u: sum(1 for r in rows for q, _ in r if q == u) for u in listed}
        for i in range(max(SECOND_LIST_LENGTHS)):
            e = [(u, float(rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]))) for u, L in zip(listed, SECOND_LIST_LENGTHS) if have[u] + i < L]
            if e:
                add(e)
        order = rng.permutation(len(rows))
        M = _minibatch(D, [rows[i] for i in order], np.array(labels)[order], False,
                       dict(kind="second", row_class=np.full(len(rows), "s"), listed=np.array(listed)))
    M["drivers"] = tuple(int(np.searchsorted(M["sub"], d)) for d in D["drivers"])
    M["push_cnt"] = False
    return M


def second_step_check(M, w, V, has):
    """assert that the step on minibatch M (second_minibatch) has one right gradient on the weights w [U2], V [U2, k], has
    [U2] — generic values: the oracle's after the step before — and return dict(gw [U2], gV [U2, k] = 0, pred | None).

    Every row holds a driver (x = 1, no V) whose |w| >= 2 sum |other terms| + 64, against the label in a saturated row and
    with it in a confident one: however the generic terms round, y pred <= -18 (V_dim > 0: clamped to -20), so
    1 + expf(y pred) == 1 and p = -y, or y pred >= 128 (V_dim = 0), expf overflows and p = -+0.  gw is then a sum of +-x on a
    grid.  A key with V sits alone-with-V in its rows with one |x|: gV = 0 exactly.  The logits are generic sums at
    V_dim = 0 (not compared); at V_dim > 0 they are -+20."""
    k = M["V_dim"]
    w, V, has = np.asarray(w, np.float64), np.asarray(V, np.float64), np.asarray(has, bool)
    ci, nrows, U = M["cidx"], len(M["label"]), len(M["keys"])
    row = _row_of(M)
    x = np.ones(len(ci)) if M["value"] is None else M["value"].astype(np.float64)
    y = np.where(M["label"] > 0, 1.0, -1.0)
    dn, dp = M["drivers"]
    isd = (ci == dn) | (ci == dp)
    assert np.all(np.bincount(row[isd], minlength=nrows) == 1) and np.all(x[isd] == 1) and not has[[dn, dp]].any()
    assert len(np.unique(row.astype(np.int64) * U + ci)) == len(ci)
    wd = np.zeros(nrows)
    wd[row[isd]] = w[ci[isd]]
    other = np.bincount(row[~isd], weights=np.abs(w[ci[~isd]] * x[~isd]), minlength=nrows)
    if k:
        Va = np.abs(V * has[:, None])
        xva = np.zeros((nrows, k))
        np.add.at(xva, row, Va[ci] * np.abs(x)[:, None])
        xxvv = np.zeros((nrows, k))
        np.add.at(xxvv, row, (Va[ci] * x[:, None]) ** 2)
        other = other + 0.5 * (xva ** 2 + xxvv).sum(1)
    sat = M["row_class"] == "s"
    assert np.all(np.abs(wd) >= 2 * other + 64) and sat.any()
    assert np.all((y * wd)[sat] < 0) and np.all((y * wd)[~sat] > 0) and np.all((np.abs(wd) - other)[~sat] >= 256)
    assert k == 0 or sat.all()
    # (the fp32 sum of a row's terms in any order is off by less than 1: far inside the margin of 64)
    assert np.bincount(row, minlength=nrows).max() * 2.0 ** -23 * (np.abs(wd) + other).max() < 1
    p = np.where(sat, -y, 0.0)
    tg = p[row] * x
    _exact_sums(tg, ci, U, "gw of the second step")
    gw = np.bincount(ci, weights=tg, minlength=U)
    gw32 = gw.astype(np.float32)
    assert np.array_equal(gw32.astype(np.float64), gw)
    if k:
        hv = has[ci]
        assert np.bincount(row[hv], minlength=nrows).max() == 1
        for u in np.flatnonzero(has):
            assert len(np.unique(np.abs(x[ci == u]))) == 1
        tx = p[row] * x * x
        _exact_sums(tx, ci, U, "xxp of the second step")
        xxp = np.bincount(ci, weights=tx, minlength=U)
        # (x V p) x and V xxp: products with +-x^2 and with a sum of at most two +-x^2 of one |x| — powers of two or zero
        m, _ = np.frexp(np.abs(xxp[has]))
        assert np.all((m == 0.5) | (m == 0)) and np.all(np.bincount(ci, minlength=U)[has] <= 2)
        cnt = np.bincount(ci, minlength=U)
        assert set(SECOND_LIST_LENGTHS) <= set(cnt[~has].tolist())
    return dict(gw=gw32, gV=np.zeros((U, k), np.float32), pred=(-20.0 * y).astype(np.float32) if k else None)
