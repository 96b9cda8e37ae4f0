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
}
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
