"""The block step of learner = bcd (difacto_amd/csrc/dfh_bcd.hip) on designed inputs: keys that end on, begin on and cover
the 64-entry steps and 128-entry shares of k_bcd_grad, chains of 63 / 64 / 65 / 127 / 128 / 129 following shares for
k_bcd_fixup's rounds of 64, block slices that start off the share grid, filtered keys (s_gk = -1) on share boundaries,
binary chunks, validation chunks with keys that training never had, a key twice in a row, empty rows, and every branch of
k_bcd_update.  Every step goes through R.check_block (tests/bcd_ref.py): g and h within 1e-6 of the sums of |terms|,
w / delta / delta w and every chunk's pred bit for bit.

test_cases_reach_their_edges runs without a GPU: it builds every case's inputs, runs the restatement alone through the
same steps and asserts, by R.share_census / R.update_census, that the case really holds the edges it is there for.  The
conditions are fixed; if a case misses one, its inputs are wrong.

The epoch form (o.epoch, launches queued back to back, gacc / hacc cleared by the update kernel) is compared bit for bit
where that is exact for a reason: the objects of cases B and D rebuilt with every block's keys in a row band of its own
and values that are multiples of 2^-10.  In the first epoch every gradient then reads pred = 0 (first touch), where
p = -y / 2 and t = 1 / 4 whatever expf rounds to, every float term is a multiple of 2^-22 below 2^5, and every fp64 sum
of them is exact in any order.  The second epoch, where the two expf differ by ulps, is held to the bound of
test_bcd_kernels.test_empty_blocks_and_epochs (objective within 1e-5)."""
import functools

import numpy as np
import pytest

import bcd_ref as R

gpu = pytest.mark.gpu


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


class Case:
    """train / val: chunks as designed_chunk returns them; steps: the block sequence both sides run"""

    def __init__(self, train, ranges, steps, val=(), l1=.1, lr=.8, tail=0):
        self.train, self.val, self.ranges, self.steps = list(train), list(val), ranges, list(steps)
        self.l1, self.lr, self.tail = l1, lr, tail

    def ref(self):
        return R.bcd_with_ranges(self.train, self.val, self.ranges, l1=self.l1, lr=self.lr, tail_feature_filter=self.tail)

    def device(self, capi, ctx):
        return R.make_device(capi, ctx, self.train, self.ranges, l1=self.l1, lr=self.lr, tail=self.tail, val=self.val)


def _twice(nblk, seed):
    """every block twice, so that pred and w are non-zero the second time; a shuffled order each pass"""
    rng = np.random.default_rng(seed)
    return [int(b) for _ in range(2) for b in rng.permutation(nblk)]


# ---- case A: boundaries and chains.  Positions below are counted from the start of the block's slice.
A_BLOCKS = [
    # block 0: a 5-entry key first, so that no later block starts on the grid; chains of 63, 64 and 65 following shares
    [5, 128 * 63 + 7, 3, 128 * 64, 128 * 65 + 3],
    # block 1: chains of 127, 128 and 129 following shares
    [128 * 127 + 9, 128 * 128, 128 * 129 + 1],
    # block 2: 128 on [0, 128) and 256 on [128, 384) fill whole shares; 64 ends on the step boundary 448, where 63 begins;
    # 1 at 511 ends on a share boundary; 65, 127, 129, 255, 257 follow; 128 and 256 again off the grid; the last key's
    # chain ends in the block's last (partial) share
    [128, 256, 64, 63, 1, 65, 127, 129, 255, 257, 128, 256, 300],
    [200],              # block 3: one key
    [3, 10, 20],        # block 4: fewer than 64 entries
]


@functools.lru_cache(None)
def case_a():
    chunk, ranges = R.designed_chunk(A_BLOCKS, 20000, seed=11)
    return Case([chunk], ranges, _twice(len(ranges), 1))


def cond_a(case, ref):
    cs = [R.share_census(ref, ref.tr[0], b) for b in range(len(ref.ranges))]
    kept = lambda c: c["gk"] >= 0
    allk = lambda name: np.concatenate([c[name][kept(c)] for c in cs])
    count, follow = allk("count"), allk("follow")
    bsh, bst, esh, est = allk("begins_share"), allk("begins_step"), allk("ends_share"), allk("ends_step")
    out = {"three or more blocks": len(cs) >= 3,
           "block 0 begins with a key of a few entries": cs[0]["count"][0] < 10,
           "every later block starts off the 64-entry grid": all(c["start"] % 64 != 0 and c["start_mod"] % 64 != 0 for c in cs[1:]),
           "a key fills exactly one share": bool(np.any(bsh & esh & (count == 128))),
           "a key fills exactly two shares": bool(np.any(bsh & esh & (count == 256))),
           "a key begins on a step start inside a share": bool(np.any(bst & ~bsh)),
           "a key ends on a step boundary inside a share": bool(np.any(est & ~esh)),
           "a key ends on a share boundary": bool(np.any(esh & ~bsh)),
           "a chain ends in its block's last share": any(
               bool(np.any(kept(c) & (c["follow"] >= 2) & (c["last"] // 128 == c["nshares"] - 1))) and c["n"] % 128 != 0 for c in cs),
           "a block of a single key": any(len(c["key"]) == 1 and c["n"] > 128 for c in cs),
           "a block of fewer than 64 entries": any(0 < c["n"] < 64 and len(c["key"]) > 1 for c in cs)}
    for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        out["a key of %d entries" % n] = bool(np.any(count == n))
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        out["a key reaching exactly %d following shares" % n] = bool(np.any(follow == n))
    return out


# ---- case B: filtered keys (tail_feature_filter = 2: merged count <= 2), two training chunks.  F: filtered.
B_BLOCKS_0 = [
    [4, 7, 1],                                        # block 0: small, so block 1 starts off the grid; its 1 is filtered
    # block 1: kept 127 on [0, 127); F 1 at 127 | F 1 at 128: two filtered keys meet on a share boundary; kept 126 on
    # [129, 255); F 2 at 255 | 256: one filtered key across a boundary; kept 127 on [257, 384); F 1 at 384 opens a share
    # behind a kept key; kept 126 on [385, 511); F 1 at 511 closes a share before the kept 300 on [512, 812), a chain
    # of 2 with F 2 right behind it; then the key with 1 entry here and 2 in chunk 1 (kept), and a kept 40
    [127, 1, 1, 126, 2, 127, 1, 126, 1, 300, 2, 1, 40],
    [30, 2, 50, 20, 45],                              # block 2: no entry at all in chunk 1
    [1, 128 * 3 + 5, 2, 700, 1],                      # block 3: chains between filtered keys; the last F sits in a row of its own
]
B_BLOCKS_1 = [
    [9, 0, 0],
    [60, 0, 0, 130, 0, 0, 0, 200, 0, 129, 0, 2, 0],
    [0, 0, 0, 0, 0],
    [0, 500, 0, 64, 0],
]
B_MERGED_KEY = 3 + 12          # the 12th key of block 1 (keys count from 1): 1 entry + 2 entries
B_SOLO_KEY = 3 + 13 + 5 + 5    # the last key of block 3


def _case_b(bands):
    kw = dict(solo=(B_SOLO_KEY,), empty_rows=7, bands=bands, dyadic=bands)
    c0, ranges = R.designed_chunk(B_BLOCKS_0, 6000, seed=21, **kw)
    c1, _ = R.designed_chunk(B_BLOCKS_1, 4000, seed=22, empty_rows=3, bands=bands, dyadic=bands)
    return Case([c0, c1], ranges, _twice(len(ranges), 2), tail=2)


@functools.lru_cache(None)
def case_b():
    return _case_b(False)


def _row_census(c):
    """per row of a chunk of the restatement: entries, filtered entries"""
    return np.bincount(c.row, minlength=c.n), np.bincount(c.row[c.gk < 0], minlength=c.n)


def cond_b(case, ref):
    c0, c1 = ref.tr
    cs = [R.share_census(ref, c0, b) for b in range(len(ref.ranges))]
    cs1 = [R.share_census(ref, c1, b) for b in range(len(ref.ranges))]
    cat = lambda name: np.concatenate([c[name] for c in cs])
    lgk, rgk, lkey, rkey = cat("b_lgk"), cat("b_rgk"), cat("b_lkey"), cat("b_rkey")
    before = after = False
    for c in cs:
        chain = np.flatnonzero((c["gk"] >= 0) & (c["follow"] >= 2))
        before |= any(i > 0 and c["gk"][i - 1] < 0 for i in chain)
        after |= any(i + 1 < len(c["gk"]) and c["gk"][i + 1] < 0 for i in chain)
    nall, nfil = _row_census(c0)
    fcount = np.concatenate([c["count"][c["gk"] < 0] for c in cs])
    mk = np.uint64(B_MERGED_KEY)
    return {"several filtered keys of 1 and of 2 entries": (fcount == 1).sum() >= 3 and (fcount == 2).sum() >= 2,
            "a key of 1 + 2 entries over the chunks is kept": bool(
                c0.cnt[c0.keys == mk] == 1 and c1.cnt[c1.keys == mk] == 2 and mk in ref.keys),
            "two different filtered keys meet on a share boundary": bool(np.any((lgk < 0) & (rgk < 0) & (lkey != rkey))),
            "one filtered key of 2 entries lies across a share boundary": bool(np.any((lgk < 0) & (rgk < 0) & (lkey == rkey))),
            "a filtered entry opens a share behind a kept key": bool(np.any((lgk >= 0) & (rgk < 0))),
            "a filtered entry closes a share before a kept key": bool(np.any((lgk < 0) & (rgk >= 0))),
            "a kept chain key directly behind a filtered key": bool(before),
            "a kept chain key directly before a filtered key": bool(after),
            "a row whose entries are all filtered": bool(np.any((nall > 0) & (nall == nfil))),
            "empty rows": bool((nall == 0).sum() >= 2),
            "a block without an entry in chunk 1": any(a["n"] > 0 and b["n"] == 0 for a, b in zip(cs, cs1)),
            "a block slice that starts off the grid": any(c["start"] % 64 != 0 for c in cs[1:])}


# ---- case C: binary chunks (A's layout without the chains beyond 65), and a binary chunk next to a valued one
C_BLOCKS = [[5, 3, 128 * 64, 128 * 65 + 3]] + A_BLOCKS[2:]
C_BLOCKS_VALUED = [[40, 0, 700, 129]] + [[max(n // 2, 1) for n in b] for b in A_BLOCKS[2:]]


@functools.lru_cache(None)
def case_c():
    chunk, ranges = R.designed_chunk(C_BLOCKS, 12000, seed=31, binary=True, dup=(3,))
    return Case([chunk], ranges, _twice(len(ranges), 3))


@functools.lru_cache(None)
def case_c_mixed():
    c0, ranges = R.designed_chunk(C_BLOCKS, 12000, seed=32, binary=True)
    c1, _ = R.designed_chunk(C_BLOCKS_VALUED, 3000, seed=33, dup=(4,))
    return Case([c0, c1], ranges, _twice(len(ranges), 4))


def cond_c(case, ref):
    c = ref.tr[0]
    cs = [R.share_census(ref, c, b) for b in range(len(ref.ranges))]
    follow = np.concatenate([x["follow"] for x in cs])
    out = {"the first chunk is binary": c.val is None,
           "a block slice that starts off the grid": any(x["start"] % 64 != 0 for x in cs[1:])}
    for n in (0, 1, 2, 64, 65):
        out["a key reaching exactly %d following shares" % n] = bool(np.any(follow == n))
    if len(ref.tr) > 1:
        out["the second chunk has values"] = ref.tr[1].val is not None
        out["both chunks hold the same blocks' keys"] = all(
            R.share_census(ref, ref.tr[1], b)["n"] > 0 for b in range(len(ref.ranges)))
    return out


# ---- case D: validation chunks.  Per key: entries in (training 0, training 1, validation 0, validation 1)
D_KEYS = [
    # block 0
    [(300, 200, 150, 100), (1, 1, 40, 6),      # the 2nd key: filtered by training (1 + 1), 40 and 6 entries in validation
     (0, 0, 60, 30),                           # never in training
     (129, 64, 10, 5), (50, 0, 0, 20), (0, 3, 7, 0)],
    # block 1: validation 1 has no entry here
    [(700, 400, 300, 0), (128, 256, 65, 0), (2, 0, 9, 0), (257, 100, 0, 0)],
    # block 2: validation 0 holds only keys without a model position here (entries, but no record)
    [(90, 10, 0, 12), (0, 0, 25, 3), (1, 0, 4, 0), (64, 63, 0, 40)],
    # block 3
    [(5, 5, 5, 5), (0, 0, 2, 2), (33, 0, 1, 0)],
]
D_DUP_TRAIN, D_DUP_VAL = 4, 1      # keys (counted from 1) put twice into one row of training 0 / of the validation chunks
D_ROWS = (3000, 2500, 2000, 1500)


def _case_d(bands):
    chunks = []
    for i, n in enumerate(D_ROWS):
        counts = [[k[i] for k in b] for b in D_KEYS]
        c, ranges = R.designed_chunk(counts, n, seed=41 + i, dup=(D_DUP_TRAIN,) if i == 0 else (D_DUP_VAL,) if i >= 2 else (),
                                     empty_rows=4, bands=bands, dyadic=bands)
        chunks.append(c)
    return Case(chunks[:2], ranges, _twice(len(ranges), 5), val=chunks[2:], tail=2)


@functools.lru_cache(None)
def case_d():
    return _case_d(False)


def _dup_in_row(c):
    """some row of the chunk holds one key twice (entries are in key order, ties in row order)"""
    return bool(np.any((c.col[1:] == c.col[:-1]) & (c.row[1:] == c.row[:-1])))


def cond_d(case, ref):
    out = {"two training and two validation chunks": len(ref.tr) == 2 and len(ref.va) == 2,
           "a key twice in one row of a training chunk": _dup_in_row(ref.tr[0])}
    trained = np.unique(np.concatenate([c.keys for c in ref.tr]))
    for i, c in enumerate(ref.va):
        unseen = ~np.isin(c.keys, trained)
        filtered = np.isin(c.keys, trained) & ~np.isin(c.keys, ref.keys)
        cs = [R.share_census(ref, c, b) for b in range(len(ref.ranges))]
        out["validation %d: keys that training never has" % i] = bool(unseen.any())
        out["validation %d: keys that training filtered" % i] = bool(filtered.any())
        out["validation %d: a key twice in one row" % i] = _dup_in_row(c)
        out["validation %d: an empty row" % i] = bool(np.any(_row_census(c)[0] == 0))
        out["validation %d: a block without a record" % i] = any(not np.any(x["gk"] >= 0) for x in cs)
        # an unseen key inside a block's range, between kept keys: its entries lie in the block's slice
        out["validation %d: an unseen key inside a block with records" % i] = any(
            np.any(x["gk"] >= 0) and np.any(x["gk"] < 0) for x in cs)
    out["validation 0: a block with entries but no record"] = any(
        x["n"] > 0 and not np.any(x["gk"] >= 0) for x in (R.share_census(ref, ref.va[0], b) for b in range(len(ref.ranges))))
    out["validation 1: a block with no entry"] = any(
        R.share_census(ref, ref.va[1], b)["n"] == 0 for b in range(len(ref.ranges)))
    return out


# ---- case E: the branches of k_bcd_update.  Small values: h is small, the steps run into the clamps and the cap
E_BLOCKS = [[80, 120, 30, 60, 200], [40, 150, 25, 90], [10, 3, 100, 1, 2, 4, 6, 8, 5, 7]]
E_ZERO_KEY = 3           # all its values are 0.0: g = h = 0
E_SCALE = 0.05
E_PASSES = 6


def _case_e(l1):
    chunk, ranges = R.designed_chunk(E_BLOCKS, 300, seed=51, zero_keys=(E_ZERO_KEY,), scale=E_SCALE)
    return Case([chunk], ranges, list(range(len(ranges))) * E_PASSES, l1=l1, lr=.8)


@functools.lru_cache(None)
def case_e():
    return _case_e(.03)


@functools.lru_cache(None)
def case_e_l1_zero():
    return _case_e(0.)


E_BRANCHES = {"pos": "g_pos <= u w", "neg": "g_neg >= u w", "zero_nz": "neither, with w != 0", "zero_z": "neither, with w == 0",
              "clamp_lo": "the lower clamp", "clamp_hi": "the upper clamp", "cap": "delta capped at 5", "h0": "h == 0"}


def _run_ref(case, ref, each=None):
    """the restatement alone through the case's steps; each(blk, g, h, w, delta): called before every update"""
    for blk in case.steps:
        pb, pe = ref.pos[blk]
        if each:
            g, h = ref.grad(blk)
            each(blk, g.astype(np.float32), h.astype(np.float32), ref.w[pb:pe].copy(), ref.delta[pb:pe].copy())
        ref.step(blk)


def cond_e(case, ref):
    seen = {k: False for k in E_BRANCHES}
    seen["negzero"] = False

    def each(blk, g, h, w, delta):
        for k, m in R.update_census(g, h, w, delta, ref.l1, ref.lr).items():
            seen[k] |= bool(m.any())
    _run_ref(case, ref, each)
    if ref.l1 == 0:
        return {"l1 = 0: a step of -0.0": seen["negzero"], "h == 0": seen["h0"]}
    return {"update branch: " + E_BRANCHES[k]: seen[k] for k in E_BRANCHES}


# ---- case F: the epoch form on B's and D's layouts, rows in bands, dyadic values (see the head of this file)
F_ORDER_B = [1, 3, 0, 2]      # the largest block directly before the smallest
F_ORDER_D = [1, 3, 0, 2]


@functools.lru_cache(None)
def case_f_b():
    c = _case_b(True)
    c.steps = F_ORDER_B
    return c


@functools.lru_cache(None)
def case_f_d():
    c = _case_d(True)
    c.steps = F_ORDER_D
    return c


def _first_touch(ref, blk):
    """every prediction the gradient of blk reads is still 0"""
    pb, pe = ref.pos[blk]
    return all(not np.any(c.pred[c.row[(c.gk >= pb) & (c.gk < pe)]]) for c in ref.tr)


def cond_f(case, ref, base):
    out = dict(base(case, ref))
    order = case.steps
    nk = [ref.pos[b][1] - ref.pos[b][0] for b in order]
    nz = [sum(R.share_census(ref, c, b)["n"] for c in ref.tr) for b in order]
    out["a non-identity order over every block"] = sorted(order) == list(range(len(ref.ranges))) and order != sorted(order)
    out["the block of most entries runs directly before the one of fewest"] = nz.index(max(nz)) + 1 == nz.index(min(nz))
    out["a block of more keys runs directly before one of fewer, and the reverse"] = (
        any(a > b for a, b in zip(nk, nk[1:])) and any(a < b for a, b in zip(nk, nk[1:])))
    touch = True
    for blk in order:
        touch &= _first_touch(ref, blk)
        ref.step(blk)
    out["every gradient of the first epoch reads pred = 0"] = bool(touch)
    out["the first epoch moves the model"] = bool(np.count_nonzero(ref.w) >= 5) and all(np.any(c.pred) for c in ref.tr + ref.va)
    vals = np.concatenate([c.val for c in ref.tr])
    out["values are multiples of 2^-10 below 2^3"] = bool(np.all(vals * 1024 == np.round(vals * 1024)) and np.abs(vals).max() < 8)
    return out


CASES = {
    "A": (case_a, cond_a),
    "B": (case_b, cond_b),
    "C": (case_c, cond_c),
    "C-mixed": (case_c_mixed, cond_c),
    "D": (case_d, cond_d),
    "E": (case_e, cond_e),
    "E-l1-zero": (case_e_l1_zero, cond_e),
    "F-B": (case_f_b, lambda case, ref: cond_f(case, ref, cond_b)),
    "F-D": (case_f_d, lambda case, ref: cond_f(case, ref, cond_d)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_edges(name):
    """CPU only: the restatement alone through the case's steps, and the census conditions of the case"""
    make, cond = CASES[name]
    case = make()
    ref = case.ref()
    out = cond(case, ref)
    if not name.startswith(("E", "F")):      # those two run the steps inside their conditions
        _run_ref(case, ref)
    missed = [k for k, v in out.items() if not v]
    assert not missed, "case %s misses: %s" % (name, "; ".join(missed))
    assert np.all(np.isfinite(ref.w)) and np.count_nonzero(ref.w) > 0
    for c in case.train + case.val:          # the row order is not the key order
        keys = R.reverse_bytes_np(c[1]).astype(np.int64)
        rows = np.repeat(np.arange(len(c[0]) - 1), np.diff(c[0].astype(np.int64)))
        assert np.any((rows[1:] == rows[:-1]) & (keys[1:] < keys[:-1])), "case %s: rows list their keys in ascending order" % name


def test_designed_chunk_layout():
    """the builder: raw ids are reverse_bytes(1, 2, 3, ...), counts and ranges as asked, options as described"""
    blocks = [[3, 0, 5], [2, 4]]
    (off, ids, val, lab), ranges = R.designed_chunk(blocks, 40, seed=1, dup=(3,), empty_rows=6, solo=(4,), zero_keys=(5,))
    assert ranges == [(1, 4), (4, 6)]
    keys = R.reverse_bytes_np(ids)
    assert [R.reverse_bytes(int(i)) for i in ids] == [int(k) for k in keys]
    assert np.array_equal(np.bincount(keys.astype(np.int64), minlength=6)[1:], [3, 0, 5, 2, 4])
    rows = np.repeat(np.arange(40), np.diff(off.astype(np.int64)))
    assert len(np.unique(rows[keys == 3])) == 4 and len(np.unique(rows[keys == 1])) == 3
    assert np.all(np.diff(off.astype(np.int64))[-6:] == 0)
    assert all(np.sum(rows == r) == 1 for r in rows[keys == 4])
    assert np.all(val[keys == 5] == 0) and np.all(val[keys != 5] != 0)
    (_, _, val_b, _), _ = R.designed_chunk(blocks, 40, seed=1, binary=True)
    assert val_b is None
    (off2, ids2, val2, _), _ = R.designed_chunk(blocks, 40, seed=1, bands=True, dyadic=True)
    rows2 = np.repeat(np.arange(40), np.diff(off2.astype(np.int64)))
    k2 = R.reverse_bytes_np(ids2)
    assert rows2[k2 < 4].max() < rows2[k2 >= 4].min()
    assert np.all(val2 * 1024 == np.round(val2 * 1024))


def test_update_census_partitions_the_branches():
    g = np.array([-1, 1, .05, .05, -9, 9, 0], np.float32)
    h = np.array([1, 1, 1, 1, 1, 1, 0], np.float32)
    w = np.array([0, 0, 0, .001, 0, 0, 0], np.float32)
    delta = np.array([5, 5, 1, 1, 1, 3, 1], np.float32)
    c = R.update_census(g, h, w, delta, .1, 1.)
    assert list(c["pos"]) == [1, 0, 0, 0, 1, 0, 0] and list(c["neg"]) == [0, 1, 0, 0, 0, 1, 0]
    assert list(c["zero_z"]) == [0, 0, 1, 0, 0, 0, 1] and list(c["zero_nz"]) == [0, 0, 0, 1, 0, 0, 0]
    assert list(c["clamp_hi"]) == [0, 0, 0, 0, 1, 0, 0] and list(c["clamp_lo"]) == [0, 0, 0, 0, 0, 1, 0]
    assert list(c["cap"]) == [0, 0, 0, 0, 0, 1, 0] and list(c["h0"]) == [0, 0, 0, 0, 0, 0, 1]
    assert np.all(c["pos"] ^ c["neg"] ^ c["zero_z"] ^ c["zero_nz"])
    z = R.update_census(np.zeros(1), np.ones(1), np.zeros(1), np.ones(1), 0., 1.)
    assert z["negzero"][0] and R.update_weight(np.zeros(1), np.ones(1), np.zeros(1), np.ones(1), 0., 1.)[2].view(np.uint32)[0] == 1 << 31


# ---- on the device

def _step_case(capi, ctx, case, after=None):
    ref = case.ref()
    o = case.device(capi, ctx)
    try:
        assert o.nkeys == len(ref.keys)
        assert np.array_equal(o.get_model()["keys"], ref.keys)
        for blk in case.steps:
            R.check_block(o, ref, blk)
        if after:
            after(o, ref)
    finally:
        o.close()


@gpu
@pytest.mark.parametrize("name", ["A", "B", "C", "C-mixed", "E", "E-l1-zero"])
def test_block_steps_on_designed_inputs(capi, ctx, name):
    _step_case(capi, ctx, CASES[name][0]())


def _auc_n(chunks):
    """sum over the chunks, in order, of n max(area, 1 - area): area from a stable argsort, in fp64"""
    tot = 0.0
    for c in chunks:
        pos = c.lab[np.argsort(c.pred, kind="stable")] > 0
        area = np.cumsum(pos)[~pos].sum() / (pos.sum() * (c.n - pos.sum()))
        tot += c.n * max(area, 1 - area)
    return tot


def _check_progress(prog, ref):
    """prog {count, objv, AUC x n, accuracy} against the restatement in ref's present state"""
    cnt, objv, acc = ref.progress()
    n = sum(c.n for c in ref.tr + ref.va)
    assert prog[0] == cnt == n
    assert prog[3] == acc, (prog[3], acc)
    assert abs(prog[1] - objv) <= 1e-5 * objv, (prog[1], objv)
    assert abs(prog[2] - _auc_n(ref.tr + ref.va)) < 1e-4 * n, (prog[2], _auc_n(ref.tr + ref.va))


@gpu
def test_validation_chunks_and_progress(capi, ctx):
    """case D: after every step all four chunks' pred bit for bit (check_block); then the progress of one more step"""
    def after(o, ref):
        blk = 0
        for c, p in zip(ref.tr + ref.va, R.device_preds(o, ref)):
            assert R.same_bits(p, c.pred)
        _, _, prog = o.step(blk, progress=True)
        for c, p in zip(ref.tr + ref.va, R.device_preds(o, ref)):
            c.pred = p.copy()
        _check_progress(prog, ref)
    _step_case(capi, ctx, case_d(), after)


@gpu
@pytest.mark.parametrize("name", ["F-B", "F-D"])
def test_epoch_form_first_touch_is_bit_exact(capi, ctx, name):
    case = CASES[name][0]()
    ref = case.ref()
    o = case.device(capi, ctx)
    try:
        prog = o.epoch(case.steps)
        for blk in case.steps:
            ref.step(blk)
        m = o.get_model()
        assert np.array_equal(m["keys"], ref.keys)
        for k, want in (("w", ref.w), ("delta", ref.delta), ("dw", ref.dw)):
            assert R.same_bits(m[k], want), "%s not bit-identical after the first epoch" % k
        for i, (c, p) in enumerate(zip(ref.tr + ref.va, R.device_preds(o, ref))):
            assert R.same_bits(p, c.pred), "pred of chunk %d (training first) not bit-identical" % i
        _check_progress(prog, ref)
        # the second epoch is no longer first touch: the bound of test_empty_blocks_and_epochs
        prog = o.epoch(case.steps)
        for blk in case.steps:
            ref.step(blk)
        cnt, objv, _ = ref.progress()
        assert prog[0] == cnt
        assert np.allclose(prog[1], objv, rtol=1e-5, atol=0), (prog[1], objv)
    finally:
        o.close()
