"""The sharded step, bit for bit: k_update_fused<..., MIXED = true>, k_forward<MIXED>, k_uw_remote and the owner side
inside a real dfh_shard_step.

One process is rank r of a 3-rank job whose peers are a script (scripted_peers.py, through capi.Comm.callback): nothing waits
for another process, and a wrong size fails the step.  The minibatches are the exact-sum designs of exact_step_design.py, so
every byte the rank sends and every field it leaves in its shard has exactly one right value (test_update_exact.expected):
no tolerance, no mask, no skipped key.

  case A  the worker side: all three ranks of a design in turn, the peers announcing no keys.  Every key goes through the
          remote path (a gradient row [gw, has_V, 0, 0 | gV, padding] for its owner) twice and through the own path (the
          in-place update) once.
  case B  rank 1 under every switch of the step and under the hyper-parameter variants: the same bytes.
  case C  the owner side: both peers also send keys of rank 1's range (keys of the minibatch with and without V, keys the
          table has never seen, keys BOTH peers send) with arbitrary full-mantissa gradient rows; one oracle store takes the
          documented order (own count push, the peers' in rank order, the pull, the own keys' gradient, the peers' in
          ascending rank) and the rows the rank answers with and its whole shard must equal it.

This file pins the SYNC schedule, one step.  The overlap schedule — two minibatches in flight, a stream of three steps on
disjoint key sets — is pinned the same way in test_sharded_overlap_exact.py.  Every step here is also held to the one right
Progress of its design (test_update_exact.assert_step_progress): a rank's penalty is that of ALL keys of its minibatch, own and
pulled, each counted once — by the MIXED update, or with shard_mixed_update = 0 by the gradient-row launch (KeyRange.inv = 3)
and the own keys' launch — so it equals the fused step's, bit for bit under the "pen" variant.  A second step on the SAME keys
on rank 1 is pinned in test_second_step_exact.py.  Not pinned: the V-dependent logits of such a step, the zero rows' loss at
V_dim = 0, l2's penalty term beside the drivers.
"""
import numpy as np
import pytest

import exact_step_design as X
import test_update_exact as E
from scripted_peers import ScriptedPeers
from split_testlib import HOT_SPLIT_MIN, split_entries_expected

same_bits, bits = E.same_bits, E.bits
W = 3
# occurrences of a key in the minibatch -> the role of k_update_fused that takes it (singles tile, few, mid, hot, split)
CLASSES = (("one occurrence", 1, 1), ("2..8", 2, 8), ("9..64", 9, 64), ("65..4096", 65, HOT_SPLIT_MIN), ("more than 4096", HOT_SPLIT_MIN + 1, 1 << 30))


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


# ------------------------------------------------------------------ the key ranges
def split_ok(cnt, off):
    """the conditions on the ranges off = [0, a, b, U]: per class of occurrences SOME rank has both an own and a remote key
    (two remote ones of one occurrence: the singles tile compacts them side by side), and some rank has remote keys on both
    sides of its range"""
    U = len(cnt)
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    if not any(off[r] > 0 and off[r + 1] < U and off[r + 1] > off[r] for r in range(len(off) - 1)):
        return False
    for _, a, b in CLASSES:
        m = (cnt >= a) & (cnt <= b)
        if not any((m & (owner == r)).any() and (m & (owner != r)).sum() >= (2 if b == 1 else 1) for r in range(len(off) - 1)):
            return False
    return True


def key_ranges(D):
    """[0, a, b, U]: thirds of the key list, moved by as little as it takes where a design's thirds miss split_ok"""
    cnt = D["cnt"].astype(np.int64)
    U = len(cnt)
    t = (U // 3, 2 * U // 3)
    for _, a, b in sorted((abs(a - t[0]) + abs(b - t[1]), a, b) for a in range(1, U - 1) for b in range(a + 1, U)):
        if split_ok(cnt, [0, a, b, U]):
            return [0, a, b, U]
    raise AssertionError("no pair of split keys gives every class an own and a remote key")


def exchange_rows(vals, lens, k, stride):
    """the ragged values of Store::Pull -> the rows of the exchange [w, has_V, 0, 0 | V, zero padding]"""
    n = len(lens)
    out = np.zeros((n, stride), np.float32)
    pos = np.cumsum(lens) - lens
    if n:
        out[:, 0] = vals[pos]
    out[lens > 1, 1] = 1.0
    for j in np.flatnonzero(lens > 1):
        out[j, 4:4 + k] = vals[pos[j] + 1:pos[j] + 1 + k]
    return out


# ------------------------------------------------------------------ case C: what the peers send rank 1
def owner_plan(D, off, r=1, seed=0):
    """-> dict(keys {p: u64}, cnt {p: f32 ones}, unseen): the keys peers 0 and 2 send rank r, all inside its range.  Keys of
    the minibatch of class V and of class N, chosen among those whose count stays BELOW V_threshold with the step's own
    count push and both peers' (the peers' pushes then leave every weight the design's check() saw as it was; the designed
    trigger keys, classes Z and C, are not sent), and keys the table has never seen; some of each kind come from both peers"""
    rng = np.random.default_rng([seed, D["V_dim"], int(D["push_cnt"])])
    keys, cls = D["keys"], D["cls"]
    lo, hi = off[r], off[r + 1]
    own = np.arange(lo, hi)
    fea1 = D["scal"][:, 0].astype(np.float64) + (D["cnt"] if D["push_cnt"] else 0)
    quiet = fea1[own] + 2 < D["hyper"]["V_threshold"]
    pick = {}
    for c in "VN":
        cand = own[(cls[own] == c) & quiet]
        assert len(cand) >= 3, "rank %d owns %d usable keys of class %s" % (r, len(cand), c)
        pick[c] = rng.permutation(cand)[:9]
    # keys of rank r's range the table has never seen: the successor of an own key (ids are 63 random bits: it is free)
    at = np.array([lo + 1, (lo + hi) // 2, hi - 2, hi - 1 if hi < len(keys) else hi - 3])
    unseen = np.unique(keys[at] + np.uint64(1))
    assert len(unseen) == 4 and not np.isin(unseen, keys).any() and unseen.min() > keys[lo]
    assert hi == len(keys) or unseen.max() < keys[hi]
    out = {}
    for p, (a, b) in ((0, (0, 3)), (2, (1, 4))):
        # of each class the first third from both peers, the others from one of them in turn
        mine = np.concatenate([np.concatenate([v[:len(v) // 3], v[len(v) // 3:][p // 2::2]]) for v in (pick["V"], pick["N"])])
        out[p] = np.unique(np.concatenate([keys[mine], unseen[a:b]]))
    both = np.intersect1d(out[0], out[2])
    idx = np.searchsorted(keys, both[np.isin(both, keys)])
    assert {"V", "N"} <= set(cls[idx]) and np.isin(unseen, both).sum() == 2, "both peers must share a key of every kind"
    for p in out:
        i = np.searchsorted(keys, out[p][np.isin(out[p], keys)])
        assert set(cls[i]) == {"V", "N"} and np.all((i >= lo) & (i < hi))
    # the condition: with every count of the step added no chosen key reaches V_threshold
    sent = np.concatenate([out[0], out[2]])
    known = np.isin(sent, keys)
    tot = np.bincount(np.searchsorted(keys, sent[known]), minlength=len(keys))
    chosen = tot > 0
    added = tot if D["push_cnt"] else 0
    assert np.all((fea1 + added)[chosen] < D["hyper"]["V_threshold"]) and tot.max() == 2
    return dict(keys=out, cnt={p: np.ones(len(out[p]), np.float32) for p in out}, unseen=unseen)


CASE_C = [(V_dim, push_cnt) for V_dim in (0, 5, 64) for push_cnt in (False, True)]


# ================================================================== CPU: the conditions
@pytest.mark.parametrize("V_dim", E.STEP_VDIMS)
@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_key_ranges_give_every_class_an_own_and_a_remote_key(V_dim, binary, push_cnt):
    """CPU: with the chosen split keys some rank has both an own and a remote key among the keys of one occurrence (two remote
    ones), of 2..8, 9..64, 65..4096 and more than 4096, and rank 1 has remote keys on both sides of its range"""
    D = E.design(X.FULL_LENGTHS, V_dim, binary, push_cnt)
    off = key_ranges(D)
    cnt, U = D["cnt"].astype(np.int64), len(D["keys"])
    assert off[0] == 0 and off[3] == U and 0 < off[1] < off[2] < U      # own_lo > 0 and own_hi < U for rank 1
    assert abs(off[1] - U // 3) + abs(off[2] - 2 * U // 3) <= U // 3, "the ranges are far from thirds: %r of %d" % (off, U)
    owner = np.repeat(np.arange(W), np.diff(off))
    for name, a, b in CLASSES:
        m = (cnt >= a) & (cnt <= b)
        ok = [r for r in range(W) if (m & (owner == r)).any() and (m & (owner != r)).sum() >= (2 if b == 1 else 1)]
        assert ok, "no rank has an own and a remote key of %s" % name
    assert split_entries_expected(D["cnt"]) == 5 + 6


@pytest.mark.parametrize("variant", ["l1_0", "Vl2_0", "beta", "pen"])
def test_key_ranges_of_the_variant_designs(variant):
    """CPU: the same for the designs of the hyper-parameter variants (key_ranges raises where no ranges qualify)"""
    for V_dim in E.SWITCH_VDIMS:
        for push_cnt in (False, True):
            D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt, variant)
            off = key_ranges(D)
            assert split_ok(D["cnt"].astype(np.int64), off) and 0 < off[1] < off[2] < len(D["keys"])


@pytest.mark.parametrize("V_dim,push_cnt", CASE_C)
def test_owner_plan_keeps_the_design_valid(oracle, V_dim, push_cnt):
    """CPU: what the peers send rank 1 in case C — keys with V, without, unseen ones, some from both peers — and that their
    count pushes leave the weights the step sees, bit for bit, what the design's check() was run on"""
    from oracle import bindings as ob
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt)
    want = E.expected(oracle, D)
    plan = owner_plan(D, key_ranges(D))
    assert len(np.intersect1d(plan["keys"][0], plan["keys"][2])) >= 4
    so = E._poked_store(oracle, D)
    if push_cnt:
        so.push(D["keys"], ob.FEA_COUNT, D["cnt"])
        for p in (0, 2):
            so.push(plan["keys"][p], ob.FEA_COUNT, plan["cnt"][p])
    vals, lens = so.pull(D["keys"])
    assert V_dim == 0 or np.array_equal(lens, want["lens"])
    same_bits(vals, want["pulled"], "the pull after the peers' count pushes against the pull check() saw")


def test_scripted_peers_refuse_a_wrong_size():
    """CPU: the script's state machine — a step of rank 1 of 3 with the right sizes passes, any other size raises"""
    stride = 12

    def play(tamper):
        sp = ScriptedPeers(1, 3, stride, True, peer_keys={0: np.array([5, 6], np.uint64)}, peer_cnt={0: np.ones(2, np.float32)},
                           rows_of=lambda p, k: np.full((len(k), stride), p, np.float32), peer_grads={0: np.ones((2, stride), np.float32)})
        nsend = [3, 0, 1]
        steps = [("COUNTS", [16] * 3, [16] * 3), ("KEYS", [24, 0, 8], [16, 0, 0]), ("CNT", [12, 0, 4], [8, 0, 0]),
                 ("ROWS", [2 * 4 * stride, 0, 0], [3 * 4 * stride, 0, 4 * stride]), ("GRADS", [3 * 4 * stride, 0, 4 * stride], [2 * 4 * stride, 0, 0])]
        for kind, sb, rb in steps:
            send = np.zeros(sum(sb), np.uint8)
            if kind == "COUNTS":
                send[:] = np.array([[nsend[0], 1], [7, 1], [nsend[2], 1]], np.int64).view(np.uint8).reshape(-1)
            if kind == tamper:       # four bytes more for rank 0
                sb = [sb[0] + 4] + sb[1:]
                send = np.concatenate([send, np.zeros(4, np.uint8)])
            recv = np.zeros(sum(rb), np.uint8)
            sp.exchange(send, sb, recv, rb)
            if kind == "COUNTS":
                assert recv.view(np.int64).reshape(3, 2).tolist() == [[2, 1], [7, 1], [0, 1]]
            if kind == "ROWS":
                assert recv.view(np.float32).reshape(4, stride)[:, 0].tolist() == [0, 0, 0, 2]
        assert sp.finished()
        with pytest.raises(AssertionError):
            sp.exchange(np.zeros(48, np.uint8), [16] * 3, np.zeros(48, np.uint8), [16] * 3)

    play(None)
    for kind in ("COUNTS", "KEYS", "CNT", "ROWS", "GRADS"):
        with pytest.raises(AssertionError):
            play(kind)


# ================================================================== one rank, one step
def run_rank(capi, D, rows_all, r, off, options=(), plan=None, peer_grads=None):
    """rank r of W on a context of its own: the design's model of the rank's own keys imported, the whole minibatch loaded and
    localized, one training step over a communicator whose peers are the script.  rows_all [U, stride]: the rows the other
    owners answer with, by rank of the key.  -> dict(pred, split_entries, model = (keys, scal, has_V, V), peers)"""
    k = D["V_dim"]
    keys = D["keys"]
    lo, hi = off[r], off[r + 1]
    stride = capi.row_stride(k)
    nrows, nnz = len(D["label"]), len(D["index"])

    def rows_of(p, sent):
        i = np.searchsorted(keys, sent)
        assert np.array_equal(keys[i], sent), "keys sent to rank %d that are not the minibatch's" % p
        return rows_all[i]

    peers = ScriptedPeers(r, W, stride, D["push_cnt"], True, rows_of=rows_of, peer_keys=plan["keys"] if plan else None,
                          peer_cnt=plan["cnt"] if plan else None, peer_grads=peer_grads)
    c = capi.Context(0)
    objs = []       # closed in reverse: the shard before its table and communicator
    try:
        for name, v in options:
            c.set_option(name, v)
        comm = capi.Comm.callback(c, r, W, peers.exchange)
        objs.append(comm)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **D["hyper"])
        objs.append(tb)
        tb.import_(keys[lo:hi], D["scal"][lo:hi], D["has_V"][lo:hi], D["V"][lo:hi] if k else None)
        bt = capi.Batch(c, nrows, nnz + 64)
        objs.append(bt)
        bt.set_option("compute_auc", 1)       # as the sharded learner sets it
        bt.load_host(D["offset"], D["index"], D["value"], D["label"])
        bt.localize()
        sh = capi.Shard(tb, comm, keys[[off[1], off[2]]])
        objs.append(sh)
        try:
            active = sh.step(bt, is_train=True, push_cnt=D["push_cnt"])
        except capi.DfhError:
            if peers.error is not None:
                raise peers.error
            raise
        assert active and peers.finished(), "the step stopped after %d exchanges of %r" % (peers.pos, peers.plan)
        c.sync()
        reads = [bt.progress(reset=False), bt.progress(reset=False)]
        out = dict(pred=bt.pred().copy(), split_entries=bt.split_entries(), peers=peers, progress=bt.progress(reset=True))
        out["reads"] = reads + [bt.progress(reset=False)]
        tb.check()
        out["model"] = E.device_model(tb)
        assert tb.size() == len(out["model"][0])
        return out
    finally:
        for o in objs[::-1]:
            o.close()
        c.close()


def pulled_rows(capi, D, want):
    return exchange_rows(want["pulled"], want["lens"], D["V_dim"], capi.row_stride(D["V_dim"]))


def grad_rows_expected(capi, D, want):
    """[U, stride]: [gw, has_V as pulled, 0, 0 | gV (zeros for a key pulled without V), zero padding]"""
    k = D["V_dim"]
    g = np.zeros((len(D["keys"]), capi.row_stride(k)), np.float32)
    g[:, 0] = want["gw"]
    g[want["lens"] > 1, 1] = 1.0
    if k:
        assert not bits(want["gV"][want["lens"] == 1]).any()
        g[:, 4:4 + k] = want["gV"]
    return g


def assert_worker_side(capi, got, D, want, r, off, what, split=True):
    """everything rank r sent and left behind against the one right answer"""
    k, keys = D["V_dim"], D["keys"]
    lo, hi = off[r], off[r + 1]
    peers = got["peers"]
    counts = peers.counts
    assert counts.tolist() == [[off[p + 1] - off[p], 1] for p in range(W)], "%s: COUNTS words %r" % (what, counts.tolist())
    gwant = grad_rows_expected(capi, D, want)
    for p in peers.peers:
        a, b = off[p], off[p + 1]
        assert np.array_equal(peers.sent["KEYS"][p], keys[a:b]), "%s: KEYS sent to rank %d" % (what, p)
        if D["push_cnt"]:
            same_bits(peers.sent["CNT"][p], D["cnt"][a:b], "%s: CNT sent to rank %d" % (what, p))
        else:
            assert "CNT" not in peers.sent
        g = peers.sent["GRADS"][p]
        assert g.shape == gwant[a:b].shape
        same_bits(g[:, 0], gwant[a:b, 0], "%s: GRADS to rank %d, word 0 (gw); occurrences %r" % (
            what, p, D["cnt"][a:b][bits(g[:, 0]) != bits(gwant[a:b, 0])][:8].tolist()))
        same_bits(g[:, 1], gwant[a:b, 1], "%s: GRADS to rank %d, word 1 (has_V as pulled)" % (what, p))
        assert not bits(g[:, 2:4]).any(), "%s: GRADS to rank %d, words 2 and 3" % (what, p)
        if k:
            same_bits(g[:, 4:4 + k], gwant[a:b, 4:4 + k], "%s: GRADS to rank %d, the V part" % (what, p))
        assert not bits(g[:, 4 + k:]).any(), "%s: GRADS to rank %d, padding" % (what, p)
        same_bits(g, gwant[a:b], "%s: GRADS to rank %d" % (what, p))
    same_bits(got["pred"], want["pred"], "%s: logits against clip(exact)" % what)
    # the rank's progress: loss, AUC and rows of its minibatch, the penalty of ALL its keys, own and pulled, each once — what the
    # fused step returns for the same design
    if "progress" in got:     # (a step out of a stream: its batch object's sums are asserted over the stream)
        E.assert_step_progress(got, want["progress"], what)
    assert_shard(got["model"], keys[lo:hi], tuple(m[lo:hi] for m in want["model"]), k, what, D["cnt"][lo:hi])
    n = split_entries_expected(D["cnt"]) if split else 0
    assert got["split_entries"] == n and n in (0, 11), "%s: %d split entries" % (what, got["split_entries"])


def assert_shard(model, wkeys, wmodel, k, what, occ=None):
    """the whole table against (keys, (scal, has_V, V | acc)): exactly these keys, every field as bit patterns"""
    dkeys, scal, has, V = model
    assert np.array_equal(dkeys, wkeys), "%s: the table holds %d keys, %d expected" % (what, len(dkeys), len(wkeys))
    wscal, whas, wV = wmodel
    bad = (has != 0) != (whas != 0)
    assert not bad.any(), "%s: has_V differs at %d keys%s" % (what, bad.sum(), "" if occ is None else " of %r occurrences" % occ[bad][:8].tolist())
    for j, name in enumerate(("fea_cnt", "w", "sqrt_g", "z")):
        bad = bits(scal[:, j]) != bits(wscal[:, j])
        assert not bad.any(), "%s: %s differs at %d keys%s; first got %r want %r" % (
            what, name, bad.sum(), "" if occ is None else " of %r occurrences" % np.unique(occ[bad]).tolist(), scal[bad, j][0], wscal[bad, j][0])
    if k:
        same_bits(V[:, :k], wV[:, :k], "%s: V" % what)
        same_bits(V[:, k:], wV[:, k:], "%s: accumulators" % what)


# ================================================================== case A
@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", E.STEP_VDIMS)
@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_worker_side_every_rank_bit_exact(capi, oracle, V_dim, binary, push_cnt):
    """ranks 0, 1 and 2 of one design in turn (k_uw_remote, k_forward<MIXED>, k_update_fused<..., MIXED>): the keys, counts and
    gradient rows sent, the logits, the shard and the split list, every word of them.  (V_dim 1 and 4 are the regression
    cases of the singles tile's -0: padded coordinates, and a true coordinate of a single-occurrence key where XV_d = 0)"""
    D = E.design(X.FULL_LENGTHS, V_dim, binary, push_cnt)
    want = E.expected(oracle, D)
    off = key_ranges(D)
    rows_all = pulled_rows(capi, D, want)
    for r in range(W):
        assert_worker_side(capi, run_rank(capi, D, rows_all, r, off), D, want, r, off, "rank %d" % r)


# ================================================================== case B
SHARD_SWITCHES = {
    "mixed_update0": dict(options=(("shard_mixed_update", 0),)),          # a launch for the others' keys, one for the own
    "upd_kernel0": dict(options=(("upd_kernel", 0),), split=False),       # k_backward_all for both
    "upd_split0": dict(options=(("upd_split", 0),), split=False),
    "hot_blocks1": dict(options=(("upd_hot_blocks", 1),)),
    "hot_blocks8": dict(options=(("upd_hot_blocks", 8),)),
    "single_queue": dict(options=(("single_queue", 1),)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", E.SWITCH_VDIMS)
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_every_switch_gives_the_same_bytes(capi, oracle, V_dim, push_cnt):
    """rank 1 of 3 under shard_mixed_update = 0, upd_kernel = 0, upd_split = 0, upd_hot_blocks = 1 and 8 and single_queue = 1:
    the default run's logits, gradient rows and shard, and each against the oracle"""
    _switch_matrix(capi, oracle, E.design(X.FULL_LENGTHS, V_dim, False, push_cnt))


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", E.SWITCH_VDIMS)
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_every_switch_gives_the_same_penalty(capi, oracle, V_dim, push_cnt):
    """the same on the "pen" design, whose penalty has one right float: the MIXED update (own and remote keys in one launch),
    shard_mixed_update = 0 (the gradient-row launch with KeyRange.inv = 3 for the pulled rows, then the own keys' launch: no key
    counted by both, none by neither), upd_kernel = 0 (k_backward_all for both) and the others"""
    _switch_matrix(capi, oracle, E.design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen"))


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", E.SWITCH_VDIMS)
@pytest.mark.parametrize("push_cnt", [False, True], ids=["nocnt", "cnt"])
def test_worker_side_every_rank_penalty(capi, oracle, V_dim, push_cnt):
    """ranks 0, 1 and 2 of the "pen" design: whichever third of the keys is the rank's own, the penalty is the fused step's"""
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt, "pen")
    want = E.expected(oracle, D)
    off = key_ranges(D)
    rows_all = pulled_rows(capi, D, want)
    for r in range(W):
        assert_worker_side(capi, run_rank(capi, D, rows_all, r, off), D, want, r, off, "rank %d, pen" % r)


def _switch_matrix(capi, oracle, D):
    want = E.expected(oracle, D)
    off = key_ranges(D)
    rows_all = pulled_rows(capi, D, want)
    runs = {"default": run_rank(capi, D, rows_all, 1, off)}
    for name, sw in SHARD_SWITCHES.items():
        runs[name] = run_rank(capi, D, rows_all, 1, off, options=sw["options"])
    base = runs["default"]
    for name, g in runs.items():
        same_bits(g["pred"], base["pred"], "%s against the default: logits" % name)
        for p in (0, 2):
            same_bits(g["peers"].sent["GRADS"][p], base["peers"].sent["GRADS"][p], "%s against the default: GRADS to rank %d" % (name, p))
        assert np.array_equal(g["model"][0], base["model"][0]) and np.array_equal(g["model"][2], base["model"][2]), name
        same_bits(g["model"][1], base["model"][1], "%s against the default: scalars" % name)
        same_bits(g["model"][3], base["model"][3], "%s against the default: V | acc" % name)
    for name, g in runs.items():
        assert_worker_side(capi, g, D, want, 1, off, name, split=SHARD_SWITCHES.get(name, {}).get("split", True))


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt,variant", E.VARIANT_CASES)
def test_hyper_parameter_variants_on_rank_1(capi, oracle, V_dim, push_cnt, variant):
    """l1 = 0, V_l2 = 0 and non-default lr_beta / V_lr_beta through rank 1's step, each against its own expected()"""
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt, variant)
    want = E.expected(oracle, D)
    off = key_ranges(D)
    assert_worker_side(capi, run_rank(capi, D, pulled_rows(capi, D, want), 1, off), D, want, 1, off, variant)


# ================================================================== case C
@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", CASE_C)
@pytest.mark.parametrize("per_key", [0, 1], ids=["per_entry", "per_key"])
def test_owner_side_inside_a_step_bit_exact(capi, oracle, V_dim, push_cnt, per_key):
    """rank 1 serves its peers inside its own training step (owner_per_key 0 and 1): the rows it answers with and its whole
    shard afterwards — the minibatch's keys, the keys only the peers touched and the new ones — against one oracle store
    that takes the documented order"""
    from oracle import bindings as ob
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt)
    want = E.expected(oracle, D)
    off = key_ranges(D)
    k, keys = V_dim, D["keys"]
    stride = capi.row_stride(k)
    plan = owner_plan(D, off)
    rng = np.random.default_rng(700 + V_dim + int(push_cnt))
    so = E._poked_store(oracle, D)
    # 1, 2: the own count push (the other ranks' keys of the minibatch are counted on their owners: the one store takes
    # them too), then the peers' in rank order
    if push_cnt:
        so.push(keys, ob.FEA_COUNT, D["cnt"])
        for p in (0, 2):
            so.push(plan["keys"][p], ob.FEA_COUNT, plan["cnt"][p])
    # 3: the pull
    rows_want, ragged, lens_of, grads = {}, {}, {}, {}
    for p in (0, 2):
        vals, lens = so.pull(plan["keys"][p])
        lens = lens if k else np.ones(len(plan["keys"][p]), np.int32)
        rows_want[p] = exchange_rows(vals, lens, k, stride)
        g = E._random_grad(rng, int(lens.sum()))
        ragged[p], lens_of[p] = g, lens
        grads[p] = E._rows_from_ragged(g, lens, rows_want[p][:, 1], k, stride)
        known = np.isin(plan["keys"][p], keys)
        assert k == 0 or ((lens[known] > 1).any() and (lens[known] == 1).any() and np.all(lens[~known] == 1))
    vals, _ = so.pull(keys)
    same_bits(vals, want["pulled"], "the weights the step sees")
    # 4, 5: the own keys' exact gradient, then the peers' in ascending rank
    so.push(keys, ob.GRADIENT, X.ragged_gradient(want["gw"], want["gV"], want["lens"], k), want["lens"] if k else None)
    for p in (0, 2):
        so.push(plan["keys"][p], ob.GRADIENT, ragged[p], lens_of[p] if k else None)

    got = run_rank(capi, D, pulled_rows(capi, D, want), 1, off, options=(("owner_per_key", per_key),), plan=plan, peer_grads=grads)
    what = "owner side, %s" % ("per key" if per_key else "per entry")
    for p in (0, 2):
        same_bits(got["peers"].sent["ROWS"][p], rows_want[p], "%s: ROWS answered to rank %d" % (what, p))
    # the worker side of the same step is what it is without the peers' keys: their pushes come after it
    same_bits(got["pred"], want["pred"], "%s: logits" % what)
    E.assert_step_progress(got, want["progress"], what)     # (the peers' keys are in no minibatch of this rank: not in its penalty)
    gwant = grad_rows_expected(capi, D, want)
    for p in (0, 2):
        same_bits(got["peers"].sent["GRADS"][p], gwant[off[p]:off[p + 1]], "%s: GRADS to rank %d" % (what, p))
    wkeys = np.union1d(keys[off[1]:off[2]], plan["unseen"])
    assert_shard(got["model"], wkeys, E.oracle_model(so, wkeys, k), k, what)
    assert got["split_entries"] == split_entries_expected(D["cnt"])
