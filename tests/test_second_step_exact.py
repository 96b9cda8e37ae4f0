"""The step after a step, bit for bit: what step t + 1 reads of what step t wrote.

Every other exact test starts from an imported model and stops after one update.  Here the pinned training step of an
exact-sum design (exact_step_design.py, test_update_exact.expected) is followed, on the model it left — generic, full
mantissas — by the two things that still have one right answer:

  the probe       a validation step on one-key rows, one per key of the design: the logit is fl(w x), clamped at V_dim > 0,
                  with the w of AFTER the update — the {row, w} word the lookup leaves in uw for the forward.  In the same
                  batch object and in a second one, under single_queue = 1, upd_kernel = 0, with the probe prepared (Localizer
                  and lookup, set_pipeline(1)) BEFORE the training step runs, and on rank 1 of a sharded step, under the sync
                  schedule and under the overlap schedule, where the own keys' words come through k_lookup_uw_remote's fold.
                  A key with V: the forward takes x^2 v^2 - fl(x^2 v^2) in one fma (it is compiled with contraction), so the
                  accepted floats are those of the interval
                  exact_step_design.probe_logits derives from the model; a w of before the step lies outside it for every key
                  the step moved (asserted on the CPU).
  a second step   a training step whose gradient is exact again (exact_step_design.second_minibatch): the model after it, and
                  at V_dim = 0 after a third, equals the oracle's two and three pushes, every field of every key as bits: the
                  header, the V row and the accumulators the update reads are those the step before wrote.  V_dim = 0: the
                  design's own rows (every role, the split role included); V_dim > 0: {driver, key} rows (gV = 0 exactly, the
                  update's V_l2 V and accumulators still run on the V and accumulator of step 1) and list rows of keys without V
                  on both sides of BWD_SMALL and BWD_MID; the logits (-+20) are compared too.

Not pinned: the V-dependent logits of a second step (a sum of generic terms is not order-free), and the second step's loss
at V_dim = 0 (its terms are generic).
"""
import numpy as np
import pytest

import exact_step_design as X
import test_sharded_exact as T
import test_update_exact as E
from scripted_peers import ScriptedPeers

same_bits, bits = E.same_bits, E.bits
VDIMS = E.SWITCH_VDIMS
CASES = [(V_dim, push_cnt) for V_dim in VDIMS for push_cnt in (False, True)]
IDS = ["V%d-%s" % (k, "cnt" if c else "nocnt") for k, c in CASES]


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


# ------------------------------------------------------------------ the oracle's walk
_PLANS = {}


def plan(oracle, D):
    """-> dict(first = expected(D), P = the probe, lo / hi = its accepted logits on the model after step 1, M = the second
    minibatch, steps = [dict(gw, gV, pred, lens, pulled_rows = (vals, lens) the step sees, model = (scal, has_V, V) of D's keys
    after it)] for the second and the third step).  push_cnt applies to the first step only (the reference's epoch 0)"""
    from oracle import bindings as ob
    if id(D) in _PLANS:
        return _PLANS[id(D)]
    k = D["V_dim"]
    first = E.expected(oracle, D)
    so = E._poked_store(oracle, D)
    if D["push_cnt"]:
        so.push(D["keys"], ob.FEA_COUNT, D["cnt"])
    so.push(D["keys"], ob.GRADIENT, X.ragged_gradient(first["gw"], first["gV"], first["lens"], k), first["lens"] if k else None)
    m1 = E.oracle_model(so, D["keys"], k)
    for a, b in zip(m1, first["model"]):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    P = X.probe(D)
    lo, hi = X.probe_logits(P, m1, stale_w=D["scal"][:, 1])
    M = X.second_minibatch(D, m1[1] != 0)
    steps = []
    for _ in range(2):
        pulled = so.pull(M["keys"])
        lens = pulled[1] if k else np.ones(len(M["keys"]), np.int32)
        w, V, has = X._dense(M, pulled)
        G = X.second_step_check(M, w, V, has)
        so.push(M["keys"], ob.GRADIENT, X.ragged_gradient(G["gw"], G["gV"], lens, k), lens if k else None)
        assert so.size() == len(D["keys"])
        steps.append(dict(G, lens=lens, pulled=np.array(pulled[0], np.float32), model=E.oracle_model(so, D["keys"], k)))
    out = dict(first=first, m1=m1, P=P, lo=lo, hi=hi, M=M, steps=steps)
    _PLANS[id(D)] = out
    return out


@pytest.mark.parametrize("V_dim,push_cnt", CASES, ids=IDS)
def test_second_step_designs_hold_their_conditions(oracle, V_dim, push_cnt):
    """CPU: on the oracle's weights after the pinned step — the probe's products are exact, fl((x v)^2) == fl(v^2) x^2, the
    accepted logits are one float wherever the key has no V and an interval of a few floats elsewhere, and the w of before
    the step lies outside it for every key the step moved; in the second and the third step the drivers still dominate by the
    design's margin, every row is saturated or confident, gw is an exact grid sum and gV is exactly 0
    (exact_step_design.second_step_check); the second minibatch reaches every list role"""
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt)
    pl = plan(oracle, D)
    P, M = pl["P"], pl["M"]
    assert len(P["label"]) == len(D["keys"]) and set(np.abs(P["x"]).tolist()) == {0.5, 1.0, 2.0}
    exact = bits(pl["lo"]) == bits(pl["hi"])
    has1 = pl["m1"][1][P["key_of_row"]] != 0
    assert np.array_equal(exact | has1, np.ones(len(exact), bool)) and exact.sum() >= (len(exact) if V_dim == 0 else 40)
    # an interval holds a handful of floats: the keys with V whose |w x| is small beside sum v^2
    width = (pl["hi"].astype(np.float64) - pl["lo"]) / np.maximum(np.spacing(np.maximum(np.abs(pl["lo"]), np.abs(pl["hi"]))), 1e-45)
    assert width.max() <= (0 if V_dim == 0 else 4096), width.max()
    cnt = M["cnt"].astype(np.int64)
    if V_dim == 0:
        assert {1, 2, 8, 9, 64, 65, 129, 257, 4096, 4097, 5121} <= set(cnt.tolist())
    else:
        assert set(X.SECOND_LIST_LENGTHS) <= set(cnt.tolist()) and cnt.max() > X.BWD_MID
        assert np.array_equal(M["sub"], np.arange(len(D["keys"])))
    # the second step moves the model, the third moves it again: a step that read stale state cannot leave the same bits
    a, b, c = pl["m1"][0], pl["steps"][0]["model"][0], pl["steps"][1]["model"][0]
    touched = np.isin(np.arange(len(D["keys"])), M["sub"])
    assert (bits(a[:, 2]) != bits(b[:, 2]))[touched].mean() > 0.9 and (bits(b[:, 2]) != bits(c[:, 2]))[touched].mean() > 0.9


# ------------------------------------------------------------------ the fused path
def _load(bt, B, table=None, lookup=False):
    bt.load_host(B["offset"], B["index"], B["value"], B["label"])
    if table is not None and not lookup:
        bt.localize(table=table)
    else:
        bt.localize()
        if lookup:
            bt.lookup(table)


def run_fused(capi, D, pl, options=(), probe_batch="same", prep=None, steps=2):
    """the design's pinned step, the probe as a validation step, then `steps` training steps on the second minibatch, on a
    context of its own -> dict(model1, probe, probe_model, pred2 [steps], models [steps], progress of the probe's batch).
    probe_batch "same": the batch object that ran the step is reloaded with the probe; "second": another one.  prep "lookup" /
    "fused": set_pipeline(1) and the probe prepared in the second batch object — Localizer, then Batch.lookup or the probing
    emit pass — BEFORE the training step is queued, as the worker loops do"""
    k = D["V_dim"]
    P, M = pl["P"], pl["M"]
    c = capi.Context(0)
    objs = []
    try:
        for name, v in options:
            c.set_option(name, v)
        if prep:
            c.set_pipeline(1)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **D["hyper"])
        objs.append(tb)
        tb.import_(D["keys"], D["scal"], D["has_V"], D["V"] if k else None)
        cap = (max(len(D["label"]), len(P["label"])), max(len(D["index"]), len(P["index"])) + 64)
        bt = capi.Batch(c, *cap)
        objs.append(bt)
        b2 = bt
        if probe_batch == "second" or prep:
            b2 = capi.Batch(c, *cap)
            objs.append(b2)
        for b_ in {id(bt): bt, id(b2): b2}.values():
            b_.set_option("compute_auc", 1)
        _load(bt, D)
        if prep:
            _load(b2, P, table=tb, lookup=prep == "lookup")
        bt.sgd_step(tb, is_train=True, push_cnt=D["push_cnt"])
        out = {}
        if not prep:
            out["model1"] = E.device_model(tb)
            bt.progress(reset=True)
            _load(b2, P)
        b2.sgd_step(tb, is_train=False, push_cnt=False)
        out["probe"] = b2.pred().copy()
        out["probe_model"] = E.device_model(tb)
        out["pred2"], out["models"] = [], []
        for _ in range(steps):
            _load(bt, M)
            bt.sgd_step(tb, is_train=True, push_cnt=False)
            out["pred2"].append(bt.pred().copy())
            tb.check()
            out["models"].append(E.device_model(tb))
        return out
    finally:
        for o in objs[::-1]:
            o.close()
        c.close()


def assert_probe(got, pl, what):
    lo, hi = pl["lo"], pl["hi"]
    g = np.ascontiguousarray(got, np.float32)
    exact = bits(lo) == bits(hi)
    same_bits(g[exact], lo[exact], "%s: the probe's logits against fl(w x) of the model after the step" % what)
    bad = ~((g >= lo) & (g <= hi))
    assert not bad.any(), "%s: the probe's logit leaves the accepted floats at %d keys with V; first got %r, accepted [%r, %r]" % (
        what, bad.sum(), g[bad][0], lo[bad][0], hi[bad][0])


def assert_model(model, wmodel, D, what):
    keys, scal, has, V = model
    assert np.array_equal(keys, D["keys"]), "%s: the steps added or lost keys" % what
    E._assert_model((scal, has, V), wmodel, D, what)


def assert_fused(got, D, pl, what):
    k = D["V_dim"]
    if "model1" in got:
        assert_model(got["model1"], pl["m1"], D, "%s: after the first step" % what)
    assert_probe(got["probe"], pl, what)
    assert_model(got["probe_model"], pl["m1"], D, "%s: after the probe (a validation step)" % what)
    for i, (model, st) in enumerate(zip(got["models"], pl["steps"])):
        w = "%s: after training step %d" % (what, i + 2)
        if k:
            same_bits(got["pred2"][i], st["pred"], "%s: logits" % w)
        assert_model(model, st["model"], D, w)


FUSED_SWITCHES = {
    "default": {},
    "second_batch": dict(probe_batch="second"),
    "upd_kernel0": dict(options=(("upd_kernel", 0),)),
    "upd_split0": dict(options=(("upd_split", 0),)),
    "single_queue": dict(options=(("single_queue", 1),)),
    "single_queue_second_batch": dict(options=(("single_queue", 1),), probe_batch="second"),
    "prep_lookup": dict(prep="lookup"),
    "prep_fused": dict(prep="fused"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", CASES, ids=IDS)
def test_probe_and_second_step_on_the_fused_path(capi, oracle, V_dim, push_cnt):
    """the pinned step, the probe, a second and a third training step on the same keys through dfh_sgd_step: the default path,
    the probe in a second batch object, upd_kernel = 0, upd_split = 0, single_queue = 1, and the probe prepared ahead of the
    training step on a preparation stream (its lookup runs before the update: the step has to read w again)"""
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt)
    pl = plan(oracle, D)
    for name, kw in FUSED_SWITCHES.items():
        assert_fused(run_fused(capi, D, pl, steps=2 if V_dim == 0 or name == "default" else 1, **kw), D, pl, name)


# ------------------------------------------------------------------ rank 1 of a sharded job
class _Relay:
    """the communicator's callback: the script of the step under way"""

    def __init__(self):
        self.peers = None

    def exchange(self, *a):
        return self.peers.exchange(*a)


def _rows_by_step(capi, D, pl):
    """[U, stride] per step: the rows the other owners answer with — the model before the first step, after it for the probe
    and the second step"""
    k = D["V_dim"]
    stride = capi.row_stride(k)
    first = pl["first"]
    rows1 = T.exchange_rows(first["pulled"], first["lens"], k, stride)
    s1, h1, V1 = pl["m1"]
    rowsm = np.zeros((len(D["keys"]), stride), np.float32)
    rowsm[:, 0] = s1[:, 1]
    rowsm[h1 != 0, 1] = 1.0
    if k:
        rowsm[:, 4:4 + k] = V1[:, :k] * (h1 != 0)[:, None]
    return rows1, rowsm, rowsm


def run_rank1(capi, D, pl, options=()):
    """rank 1 of 3 with scripted peers: the pinned step, the probe as a validation step, the second training step.  The rows
    the other owners answer with are the oracle's of the moment: the model before the first step, after it (probe, second
    step)"""
    k = D["V_dim"]
    keys = D["keys"]
    off = T.key_ranges(D)
    lo, hi = off[1], off[2]
    stride = capi.row_stride(k)
    P, M = pl["P"], pl["M"]
    rows1, rowsm, _ = _rows_by_step(capi, D, pl)

    def script(rows_all, push_cnt, train):
        def rows_of(p, sent):
            i = np.searchsorted(keys, sent)
            assert np.array_equal(keys[i], sent)
            return rows_all[i]
        return ScriptedPeers(1, T.W, stride, push_cnt, train, rows_of=rows_of)

    relay = _Relay()
    c = capi.Context(0)
    objs = []
    try:
        for name, v in options:
            c.set_option(name, v)
        comm = capi.Comm.callback(c, 1, T.W, relay.exchange)
        objs.append(comm)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **D["hyper"])
        objs.append(tb)
        tb.import_(keys[lo:hi], D["scal"][lo:hi], D["has_V"][lo:hi], D["V"][lo:hi] if k else None)
        bt = capi.Batch(c, max(len(D["label"]), len(P["label"])), max(len(D["index"]), len(P["index"])) + 64)
        objs.append(bt)
        bt.set_option("compute_auc", 1)
        sh = capi.Shard(tb, comm, keys[[off[1], off[2]]])
        objs.append(sh)
        out = dict(off=off, sent=[])
        for B, rows_all, push_cnt, train in ((D, rows1, D["push_cnt"], True), (P, rowsm, False, False), (M, rowsm, False, True)):
            relay.peers = script(rows_all, push_cnt, train)
            _load(bt, B)
            try:
                assert sh.step(bt, is_train=train, push_cnt=push_cnt)
            except capi.DfhError:
                if relay.peers.error is not None:
                    raise relay.peers.error
                raise
            assert relay.peers.finished()
            c.sync()
            out.setdefault("pred", []).append(bt.pred().copy())
            out["sent"].append(relay.peers.sent)
            tb.check()
            out.setdefault("models", []).append(E.device_model(tb))
        out["keys2"], out["grads2"] = out["sent"][2]["KEYS"], out["sent"][2]["GRADS"]
        return out
    finally:
        for o in objs[::-1]:
            o.close()
        c.close()


def run_rank1_overlap(capi, D, pl, options=()):
    """the same three steps as one stream under the overlap schedule (two batch objects in rotation, every following
    minibatch announced): the probe's own keys get their row words from the lookup that folds the others' rows in
    (k_lookup_uw_remote), queued behind the first step's update.  A design without counts: the stream has one push_cnt"""
    from scripted_peers import StreamPeers
    assert not D["push_cnt"]
    k, keys = D["V_dim"], D["keys"]
    off = T.key_ranges(D)
    lo, hi = off[1], off[2]
    stride = capi.row_stride(k)
    stream, train = [D, pl["P"], pl["M"]], (True, False, True)
    rows = _rows_by_step(capi, D, pl)

    def rows_of_step(t):
        def rows_of(p, sent):
            i = np.searchsorted(keys, sent)
            assert np.array_equal(keys[i], sent)
            return rows[t][i]
        return rows_of

    peers = StreamPeers(1, T.W, stride, False, [dict(have=True, is_train=train[t], rows_of=rows_of_step(t)) for t in range(3)], "overlap")
    c = capi.Context(0)
    objs = []
    try:
        for name, v in options:
            c.set_option(name, v)
        comm = capi.Comm.callback(c, 1, T.W, peers.exchange)
        objs.append(comm)
        tb = capi.Table(c, 4096, V_dim=k, init_mode=capi.INIT_HASH, **D["hyper"])
        objs.append(tb)
        tb.import_(keys[lo:hi], D["scal"][lo:hi], D["has_V"][lo:hi], D["V"][lo:hi] if k else None)
        cap = (max(len(B["label"]) for B in stream), max(len(B["index"]) for B in stream) + 64)
        bts = [capi.Batch(c, *cap) for _ in range(2)]
        objs += bts
        sh = capi.Shard(tb, comm, keys[[off[1], off[2]]])
        objs.append(sh)
        sh.set_exchange("overlap")

        def prepare(t):
            _load(bts[t % 2], stream[t])
            return bts[t % 2]

        out = dict(off=off, pred=[], models=[])
        cur = prepare(0)
        for t in range(3):
            nxt = prepare(t + 1) if t + 1 < 3 else None
            if nxt is not None:
                sh.prefetch_counts(nxt)
            try:
                assert sh.step(cur, is_train=train[t], push_cnt=False)
            except capi.DfhError:
                if peers.error is not None:
                    raise peers.error
                raise
            assert peers.done_steps(t + 1), "step %d stopped after %d exchanges of %r" % (t, peers.pos, peers.steps)
            c.sync()
            out["pred"].append(cur.pred().copy())
            tb.check()
            out["models"].append(E.device_model(tb))
            cur = nxt
        assert peers.finished()
        out["keys2"], out["grads2"] = peers.sent[(2, "KEYS")], peers.sent[(2, "GRADS")]
        return out
    finally:
        for o in objs[::-1]:
            o.close()
        c.close()


def assert_rank1(got, D, pl, name):
    V_dim = k = D["V_dim"]
    M, st = pl["M"], pl["steps"][0]
    off = got["off"]
    lo, hi = off[1], off[2]
    mine = lambda m: tuple(x[lo:hi] for x in m)
    T.assert_shard(got["models"][0], D["keys"][lo:hi], mine(pl["m1"]), V_dim, "%s: after the first step" % name, D["cnt"][lo:hi])
    assert_probe(got["pred"][1], pl, "%s, rank 1" % name)
    T.assert_shard(got["models"][1], D["keys"][lo:hi], mine(pl["m1"]), V_dim, "%s: after the probe" % name)
    if V_dim:
        same_bits(got["pred"][2], st["pred"], "%s: logits of the second step" % name)
    # the gradient rows of the second step, for the keys of ranks 0 and 2 in the second minibatch
    owner = np.searchsorted(np.array(off[1:3]), M["sub"], side="right")
    for p in (0, 2):
        sel = owner == p
        g = got["grads2"][p]
        want = np.zeros((int(sel.sum()), g.shape[1]), np.float32)
        want[:, 0] = st["gw"][sel]
        want[st["lens"][sel] > 1, 1] = 1.0
        assert np.array_equal(got["keys2"][p], M["keys"][sel])
        same_bits(g, want, "%s: GRADS of the second step to rank %d" % (name, p))
    T.assert_shard(got["models"][2], D["keys"][lo:hi], mine(st["model"]), V_dim, "%s: after the second step" % name)


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim,push_cnt", CASES, ids=IDS)
def test_probe_and_second_step_on_rank_1(capi, oracle, V_dim, push_cnt):
    """rank 1 of 3 against scripted peers, under the mixed update, shard_mixed_update = 0 and upd_kernel = 0: after the pinned
    step the probe's logits — own keys through the rank's lookup, the others' from the rows the script answers with — then the
    second training step: the gradient rows sent for the others' keys and the rank's own shard, every word"""
    D = E.design(X.FULL_LENGTHS, V_dim, False, push_cnt)
    pl = plan(oracle, D)
    for name, options in (("mixed", ()), ("mixed_update0", (("shard_mixed_update", 0),)), ("upd_kernel0", (("upd_kernel", 0),))):
        assert_rank1(run_rank1(capi, D, pl, options), D, pl, name)


@pytest.mark.gpu
@pytest.mark.parametrize("V_dim", VDIMS)
def test_probe_and_second_step_on_rank_1_overlap_schedule(capi, oracle, V_dim):
    """the same three steps as a stream under the overlap schedule, default and single_queue = 1: the probe's own keys are
    looked up by k_lookup_uw_remote, folded with the others' rows"""
    D = E.design(X.FULL_LENGTHS, V_dim, False, False)
    pl = plan(oracle, D)
    for name, options in (("overlap", ()), ("overlap, single_queue", (("single_queue", 1),))):
        assert_rank1(run_rank1_overlap(capi, D, pl, options), D, pl, name)
