"""learner = lbfgs with l1 > 0 over several ranks (dfh_lbfgs_create_sharded + dfh_lbfgs_set_l1): the orthant-wise passes run
on each rank's owned slice and every new scalar is a sum over the ranks.  As tests/test_lbfgs_sharded.py: the ranks share the
one GPU, through DIFACTO_COMM=file (the command line) or a gloo callback communicator (the C ABI); at most 4 processes."""
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import owlqn_ref as O                                               # noqa: E402
import test_lbfgs_sharded as S                                      # noqa: E402
from test_lbfgs_l1_learner import CONF, DATA, _accepted, _lines, _model    # noqa: E402

L1 = 0.05


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def problem():
    ids, X, y = O.read_libsvm(DATA)
    w, F, g = O.fista(X, y, 0.1, 0.1, tol=1e-14)
    return ids, w, g


@pytest.fixture(scope="module")
def plain_log(built):
    return S._plain(built, ["argfile=" + CONF])


@pytest.mark.gpu
def test_world1_sharded_prints_the_plain_bits(built, tmp_path, plain_log):
    one = S._run_ranks(built, 1, ["argfile=" + CONF], tmp_path, "w1")[0]
    keep = lambda log: [l for l in _lines(log) if "objv" in l or "nnz(w)" in l or "c2 is unused" in l]   # noqa: E731
    assert len(keep(plain_log)) > 20 and keep(one) == keep(plain_log)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_example_conf_over_ranks(built, tmp_path, world, plain_log, problem):
    ids, ws, gs = problem
    model = str(tmp_path / "m")
    logs = S._run_ranks(built, world, ["argfile=" + CONF, "model_out=" + model], tmp_path, "l1")
    keep = lambda log: [l for l in _lines(log) if "objv" in l or "nnz(w)" in l or "dropped" in l]   # noqa: E731
    for r in range(1, world):
        assert keep(logs[r]) == keep(logs[0]), r
    want, got = _accepted(plain_log)[1], _accepted(logs[0])[1]
    assert len(got) == len(want) >= 10
    np.testing.assert_allclose(got, want, rtol=1e-4)
    assert int(open(model + ".parts").read()) == world
    w = np.zeros(len(ids))
    for r in range(world):
        mids, mw, _, _ = _model("%s.part-%d" % (model, r))
        assert not w[np.searchsorted(ids, np.array(mids, np.uint64))].any(), "a key in two parts"
        w[np.searchsorted(ids, np.array(mids, np.uint64))] = mw
    assert 250 <= np.count_nonzero(w) <= 300
    big = np.abs(ws) >= 2e-3
    zero = 0.1 - np.abs(gs) >= 5e-4
    assert (np.sign(w[big]) == np.sign(ws[big])).all() and not w[zero].any()


def _drive(obj):
    """fixed coefficients and steps, two trials an epoch: the vectors and scalars of every epoch"""
    out = []
    obj.calc_grad()
    for ep in range(S.STATE["epochs"]):
        incr = obj.prepare_direction()
        coef = None
        if incr is not None:
            k = (len(incr) - 1) // 6
            coef = np.linspace(-0.5, 0.5, 2 * k + 1).astype(np.float32)
        pgp = obj.calc_direction(coef)
        rec = dict(incr=None if incr is None else incr.copy(), pgp=pgp, pg=obj.owlqn_vector(0), w0=obj.owlqn_vector(1),
                   p=obj.vector(2, ep), trials=[])
        for alpha in (0.5, 0.25):
            f, armijo, auc = obj.line_search(alpha if ep else alpha / 10)
            rec["trials"].append((f, armijo, auc, obj.evaluate(), obj.owlqn_moved()))
        rec["w"] = obj.get_model()["w"]
        out.append(rec)
    return out


def _ranges(n, world):
    return [(r * n // world, (r + 1) * n // world) for r in range(world)]


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from difacto_amd import capi
    ctx = capi.Context(0)

    def exchange(send, sb, recv, rb):
        out = torch.empty(sum(rb), dtype=torch.uint8)
        dist.all_to_all_single(out, torch.from_numpy(np.array(send, copy=True)), output_split_sizes=rb, input_split_sizes=sb)
        recv[:] = out.numpy()

    comm = capi.Comm.callback(ctx, rank, world, exchange)
    data = S._rcv1_rows()
    st = S.STATE
    obj = capi.Lbfgs(ctx, st["K"], st["m"], comm=comm)
    S._add_rows(obj, data, *_ranges(len(data[3]), world)[rank])      # one chunk per rank
    obj.init_model(st["filter"], st["vth"], st["scale"], st["l2"], st["V_l2"])
    obj.set_l1(L1)
    trace = _drive(obj)
    pickle.dump(trace, open(os.path.join(out_dir, "trace%d.pkl" % rank), "wb"))
    obj.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_owned_slices_concatenate_to_the_single_vectors(tmp_path, world):
    """the one-process object takes the ranks' chunks in rank order, so every element's gradient adds the same floats in
    the same order and the element-wise passes must give the same bits: pg, w0, the aligned p and w, slice by slice"""
    import torch.multiprocessing as mp
    from difacto_amd import capi
    port = 29650 + (os.getpid() % 200) + world
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    ctx = capi.Context(0)
    st = S.STATE
    one = capi.Lbfgs(ctx, st["K"], st["m"])
    data = S._rcv1_rows()
    for lo, hi in _ranges(len(data[3]), world):
        S._add_rows(one, data, lo, hi)
    one.init_model(st["filter"], st["vth"], st["scale"], st["l2"], st["V_l2"])
    one.set_l1(L1)
    lens = one.get_model()["lens"]
    single = _drive(one)
    one.close()
    ctx.close()
    assert np.any(lens > 1) and np.any(lens == 1)
    traces = [pickle.load(open(os.path.join(tmp_path, "trace%d.pkl" % r), "rb")) for r in range(world)]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731
    for ep, s in enumerate(single):
        for name in ("pg", "w0", "p", "w"):
            got = np.concatenate([t[ep][name] for t in traces])
            assert np.array_equal(bits(got), bits(s[name])), "epoch %d: %s" % (ep, name)
        assert all(len(t[ep]["pg"]) for t in traces)
        assert (s["pg"] == 0).any() and (s["p"] == 0).any() and (s["w"][lens.cumsum() - lens] == 0).any()
        for r in range(1, world):    # the same bits on every rank
            a, b = traces[0][ep], traces[r][ep]
            assert (a["incr"] is None and b["incr"] is None) or np.array_equal(a["incr"], b["incr"])
            assert a["pgp"] == b["pgp"] and a["trials"] == b["trials"]
        a = traces[0][ep]
        if s["incr"] is not None:
            np.testing.assert_allclose(a["incr"], s["incr"], rtol=1e-6, atol=1e-6 * np.abs(s["incr"]).max())
        assert a["pgp"] == pytest.approx(s["pgp"], rel=1e-6, abs=1e-9)
        for (f, arm, auc, ev, moved), (f1, arm1, auc1, ev1, moved1) in zip(a["trials"], s["trials"]):
            assert f == pytest.approx(f1, rel=1e-6) and arm == pytest.approx(arm1, rel=1e-6, abs=1e-9)
            assert ev[1] == ev1[1] and moved == moved1 and ev[2] == pytest.approx(ev1[2], rel=1e-6)
