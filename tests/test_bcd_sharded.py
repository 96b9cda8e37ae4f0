"""learner = bcd over several ranks (dfh_bcd_create_sharded, shard_rows=1): every rank a worker for its part of the rows
and, block by block, the server of one slice of the block's keys; the model replicated.  The ranks share the one GPU of
the test box, through DIFACTO_COMM=file (the CLI) or a gloo callback communicator (the C ABI); at most 4 ranks per test.

The C-ABI checks run inside the ranks (torch.multiprocessing.spawn ends every rank when one of them raises); every wait
is bounded by the process group's timeout or by a deadline on the CLI's processes."""
import datetime
import hashlib
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bcd_ref as R  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
PG_TIMEOUT = datetime.timedelta(seconds=120)
DIAG_ARGS = ["l1=.1", "lr=.05", "block_ratio=.001", "tail_feature_filter=0", "max_num_epochs=10"]
MULTI_ARGS = ["l1=.1", "lr=.8", "block_ratio=1", "tail_feature_filter=0"]


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


# ------------------------------------------------------------------------------------------------ refusals (no GPU)
def _refused(built, env):
    return subprocess.run([os.path.join(built, "difacto"), "learner=bcd", "shard_rows=1", "data_in=" + DATA], capture_output=True,
                          text=True, timeout=120, env=env)


def test_shard_rows_without_rendezvous_names_what_is_missing(built):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="1")
    env.pop("DIFACTO_RENDEZVOUS", None)
    r = _refused(built, env)
    assert r.returncode != 0
    assert "shard_rows=1 needs the complete environment of a rank" in r.stderr and "DIFACTO_RENDEZVOUS is not set" in r.stderr


def test_shard_rows_without_any_rank_env_names_all_of_it(built):
    env = {k: v for k, v in os.environ.items() if k not in ("DMLC_ROLE", "DMLC_NUM_WORKER", "DIFACTO_RANK", "DIFACTO_RENDEZVOUS")}
    r = _refused(built, env)
    assert r.returncode != 0 and "DMLC_ROLE, DMLC_NUM_WORKER, DIFACTO_RANK, DIFACTO_RENDEZVOUS is not set" in r.stderr


def test_shard_rows_with_a_server_role_is_refused(built):
    env = dict(os.environ, DMLC_ROLE="server", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_RENDEZVOUS="/nonexistent")
    r = _refused(built, env)
    assert r.returncode != 0 and "DMLC_ROLE=server: this build runs workers only" in r.stderr


# ------------------------------------------------------------------------------------------------ the C ABI
def _bits(*arrays):
    return hashlib.sha1(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def _slice(p, n, world):
    return p * n // world


class Rank:
    """what a scenario gets: its place, the device context, the callback communicator over gloo"""

    def __init__(self, rank, world, dist, capi):
        import torch
        self.rank, self.world, self.dist, self.capi = rank, world, dist, capi
        self.ctx = capi.Context(0)

        def exchange(send, sb, recv, rb):
            out = torch.empty(sum(rb), dtype=torch.uint8)
            dist.all_to_all_single(out, torch.from_numpy(np.array(send, copy=True)), output_split_sizes=rb, input_split_sizes=sb)
            recv[:] = out.numpy()

        self.comm = capi.Comm.callback(self.ctx, rank, world, exchange)

    def gather(self, x):
        out = [None] * self.world
        self.dist.all_gather_object(out, x)
        return out

    def sharded(self, mine, ranges, val=(), **kw):
        """a sharded object over this rank's chunks"""
        o = self.capi.Bcd(self.ctx, comm=self.comm)
        for c in mine:
            o.add_chunk(*c)
        for c in val:
            o.add_chunk(*c, is_val=True)
        o.build(ranges, **kw)
        return o


def _spawned(rank, world, port, scenario, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)
    from difacto_amd import capi
    rk = Rank(rank, world, dist, capi)
    globals()[scenario](rk, out_dir)
    rk.comm.close()
    rk.ctx.close()
    dist.barrier()
    dist.destroy_process_group()


def _spawn(scenario, world, tmp_path):
    import torch.multiprocessing as mp
    port = 29600 + (os.getpid() % 300) + world
    # join: a rank that raises ends the others, so none of them is left waiting in a collective
    mp.spawn(_spawned, args=(world, port, scenario, str(tmp_path)), nprocs=world, join=True)


def _check_block(rk, o, ref, blk, first, ntrain, nval):
    """R.check_block's criterion on a sharded object: ref holds every rank's chunks in rank order (training, then
    validation), this rank's are ref.tr[first[0] : first[0] + ntrain] and ref.va[first[1] : first[1] + nval].  The ranks
    swap their predictions; -> g, h"""
    mine = [o.get_pred(i) for i in range(ntrain)], [o.get_pred(i, is_val=True) for i in range(nval)]
    every = rk.gather(mine)
    for c, p in zip(ref.tr, [p for t, _ in every for p in t]):
        c.pred = p.copy()
    for c, p in zip(ref.va, [p for _, v in every for p in v]):
        c.pred = p.copy()
    m = o.get_model()
    assert np.array_equal(m["keys"], ref.keys)
    ref.w, ref.delta = m["w"].copy(), m["delta"].copy()
    g_want, h_want, g_mag, h_mag = ref.grad(blk, mag=True)
    g, h, _ = o.step(blk, grad=True)
    assert np.all(np.abs(g - g_want) <= 1e-6 * g_mag), np.max(np.abs(g - g_want) / np.maximum(g_mag, 1e-300))
    assert np.all(np.abs(h - h_want) <= 1e-6 * h_mag), np.max(np.abs(h - h_want) / np.maximum(h_mag, 1e-300))
    pb, pe = ref.pos[blk]
    w, d, dw = R.update_weight(g.astype(np.float32), h.astype(np.float32), ref.w[pb:pe], ref.delta[pb:pe], ref.l1, ref.lr)
    m2 = o.get_model()
    assert R.same_bits(m2["w"][pb:pe], w) and R.same_bits(m2["delta"][pb:pe], d) and R.same_bits(m2["dw"][pb:pe], dw)
    out = np.r_[0:pb, pe:len(ref.w)]   # the other blocks' keys stay as they were
    assert R.same_bits(m2["w"][out], ref.w[out]) and R.same_bits(m2["delta"][out], ref.delta[out])
    ref.w, ref.delta, ref.dw = m2["w"].copy(), m2["delta"].copy(), m2["dw"].copy()
    ref.update_pred(blk)
    for i in range(ntrain):
        assert R.same_bits(o.get_pred(i), ref.tr[first[0] + i].pred), "pred of training chunk %d not bit-identical" % i
    for i in range(nval):
        assert R.same_bits(o.get_pred(i, is_val=True), ref.va[first[1] + i].pred), "pred of validation chunk %d" % i
    # the replicated model and the returned sums: the same bits on every rank
    digests = rk.gather(_bits(m2["w"], m2["delta"], m2["dw"], g, h))
    assert len(set(digests)) == 1, digests
    return g, h


def _state(o, ntrain, nval=0):
    m = o.get_model()
    return _bits(m["w"], m["delta"], m["dw"], *[o.get_pred(i) for i in range(ntrain)],
                 *[o.get_pred(i, is_val=True) for i in range(nval)])


def _rcv1_chunks(world):
    """rcv1_100 split unevenly over the ranks, two chunks per rank -> (all chunks in rank order, rows per chunk)"""
    d = R.read_libsvm(DATA)
    edges = {1: [0, 100], 2: [0, 37, 100], 3: [0, 21, 64, 100]}[world]
    rows = []
    for r in range(world):
        n = edges[r + 1] - edges[r]
        rows += [n // 3, n - n // 3]
    return R.split_rows(*d, rows), rows


def scenario_world1(rk, out_dir):
    """one rank over the callback transport against the plain object on the same chunks: every bit, and no wire bytes"""
    parts, _ = _rcv1_chunks(1)
    train, val = parts[:1], parts[1:]
    ref = R.BCD(train, val, l1=.1, lr=.8, block_ratio=.2, tail_feature_filter=1)
    kw = dict(tail_feature_filter=1, l1=.1, lr=.8)
    a = R.make_device(rk.capi, rk.ctx, train, ref.ranges, val=val, **{"tail": 1, "l1": .1, "lr": .8})
    b = rk.sharded(train, ref.ranges, val=val, **kw)
    assert a.nkeys == b.nkeys == len(ref.keys) and len(ref.ranges) >= 10
    rk.comm.stats(reset=True)
    for blk in range(len(ref.ranges)):
        ga, ha, _ = a.step(blk, grad=True)
        gb, hb, _ = b.step(blk, grad=True)
        assert _bits(ga, ha) == _bits(gb, hb), blk
        assert _state(a, 1, 1) == _state(b, 1, 1), blk
    order, stream = list(range(len(ref.ranges))), R.RefRand()
    for _ in range(3):
        stream.shuffle(order)
        pa, pb = a.epoch(order), b.epoch(order)
        assert _bits(pa) == _bits(pb) and pa[0] == 100
        assert _state(a, 1, 1) == _state(b, 1, 1)
    assert np.count_nonzero(b.get_model()["w"]) > 10
    sent, recv, groups = rk.comm.stats()
    assert sent == 0 and recv == 0 and groups > 0
    a.close()
    b.close()


def scenario_rcv1(rk, out_dir):
    """worlds 2 and 3: ~30 block steps against the restatement over all ranks' chunks, a second run, the wire bytes of a
    step, set_model"""
    W, r = rk.world, rk.rank
    parts, rows = _rcv1_chunks(W)
    mine = parts[2 * r:2 * r + 2]
    kw = dict(tail_feature_filter=1, l1=.1, lr=.8)
    ref = R.BCD(parts, l1=.1, lr=.8, block_ratio=.2, tail_feature_filter=1)
    nblk = len(ref.ranges)
    assert 10 <= nblk <= 30
    steps = list(range(nblk)) + list(range(nblk))[:max(0, 30 - nblk)]   # every block, the first ones a second time
    o = rk.sharded(mine, ref.ranges, **kw)
    first = [_check_block(rk, o, ref, blk, (2 * r, 0), 2, 0) for blk in steps]
    assert np.count_nonzero(ref.w) > 10
    end = _state(o, 2)
    o.close()
    # a second run: the same bits
    o = rk.sharded(mine, ref.ranges, **kw)
    again = [o.step(blk, grad=True)[:2] for blk in steps]
    assert all(_bits(*a) == _bits(*b) for a, b in zip(first, again)) and _state(o, 2) == end
    o.close()
    # the bytes a step without g, h and progress sends: the partials of the other slices, the own slice's delta w
    o = rk.sharded(mine, ref.ranges, **kw)
    owns = set()
    for blk in range(nblk):
        pb, pe = ref.pos[blk]
        n = pe - pb
        own = _slice(r + 1, n, W) - _slice(r, n, W)
        owns.add(own)
        rk.comm.stats(reset=True)
        o.step(blk)
        assert rk.comm.stats()[0] == 16 * (n - own) + 4 * own * (W - 1), (blk, n, own)
    assert max(owns) > 1
    o.close()
    # set_model: every rank passes the same input; w and the rebuilt pred are the plain object's for the rank's chunks
    rng = np.random.default_rng(5)
    keys = rng.permutation(ref.keys)[:len(ref.keys) * 2 // 3]
    assert 1 not in ref.keys and 2 not in ref.keys
    keys = np.concatenate([keys, np.array([1, 2], np.uint64)])   # and two keys the model does not hold
    w = rng.normal(size=len(keys)).astype(np.float32)
    plain = R.make_device(rk.capi, rk.ctx, parts, ref.ranges, tail=1, l1=.1, lr=.8)
    o = rk.sharded(mine, ref.ranges, **kw)
    assert o.set_model(keys, w) == plain.set_model(keys, w) == len(keys) - 2
    assert R.same_bits(o.get_model()["w"], plain.get_model()["w"]) and np.count_nonzero(o.get_model()["w"]) > 10
    for i in range(2):
        p = o.get_pred(i)
        assert R.same_bits(p, plain.get_pred(2 * r + i)) and np.count_nonzero(p) > 0
    _check_block(rk, o, _with_state(ref, plain), 0, (2 * r, 0), 2, 0)   # and the steps go on from there
    o.close()
    plain.close()


def _with_state(ref, plain):
    m = plain.get_model()
    ref.w, ref.delta, ref.dw = m["w"].copy(), m["delta"].copy(), m["dw"].copy()
    return ref


# designed edges, three ranks.  Keys 1.. in ReverseBytes space; per block the entry count of each key, on rank 0 (a chunk
# with values), on rank 1's training chunk (binary) and on rank 1's validation chunk; rank 2 has no rows.
EDGE_A = [[9, 0, 7, 12, 5, 0, 8, 30, 3, 6, 11], [4, 3], [0, 0, 0], [6], [5, 2, 1, 0, 1, 7, 4]]
EDGE_B = [[6, 8, 0, 10, 0, 4, 9, 25, 5, 3, 0], [0, 5], [0, 0, 0], [3], [0, 1, 0, 0, 1, 6, 3]]
EDGE_V = [[3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3], [2, 2], [0, 0, 1], [2], [2, 2, 2, 2, 2, 2, 2]]
EDGE_FILTER = 2


def scenario_edges(rk, out_dir):
    W, r = rk.world, rk.rank
    assert W == 3
    a, ranges = R.designed_chunk(EDGE_A, 300, seed=1)
    b, ranges_b = R.designed_chunk(EDGE_B, 200, seed=2, binary=True)
    v, ranges_v = R.designed_chunk(EDGE_V, 60, seed=3)
    assert ranges == ranges_b == ranges_v and a[2] is not None and b[2] is None
    ref = R.bcd_with_ranges([a, b], [v], ranges, l1=.05, lr=.7, tail_feature_filter=EDGE_FILTER)
    first5 = ranges[4][0]
    sizes = [pe - pb for pb, pe in ref.pos]
    # the edges, each shown to occur in this input
    assert sizes[1] == 2 < W and _slice(1, 2, W) - _slice(0, 2, W) == 0      # fewer keys than ranks: rank 0's slice is empty
    assert sizes[3] == 1 and sizes[2] == 0                                   # one key; no key (the range holds none)
    assert sizes[0] > 2 * W                                                  # and a block with several keys per slice
    assert EDGE_A[1][0] > EDGE_FILTER and EDGE_B[1][0] == 0 and ranges[1][0] in ref.keys      # a key of rank 0's rows alone
    assert EDGE_A[0][1] == 0 and EDGE_B[0][1] > EDGE_FILTER and 2 in ref.keys                # a key of rank 1's rows alone
    k = first5 + 1   # counts 2 and 1: filtered on either rank alone, kept on the global count
    assert EDGE_A[4][1] <= EDGE_FILTER and EDGE_B[4][1] <= EDGE_FILTER < EDGE_A[4][1] + EDGE_B[4][1] and k in ref.keys
    assert first5 + 2 not in ref.keys and first5 + 4 not in ref.keys         # counts 1 + 0 and 1 + 1: filtered globally too
    assert first5 + 3 not in ref.keys                                        # a key of the validation chunk alone
    mine = ([a], [], (0, 0)) if r == 0 else ([b], [v], (1, 0)) if r == 1 else ([], [], (2, 1))
    kw = dict(tail_feature_filter=EDGE_FILTER, l1=.05, lr=.7)
    o = rk.sharded(mine[0], ranges, val=mine[1], **kw)
    assert o.nkeys == len(ref.keys)
    for blk in [0, 1, 2, 3, 4, 1, 0, 4, 3, 2]:
        _check_block(rk, o, ref, blk, mine[2], len(mine[0]), len(mine[1]))
    assert np.count_nonzero(ref.w) > 5 and ref.w[ref.pos[1][0]] != 0 and ref.w[list(ref.keys).index(k)] != 0
    # an epoch: the progress counts every rank's rows, the same bits on every rank
    p = o.epoch([4, 2, 0, 3, 1])
    assert p[0] == 300 + 200 + 60 and len(set(rk.gather(_bits(p)))) == 1
    o.close()


@pytest.mark.gpu
def test_world1_has_the_bits_of_the_plain_object(tmp_path):
    _spawn("scenario_world1", 1, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_block_steps_follow_the_restatement(tmp_path, world):
    _spawn("scenario_rcv1", world, tmp_path)


@pytest.mark.gpu
def test_designed_edges(tmp_path):
    _spawn("scenario_edges", 3, tmp_path)


# ------------------------------------------------------------------------------------------------ the command line
def _run_ranks(built, world, args, tmp_path, tag):
    """one process per rank on the one GPU, the file transport; a rank that fails or a deadline ends every rank;
    -> every rank's log"""
    rv = os.path.join(str(tmp_path), "rv_" + tag)
    os.makedirs(rv)
    logs = [open(os.path.join(str(tmp_path), "%s.%d.log" % (tag, r)), "w+") for r in range(world)]
    procs = []
    for r in range(world):
        env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER=str(world), DIFACTO_RANK=str(r), DIFACTO_DEVICE="0",
                   DIFACTO_COMM="file", DIFACTO_RENDEZVOUS=rv)
        procs.append(subprocess.Popen([os.path.join(built, "difacto"), "learner=bcd", "shard_rows=1"] + list(args), stdout=logs[r],
                                      stderr=subprocess.STDOUT, cwd=ROOT, env=env))
    deadline = time.monotonic() + 300
    try:
        while True:
            running = [p for p in procs if p.poll() is None]
            if not running or any(p.returncode not in (None, 0) for p in procs) or time.monotonic() > deadline:
                break
            try:
                running[0].wait(timeout=0.2)
            except subprocess.TimeoutExpired:
                pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    outs = []
    for f in logs:
        f.seek(0)
        outs.append(f.read())
        f.close()
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d (exit %s): %s" % (r, p.returncode, out[-3000:])
    return outs


def _epoch_lines(log):
    return [l.split("] ", 1)[-1] for l in log.splitlines() if re.search(r"epoch: \d+, objv: ", l)]


def _objv(log):
    return [float(x) for x in re.findall(r"epoch: \d+, objv: (\S+),", log)]


def _logged_split(logs):
    """the training rows and chunks of every rank, from its own log line"""
    out = []
    for r, log in enumerate(logs):
        m = re.search(r"rank %d: (\d+) training examples in (\d+) chunks" % r, log)
        out.append((int(m.group(1)), int(m.group(2))))
    return out


def _restated(logs, epochs, **kw):
    """R.BCD on the ranks' row split -> objv per row and epoch, as the log prints it"""
    split = _logged_split(logs)
    assert sum(n for n, _ in split) == 100 and all(c == (1 if n else 0) for n, c in split), split
    parts = R.split_rows(*R.read_libsvm(DATA), [n for n, _ in split if n])
    return [float(np.float32(v) / np.float32(100)) for v in R.BCD(parts, **kw).run(epochs, R.RefRand())], split


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_cli_diag_newton_lockstep_and_repeatable(built, tmp_path, world):
    logs = _run_ranks(built, world, ["data_in=" + DATA] + DIAG_ARGS, tmp_path, "a")
    lines = _epoch_lines(logs[0])
    assert len(lines) == 10
    for r in range(1, world):
        assert _epoch_lines(logs[r]) == lines, r
    assert all("loaded 100 examples" in l for l in logs)
    want, split = _restated(logs, 10, l1=.1, lr=.05, block_ratio=.001, tail_feature_filter=0)
    assert sum(1 for n, _ in split if n) >= 2
    np.testing.assert_allclose(_objv(logs[0]), want, rtol=1e-5, atol=0)
    again = _run_ranks(built, world, ["data_in=" + DATA] + DIAG_ARGS, tmp_path, "b")
    assert all(_epoch_lines(l) == lines for l in again)


@pytest.mark.gpu
def test_cli_many_blocks_follow_the_restatement(built, tmp_path):
    logs = _run_ranks(built, 2, ["data_in=" + DATA, "max_num_epochs=8"] + MULTI_ARGS, tmp_path, "m")
    want, _ = _restated(logs, 8, l1=.1, lr=.8, block_ratio=1, tail_feature_filter=0)
    assert re.search(r"partitioning feature into (\d+) blocks", logs[0]) and "partitioning feature into 1 blocks" not in logs[0]
    assert _epoch_lines(logs[1]) == _epoch_lines(logs[0])
    np.testing.assert_allclose(_objv(logs[0]), want, rtol=1e-4, atol=0)


@pytest.mark.gpu
def test_cli_model_out_scores_with_sgd_predict(built, tmp_path):
    """rank 0's one model file scored by task=predict learner=sgd against the final predictions of the same block steps
    on the ranks' split (the C ABI on the logged split's chunks)"""
    from difacto_amd import capi
    model, pred = str(tmp_path / "m"), str(tmp_path / "p")
    logs = _run_ranks(built, 2, ["data_in=" + DATA, "max_num_epochs=5", "model_out=" + model] + MULTI_ARGS, tmp_path, "s")
    assert "model saved to" in logs[0] and "model saved to" not in logs[1]
    assert os.path.exists(model) and not os.path.exists(model + ".part-0") and not os.path.exists(model + ".parts")
    r = subprocess.run([os.path.join(built, "difacto"), "task=predict", "learner=sgd", "data_in=" + DATA, "V_dim=0",
                        "batch_size=100", "model_in=" + model, "pred_out=" + pred], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.loadtxt(pred, dtype=np.float64)
    split = [n for n, _ in _logged_split(logs)]
    assert len(split) == 2 and min(split) > 0
    parts = R.split_rows(*R.read_libsvm(DATA), split)
    ref = R.BCD(parts, l1=.1, lr=.8, block_ratio=1, tail_feature_filter=0)
    ctx = capi.Context(0)
    o = R.make_device(capi, ctx, parts, ref.ranges, l1=.1, lr=.8, tail=0)
    try:
        order, stream = list(range(len(ref.ranges))), R.RefRand()
        for _ in range(5):
            stream.shuffle(order)
            o.epoch(order)
        want = np.concatenate([o.get_pred(i) for i in range(2)]).astype(np.float64)
        assert np.count_nonzero(o.get_model()["w"]) > 10
    finally:
        o.close()
        ctx.close()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
