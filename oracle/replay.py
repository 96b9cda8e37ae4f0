"""Recorded answers of the reference build (oracle/_ref).  TEST INFRASTRUCTURE ONLY.

oracle/_ref is compiled from the reference's own sources and exists only where those sources do.  The tests that
compare against it get, elsewhere, the answers it gave when they were recorded: tests/golden/ref_replay.pkl.gz maps
a test's node id to the sequence of its calls on the reference (method, digest of the arguments, returned value).

  * Recorder wraps a live Ref (and the RefStores it creates) and appends every call to the test's sequence;
  * Replay answers the same calls in the same order, and fails a call whose arguments differ from the recorded ones
    (the test changed: record again with DIFACTO_REF_RECORD=1 where oracle/_ref is built).
"""
import copy
import gzip
import hashlib
import os
import pickle

import numpy as np

RECORDING = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                         "ref_replay.pkl.gz")
_OBJECT = "<object>"


def _feed(h, a):
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    elif isinstance(a, (list, tuple)):
        h.update(b"(")
        for x in a:
            _feed(h, x)
        h.update(b")")
    else:
        h.update(repr(a).encode())


def digest(name, args, kw):
    h = hashlib.sha1(name.encode())
    _feed(h, list(args))
    for k in sorted(kw):
        h.update(k.encode())
        _feed(h, kw[k])
    return h.hexdigest()


def _plain(v):
    if v is None or isinstance(v, (np.ndarray, np.generic, int, float, str, bytes, bool)):
        return True
    if isinstance(v, (list, tuple)):
        return all(_plain(x) for x in v)
    if isinstance(v, dict):
        return all(_plain(x) for x in v.values())
    return False


class Recorder:
    def __init__(self, target, calls):
        self._target, self._calls = target, calls

    def __getattr__(self, attr):
        v = getattr(self._target, attr)
        if not callable(v):
            self._calls.append(("." + attr, digest("." + attr, (), {}), copy.deepcopy(v)))
            return v

        def call(*args, **kw):
            out = v(*args, **kw)
            d = digest(attr, args, kw)
            if _plain(out):
                self._calls.append((attr, d, copy.deepcopy(out)))
                return out
            self._calls.append((attr, d, _OBJECT))
            return Recorder(out, self._calls)
        return call


class Replay:
    def __init__(self, calls, nodeid, cursor=None):
        self._calls, self._nodeid = calls, nodeid
        self._cursor = cursor if cursor is not None else [0]

    def _next(self, name, d):
        i = self._cursor[0]
        assert i < len(self._calls), "%s: call %d (%s) beyond the recorded reference calls" % (self._nodeid, i, name)
        rname, rd, value = self._calls[i]
        assert (rname, rd) == (name, d), ("%s: call %d is %s with other arguments than the recorded %s; record the reference's "
                                          "answers again" % (self._nodeid, i, name, rname))
        self._cursor[0] = i + 1
        return value

    def __getattr__(self, attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        if self._cursor[0] < len(self._calls) and self._calls[self._cursor[0]][0] == "." + attr:
            return copy.deepcopy(self._next("." + attr, digest("." + attr, (), {})))

        def call(*args, **kw):
            value = self._next(attr, digest(attr, args, kw))
            return Replay(self._calls, self._nodeid, self._cursor) if isinstance(value, str) and value == _OBJECT \
                else copy.deepcopy(value)
        return call


def load(path=RECORDING):
    if not os.path.exists(path):
        return {}
    with gzip.open(path, "rb") as f:
        return pickle.load(f)


def save(recorded, path=RECORDING):
    """merge the sequences of the tests that ran into the recording"""
    all_ = load(path)
    all_.update(recorded)
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        pickle.dump(dict(sorted(all_.items())), f, protocol=4)
