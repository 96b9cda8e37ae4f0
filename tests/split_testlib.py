"""Host-side arithmetic of the update's split role (k_update_fused, upd_split_role) and minibatch generators that reach it.

A key with more than HOT_SPLIT_MIN occurrences in a minibatch is cut into parts of HOT_SPLIT occurrences; every part is one
entry of the batch object's split list.  What the list must hold after a training step can be computed from the Localizer's
counts alone, which is what makes the tests of the list deterministic.
"""
import numpy as np

HOT_SPLIT = 1024        # dfh_internal.h
HOT_SPLIT_MIN = 4096


def split_entries_expected(seglens):
    """entries a training step lists: the sum over the segments longer than HOT_SPLIT_MIN of ceil(len / HOT_SPLIT)"""
    n = np.asarray(seglens).astype(np.int64)
    n = n[n > HOT_SPLIT_MIN]
    return int(((n + HOT_SPLIT - 1) // HOT_SPLIT).sum())


def split_cap(max_nnz):
    """entries the split list of a batch object created for max_nnz pairs can hold (dfh_batch_create)"""
    return 2 * (int(max_nnz) // HOT_SPLIT) + 16


def hot_batch(rng, nrows, hot, n_other=(2, 6), id_lo=100, id_hi=40000, binary=False, labels01=False):
    """nrows rows; key `id` of hot = [(id, fraction or exact count), ...] sits in that share of the rows (an int: in exactly
    that many, the first ones), and every row carries n_other[0] .. n_other[1] - 1 ids drawn from [id_lo, id_hi) beside them"""
    member = []
    for _, f in hot:
        if isinstance(f, (int, np.integer)):
            m = np.zeros(nrows, bool)
            m[:int(f)] = True
        else:
            m = rng.random(nrows) < f
        member.append(m)
    rows_idx, off = [], [0]
    for i in range(nrows):
        ids = [h for (h, _), m in zip(hot, member) if m[i]]
        ids += list(rng.integers(id_lo, id_hi, size=int(rng.integers(n_other[0], n_other[1]))))
        rows_idx.append(np.array(ids, np.uint64))
        off.append(off[-1] + len(ids))
    idx = np.concatenate(rows_idx)
    val = None if binary else (rng.normal(size=len(idx)) * 0.3).astype(np.float32)
    lab = np.where(rng.random(nrows) < 0.3, 1.0, 0.0 if labels01 else -1.0).astype(np.float32)
    return dict(offset=np.array(off, np.uint64), index=idx, value=val, label=lab)
