"""Shared by tests/test_rank.py and tests/test_gpu_rank.py: the fixture tests/golden/rank.npz
(gen_golden_rank.py) and restatements of the specification of sd_diverse_rank (include/skeldiff.h)."""
import numpy as np

from conftest import golden

RANK_CASES = 3  # rank{c}_pred / _target / _idx
STORER_BATCH = 64


def fixture():
    return golden("rank")


def dist64(points):
    """(N, N) float64 distances of the rows of `points` (N, ...), from differences"""
    x = np.asarray(points, dtype=np.float64).reshape(len(points), -1)
    return np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))


def greedy(d, n, anchor=0):
    """The farthest-point greedy on a distance matrix d (N, N) whose point 0 is the anchor (or, with
    `anchor` = 1 + closest, whose row `anchor` stands in for it): NaN ranks below every number, the
    lowest index wins a tie, min keeps a NaN.  -> (picks (n,), scores (n,)) in d's dtype."""
    N = d.shape[0]
    m = d[anchor].copy()
    free = np.ones(N, bool)
    free[0] = False
    picks, scores = [], []
    for _ in range(n):
        key = np.where(np.isnan(m), -1.0, m)  # distances are >= 0
        key = np.where(free, key, -2.0)
        c = int(np.argmax(key))  # the first maximum
        picks.append(c - 1)
        scores.append(m[c])
        free[c] = False
        m = np.where(np.isnan(m) | np.isnan(d[c]), np.nan, np.minimum(m, d[c])).astype(d.dtype)
    return np.array(picks, dtype=np.int64), np.array(scores, dtype=d.dtype)


def closest(d):
    """first index of the minimum of d[0, 1:], NaN ranking above every number"""
    return int(np.argmin(np.where(np.isnan(d[0, 1:]), np.inf, d[0, 1:])))


def cmd_float64(motion, cls, ref):
    """(value, motion_per_class (C, W), bound of the reference's float32 means) of the class-wise CMD
    (cmd.py:15-31) in float64; bound = 8 * 2^-24 * sum_c w_c sum_t (T - t) |M_ct|"""
    motion, cls = np.asarray(motion, dtype=np.float64), np.asarray(cls)
    C, W = len(ref), motion.shape[1]
    weights = np.arange(W, 0, -1, dtype=np.float64)  # T - t for t = 1 .. T - 1, T = W + 1
    per_class = np.zeros((C, W))
    value = bound = 0.0
    for c in range(C):
        mask = cls == c
        if mask.sum() == 0:
            continue
        per_class[c] = motion[mask].sum(0) / mask.sum()
        w = mask.sum() / len(cls)
        value += float((weights * np.abs(per_class[c] - ref[c])).sum()) * w
        bound += float((weights * np.abs(per_class[c])).sum()) * w
    return value, per_class, 8 * 2.0 ** -24 * bound
