"""Hand-made posterior rows for the expert-target tests (include/msexpert.h) and a numpy
restatement of the targets, shared by tests/test_expert_host.py and tests/test_expert_gpu.py."""
from __future__ import annotations

import numpy as np

SIZES = (1, 63, 64, 65, 81, 512)
TINY = float(np.nextafter(0.0, 1.0))  # the smallest positive subnormal f64
OUTPUTS = ("best", "action", "kind", "n_best", "labels")


def numpy_targets(status, prob, hidden):
    """include/msexpert.h restated: dict of best, action, kind, n_best, labels."""
    n, A = prob.shape
    out = dict(best=np.zeros((n, A), np.uint8), action=np.full(n, -1, np.int64), kind=np.zeros(n, np.uint8),
               n_best=np.zeros(n, np.int32), labels=np.zeros((n, A), np.float32))
    for i in range(n):
        h = hidden[i] != 0
        if status[i] != 1 or not h.any():
            continue
        pmin = prob[i][h].min()
        b = h & (prob[i] == pmin)
        out["best"][i], out["n_best"][i], out["action"][i] = b, b.sum(), np.flatnonzero(b)[0]
        out["kind"][i] = 1 if pmin == 0.0 else 2
        out["labels"][i] = np.where(h, prob[i], 0.0).astype(np.float32)
    return out


def hand_rows(A: int):
    """-> (status u8 [n], prob f64 [n, A], hidden u8 [n, A], names): one row per directed case."""
    rng = np.random.default_rng(A)
    rows = []

    def add(name, status, prob, hidden):
        rows.append((name, status, np.asarray(prob, np.float64), np.asarray(hidden, np.uint8)))

    ones = np.ones(A, np.uint8)
    p = rng.uniform(0.1, 0.9, A)
    q = p.copy()
    q[A - 1] = 0.05
    add("single minimum at the last cell", 1, q, ones)
    add("all hidden cells tied", 1, np.full(A, 0.3), ones)
    one = np.zeros(A, np.uint8)
    one[A // 2] = 1
    add("one hidden cell", 1, p, one)
    z = p.copy()
    z[::3] = 0.0
    add("several exact zeros: a safe move", 1, z, ones)
    s = p.copy()
    s[::3] = TINY
    add("smallest subnormal: a forced guess", 1, s, ones)
    r = p.copy()
    hid = ones.copy()
    r[0], hid[0] = 0.0, 0  # a revealed cell's 0 must not enter the minimum
    if A > 1:
        add("revealed zero", 1, r, hid)
    add("status 0", 0, p, ones)
    add("status 2", 2, p, ones)
    add("nothing hidden", 1, p, np.zeros(A, np.uint8))
    mixed = rng.uniform(0.0, 1.0, A)
    mixed[rng.integers(0, A, max(1, A // 8))] = mixed.min()
    add("random with ties", 1, mixed, rng.integers(0, 2, A))
    add("labels: exact 1 and 2^-24", 1, np.where(np.arange(A) % 2 == 0, 1.0, 2.0 ** -24), ones)
    names = [x[0] for x in rows]
    return (np.array([x[1] for x in rows], np.uint8), np.stack([x[2] for x in rows]), np.stack([x[3] for x in rows]),
            names)


def tiled(A: int, n: int):
    """The hand rows of size A repeated to exactly n rows (grids with partial tails)."""
    st, pr, hd, _ = hand_rows(A)
    idx = np.arange(n) % len(st)
    return st[idx].copy(), pr[idx].copy(), hd[idx].copy()
