"""Test helpers for the exact posterior (our code, shared by test_posterior_host.py and
test_posterior_gpu.py): a numpy player that places mines, flood-fills and clicks random safe
cells, and a brute-force oracle that enumerates every layout of M mines on the hidden cells as
u64 masks and keeps those that reproduce the revealed numbers. Results are integer counts, so
p = count / configs exactly (``fractions``)."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

SHAPES = ((4, 4, 3), (5, 5, 5), (4, 6, 5), (5, 5, 7), (3, 7, 4), (1, 7, 2), (5, 1, 1))
STATES_PER_SHAPE = 12
MAX_LAYOUTS = 500_000
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def popcount64(a: np.ndarray) -> np.ndarray:
    return _POP8[np.ascontiguousarray(a, dtype=np.uint64).view(np.uint8).reshape(a.shape + (8,))].sum(-1, dtype=np.int64)


def neighbours(H: int, W: int, i: int):
    r, c = divmod(i, W)
    return [rr * W + cc for rr in range(r - 1, r + 2) for cc in range(c - 1, c + 2)
            if (rr, cc) != (r, c) and 0 <= rr < H and 0 <= cc < W]


def play(H: int, W: int, M: int, seed: int, clicks=None):
    """A random consistent state: mines u8 [H, W], revealed u8 [H, W], number u8 [H, W] (the true
    count at revealed cells, garbage 200+ at hidden ones: the analysis must not read it)."""
    rng = np.random.default_rng(seed)
    A = H * W
    mine = np.zeros(A, dtype=np.uint8)
    mine[rng.choice(A, size=M, replace=False)] = 1
    count = np.array([sum(mine[j] for j in neighbours(H, W, i)) for i in range(A)], dtype=np.uint8)
    rev = np.zeros(A, dtype=np.uint8)
    for _ in range(int(rng.integers(1, 4)) if clicks is None else clicks):
        safe = np.flatnonzero((mine == 0) & (rev == 0))
        if safe.size == 0:
            break
        stack = [int(rng.choice(safe))]
        while stack:
            i = stack.pop()
            if rev[i]:
                continue
            rev[i] = 1
            if count[i] == 0:
                stack += [j for j in neighbours(H, W, i) if not rev[j]]
    number = np.where(rev == 1, count, 200 + (np.arange(A) % 50)).astype(np.uint8)
    return mine.reshape(H, W), rev.reshape(H, W), number.reshape(H, W)


def _layouts(cells, M: int) -> np.ndarray:
    """Every mask with exactly M bits among ``cells``, built cell by cell."""
    masks = np.zeros(1, dtype=np.uint64)
    bits = np.zeros(1, dtype=np.int64)
    for n, c in enumerate(cells):
        left = len(cells) - n - 1
        take = bits < M
        masks = np.concatenate((masks, masks[take] | np.uint64(1 << c)))
        bits = np.concatenate((bits, bits[take] + 1))
        keep = bits + left >= M
        masks, bits = masks[keep], bits[keep]
    return masks[bits == M]


def oracle(rev: np.ndarray, number: np.ndarray, M):
    """Brute force. M an int: layouts of exactly M mines on hidden cells; M None: any number of
    mines (what the numbers alone say). Returns (configs, counts[A]) as Python ints."""
    H, W = rev.shape
    A = H * W
    assert A <= 64
    r, num = rev.reshape(-1), number.reshape(-1)
    hidden = [i for i in range(A) if not r[i]]
    if M is None:
        assert len(hidden) <= 22
        masks = np.zeros(1, dtype=np.uint64)
        for c in hidden:
            masks = np.concatenate((masks, masks | np.uint64(1 << c)))
    else:
        assert math.comb(len(hidden), M) <= MAX_LAYOUTS
        masks = _layouts(hidden, M)
    for i in range(A):
        if r[i]:
            nb = np.uint64(sum(1 << j for j in neighbours(H, W, i)))
            masks = masks[popcount64(masks & nb) == int(num[i])]
    counts = [int(((masks >> np.uint64(i)) & np.uint64(1)).sum()) for i in range(A)]
    return int(masks.size), counts


def describe(rev: np.ndarray, number: np.ndarray, M: int):
    """What the oracle says about a state beyond p: U (hidden cells off the frontier), the number
    of components of the undetermined frontier cells (linked through a revealed cell next to
    both), and the cells decided (p = 0 or 1) only through the global mine count: undetermined
    by the numbers alone (or off the frontier), determined once the count is known."""
    H, W = rev.shape
    A = H * W
    r = rev.reshape(-1)
    configs, counts = oracle(rev, number, M)
    frontier = [i for i in range(A) if not r[i] and any(r[j] for j in neighbours(H, W, i))]
    interior = [i for i in range(A) if not r[i] and i not in frontier]
    decided = [i for i in range(A) if not r[i] and counts[i] in (0, configs)]
    loose = [i for i in frontier if i not in decided]
    parent = {i: i for i in loose}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for i in range(A):
        if r[i]:
            nb = [j for j in neighbours(H, W, i) if j in parent]
            for j in nb[1:]:
                parent[find(j)] = find(nb[0])
    n_comp = len({find(i) for i in loose})
    by_count = []
    if len(frontier) + len(interior) <= 22:
        local_n, local = oracle(rev, number, None)
        by_count = [i for i in decided if i in interior or local[i] not in (0, local_n)]
    return {"U": len(interior), "n_comp": n_comp, "by_count": by_count, "configs": configs, "counts": counts}


@functools.lru_cache(maxsize=None)
def oracle_states():
    """The oracle set: STATES_PER_SHAPE states of each of SHAPES, seeds 0, 1, ... per shape in
    order, skipping states with more than MAX_LAYOUTS layouts. Computed once per session; every
    array is read-only. Each entry: H, W, M, rev, number, mine, p (f64 [A], correctly rounded
    from the exact fraction), configs (int), and describe()'s facts."""
    out = []
    for H, W, M in SHAPES:
        seed, got = 0, 0
        while got < STATES_PER_SHAPE:
            mine, rev, number = play(H, W, M, seed=1000 * (H * W + M) + seed)
            seed += 1
            if math.comb(int((rev == 0).sum()), M) > MAX_LAYOUTS:
                continue
            d = describe(rev, number, M)
            assert d["configs"] >= 1
            d.update(H=H, W=W, M=M, rev=rev, number=number, mine=mine,
                     p=np.array([float(Fraction(c, d["configs"])) for c in d["counts"]], dtype=np.float64))
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            out.append(d)
            got += 1
    return tuple(out)


def by_shape(states):
    """{(H, W, M): stacked rev [S, H, W], number [S, H, W], p [S, A], configs [S] (float)}."""
    groups = {}
    for s in states:
        groups.setdefault((s["H"], s["W"], s["M"]), []).append(s)
    return {k: (np.stack([s["rev"] for s in v]), np.stack([s["number"] for s in v]), np.stack([s["p"] for s in v]),
                np.array([float(s["configs"]) for s in v])) for k, v in groups.items()}
