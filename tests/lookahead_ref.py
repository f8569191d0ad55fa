"""Reference for the two-guess lookahead (include/mslookahead.h), our code: the rule in numpy and
``fractions`` on top of the brute-force layout enumeration of tests/posterior_ref.py. Every layout
of M mines on the hidden cells that reproduces the revealed numbers is listed once as a u64 mask;
the layouts of the hypothetical board "c revealed showing v" are then the listed ones without a
mine on c and with v mines around it, so every Z_v, every next-move probability and every score is
an exact rational.

The candidates are a function of the f64 ``prob`` the rule is given (``prob <= pmin + margin`` and
the order are f64 comparisons by definition), so ``exact`` takes that array; everything else is
exact arithmetic.

States: ``posterior_ref.play`` positions (flood fill) and boards with an arbitrary set of safe
cells revealed, both legal inputs of the analysis. The 5x1 board with one mine has only five
guess boards among its 80 states (``all_states(5, 1, 1)``): the finished games, whose one hidden
cell is the mine. That shape contributes those five."""
from __future__ import annotations

import functools
import itertools
import math
from fractions import Fraction

import numpy as np

import posterior_ref as P

GUESS_PER_SHAPE = 30
MAX_LAYOUTS = 60_000  # per state: nine filters per candidate stay quick


def consistent_masks(rev: np.ndarray, number: np.ndarray, M: int) -> np.ndarray:
    H, W = rev.shape
    r, num = rev.reshape(-1), number.reshape(-1)
    hidden = [i for i in range(H * W) if not r[i]]
    masks = P._layouts(hidden, M)
    for i in range(H * W):
        if r[i]:
            nb = np.uint64(sum(1 << j for j in P.neighbours(H, W, i)))
            masks = masks[P.popcount64(masks & nb) == int(num[i])]
    return masks


def posterior(masks: np.ndarray, rev: np.ndarray):
    """(Z, counts[A]) of a mask list."""
    A = rev.size
    return int(masks.size), [int(((masks >> np.uint64(i)) & np.uint64(1)).sum()) for i in range(A)]


def is_guess(rev: np.ndarray, Z: int, counts) -> bool:
    hidden = [i for i in range(rev.size) if not rev.reshape(-1)[i]]
    return Z > 0 and bool(hidden) and min(counts[i] for i in hidden) > 0


def candidates(prob: np.ndarray, rev: np.ndarray, K: int, margin: float):
    """The rule's candidate list from the f64 probabilities it is given."""
    r = rev.reshape(-1)
    hidden = [i for i in range(r.size) if not r[i]]
    pmin = min(float(prob[i]) for i in hidden)
    thr = np.float64(pmin) + np.float64(margin)
    el = [i for i in hidden if np.float64(prob[i]) <= thr]
    el.sort(key=lambda i: (float(prob[i]), i))
    return el[:K]


def outcome(masks: np.ndarray, rev: np.ndarray, M: int, c: int, v: int):
    """(Z_v, t(c, v)) exactly; Z_v = 0: the outcome cannot occur."""
    H, W = rev.shape
    nb = np.uint64(sum(1 << j for j in P.neighbours(H, W, c)))
    keep = masks[(((masks >> np.uint64(c)) & np.uint64(1)) == 0) & (P.popcount64(masks & nb) == v)]
    Zv = int(keep.size)
    if Zv == 0:
        return 0, Fraction(0)
    r = rev.reshape(-1)
    hidden = [i for i in range(r.size) if not r[i] and i != c]
    if len(hidden) == M:
        return Zv, Fraction(1)
    cnt = [int(((keep >> np.uint64(i)) & np.uint64(1)).sum()) for i in hidden]
    if min(cnt) == 0:
        return Zv, Fraction(1)
    return Zv, 1 - Fraction(min(cnt), Zv)


def exact(rev: np.ndarray, number: np.ndarray, M: int, prob: np.ndarray, K: int, margin: float, masks=None):
    """The rule on one guess board: {"cand": [...], "score": [Fraction ...], "action", "changed",
    "identity": the largest |sum_v Z_v - (Z - count_c)| (0 exactly)}."""
    if masks is None:
        masks = consistent_masks(rev, number, M)
    Z, counts = posterior(masks, rev)
    assert is_guess(rev, Z, counts)
    cand = candidates(prob, rev, K, margin)
    scores, worst = [], 0
    for c in cand:
        zs = [outcome(masks, rev, M, c, v) for v in range(9)]
        worst = max(worst, abs(sum(z for z, _ in zs) - (Z - counts[c])))
        scores.append(sum(z * t for z, t in zs) / Fraction(Z))
    best = 0
    for k in range(1, len(cand)):
        if scores[k] > scores[best]:
            best = k
    return {"cand": cand, "score": scores, "action": cand[best], "changed": int(best != 0), "identity": worst,
            "Z": Z, "counts": counts}


def all_states(H: int, W: int, M: int):
    """Every (rev, number) of a tiny board: each mine layout with each non-empty set of safe cells
    revealed."""
    A = H * W
    for mines in itertools.combinations(range(A), M):
        mine = np.zeros(A, dtype=np.uint8)
        mine[list(mines)] = 1
        count = np.array([sum(mine[j] for j in P.neighbours(H, W, i)) for i in range(A)], dtype=np.uint8)
        safe = [i for i in range(A) if not mine[i]]
        for bits in range(1, 1 << len(safe)):
            rev = np.zeros(A, dtype=np.uint8)
            rev[[s for k, s in enumerate(safe) if bits >> k & 1]] = 1
            number = np.where(rev == 1, count, 200 + (np.arange(A) % 50)).astype(np.uint8)
            yield rev.reshape(H, W), number.reshape(H, W)


def _random_state(H: int, W: int, M: int, rng: np.random.Generator):
    A = H * W
    if rng.integers(2):
        _, rev, number = P.play(H, W, M, seed=int(rng.integers(1 << 31)), clicks=int(rng.integers(1, 6)))
        return rev, number
    mine = np.zeros(A, dtype=np.uint8)
    mine[rng.choice(A, size=M, replace=False)] = 1
    count = np.array([sum(mine[j] for j in P.neighbours(H, W, i)) for i in range(A)], dtype=np.uint8)
    safe = np.flatnonzero(mine == 0)
    lo = max(1, safe.size - 14)
    rev = np.zeros(A, dtype=np.uint8)
    rev[rng.choice(safe, size=int(rng.integers(lo, safe.size + 1)), replace=False)] = 1
    number = np.where(rev == 1, count, 200 + (np.arange(A) % 50)).astype(np.uint8)
    return rev.reshape(H, W), number.reshape(H, W)


@functools.lru_cache(maxsize=None)
def guess_states():
    """{(H, W, M): tuple of guess boards}, GUESS_PER_SHAPE distinct ones per shape of
    posterior_ref.SHAPES that has any (seeded; thin boards are listed exhaustively). Each entry:
    rev, number (read-only u8 [H, W]), masks (the consistent layouts), Z, counts."""
    out = {}
    for H, W, M in P.SHAPES:
        found, seen = [], set()
        if H * W <= 7:
            source = all_states(H, W, M)
        else:
            rng = np.random.default_rng(77_000 + 100 * H * W + M)
            source = (_random_state(H, W, M, rng) for _ in range(4000))
        for rev, number in source:
            if len(found) >= GUESS_PER_SHAPE:
                break
            key = (rev.tobytes(), np.where(rev == 1, number, 0).tobytes())
            if key in seen or math.comb(int((rev == 0).sum()), M) > MAX_LAYOUTS:
                continue
            seen.add(key)
            masks = consistent_masks(rev, number, M)
            Z, counts = posterior(masks, rev)
            if not is_guess(rev, Z, counts):
                continue
            rev, number = rev.copy(), number.copy()
            for a in (rev, number, masks):
                a.setflags(write=False)
            found.append({"H": H, "W": W, "M": M, "rev": rev, "number": number, "masks": masks, "Z": Z,
                          "counts": tuple(counts)})
        out[(H, W, M)] = tuple(found)
    return out
