"""numpy restatement of the action mix of include/msdagger.h (csrc/msdagger.hip k_dagger): the two
coins, the greedy arg-max, the choice rule and the agreement flag. The two Gumbel-max actions (the
uniform one and the sampled learner) hold the only floating-point arithmetic that numpy does not
reproduce bit for bit (logf), so the tests take them from ms_sample_masked on the device and pass
them in. Built on tests/sampler_ref.py's splitmix64 / uniform01."""
from __future__ import annotations

import numpy as np

from sampler_ref import splitmix64, uniform01

C_LEARNER = 0xA0761D6478BD642F
C_BETA = 0xE7037ED1A0B428DB
C_EXPLORE = 0x8EBC6AF09C88C6E3
GREEDY, SAMPLE = 0, 1
SRC_UNIFORM, SRC_EXPERT, SRC_LEARNER = 0, 1, 2
SENTINEL = 0x7FFFFFFF  # what k_sample leaves when every legal key is NaN


def stream_seed(seed: int, const: int) -> int:
    """splitmix64(seed ^ const): the seed of one of the three domain-separated streams."""
    return int(splitmix64(np.uint64(seed & (2**64 - 1)) ^ np.uint64(const)))


def coin(seed: int, const: int, counter: int, rows) -> np.ndarray:
    """The f32 coin of every global row in ``rows``: the device computes ((float)k + 0.5f) * 2^-24
    for the 24 hash bits k, which is (k + 0.5) / 2^24 rounded once to f32 (the scaling is exact), so
    rounding sampler_ref's f64 value gives the same bits."""
    return uniform01(stream_seed(seed, const), counter, rows, [0])[:, 0].astype(np.float32)


def legal(mask) -> np.ndarray:
    """bool [n, A]; a row with no legal cell counts as all legal."""
    m = np.asarray(mask).astype(bool).copy()
    m[~m.any(1)] = True
    return m


def lowest_legal(mask) -> np.ndarray:
    return legal(mask).argmax(1).astype(np.int64)


def greedy(logits, mask) -> np.ndarray:
    """The lowest-index legal cell whose logit is maximal; NaN compares below everything; when no
    legal logit is above -inf, the lowest-index legal cell."""
    m = legal(mask)
    lg = np.asarray(logits, dtype=np.float32)
    v = np.where(m & ~np.isnan(lg), lg, -np.inf)
    mx = v.max(1)
    first_max = (v == mx[:, None]).argmax(1)
    return np.where(mx > -np.inf, first_max, m.argmax(1)).astype(np.int64)


def sampled(device_actions, mask) -> np.ndarray:
    """Mode 1's learner action from ms_sample_masked's output on the learner's stream: the same
    cell, or the lowest-index legal cell where k_sample left its sentinel."""
    a = np.asarray(device_actions, dtype=np.int64)
    return np.where(a == SENTINEL, lowest_legal(mask), a)


def act(u, learner, expert_action, kind, best, *, seed, counter, beta, explore, row_begin=0):
    """-> dict(action, source, learner_action, agree). ``u``: the uniform action per row;
    ``learner``: the learner's action per row (greedy() or sampled()), or None for NULL logits."""
    kind = np.asarray(kind, dtype=np.uint8)
    n = kind.shape[0]
    rows = np.arange(row_begin, row_begin + n)
    cb = coin(seed, C_BETA, counter, rows)
    ce = coin(seed, C_EXPLORE, counter, rows)
    has = kind != 0
    source = np.full(n, SRC_UNIFORM, dtype=np.uint8)
    teacher_turn = ~(ce < np.float32(explore)) & ~(cb >= np.float32(beta))
    source[~(ce < np.float32(explore)) & (cb >= np.float32(beta))] = SRC_LEARNER
    source[teacher_turn & has] = SRC_EXPERT
    if learner is None:
        assert not (source == SRC_LEARNER).any(), "NULL logits need beta >= 1"
        l = np.full(n, -1, dtype=np.int64)
        agree = np.zeros(n, dtype=np.uint8)
    else:
        l = np.asarray(learner, dtype=np.int64)
        agree = (has & (np.asarray(best)[np.arange(n), l] != 0)).astype(np.uint8)
    action = np.where(source == SRC_LEARNER, l, np.where(source == SRC_EXPERT, np.asarray(expert_action), u))
    return {"action": action.astype(np.int64), "source": source, "learner_action": l, "agree": agree}
