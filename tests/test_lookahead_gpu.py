"""The two-guess lookahead on the device (csrc/mslookahead.hip through ms_amd/lookahead.py)
against the host twin (ms_lookahead_host), bitwise, and through its users: the expert targets,
the collectors and PosteriorModel under evaluate_vec.

Boards: the guess boards of tests/lookahead_ref.py for the small shapes, mixed with boards that
are no guess (tests/posterior_ref.py states and blank boards); for 9x9x10, 16x16x40 and 30x16x99 a
pool of live boards of the env after some moves of the greedy posterior player (a lost game
restarts blank, so the pool holds blank, safe and guess boards). Both sides get the device's base
posterior and the same node budget, so they run the same searches: every output must be equal,
``score`` bit for bit (NaN against NaN)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import lookahead_ref as R
import posterior_ref as P

pytestmark = pytest.mark.gpu

BUDGET = 1 << 12
KEYS = ("slot", "count", "cand", "action", "n_scored", "changed")


@functools.lru_cache(maxsize=None)
def _small_pool(shape):
    """(rev, num, guess) numpy: the shape's guess boards interleaved with boards that are none."""
    H, W, M = shape
    guess = R.guess_states()[shape]
    other = [s for s in P.oracle_states() if (s["H"], s["W"], s["M"]) == shape]
    hidden = [np.flatnonzero(o["rev"].reshape(-1) == 0) for o in other]
    other_guess = [h.size > 0 and min(o["counts"][c] for c in h) > 0 for o, h in zip(other, hidden)]
    rows, flags = [], []
    for i, g in enumerate(guess):
        rows.append((g["rev"], g["number"]))
        flags.append(True)
        j = i % len(other)
        blank = i % 3 == 2
        rows.append((np.zeros_like(other[j]["rev"]) if blank else other[j]["rev"], other[j]["number"]))
        flags.append(not blank and other_guess[j])
    return np.stack([r for r, _ in rows]), np.stack([n for _, n in rows]), np.array(flags)


@functools.lru_cache(maxsize=None)
def _env_pool(shape, n=128, steps=40, seed=11, keep=64):
    """(rev, num, guess) numpy: n envs play ``steps`` moves of the greedy posterior player; the pool
    is every third board of the last step (blank, safe or guess) with, in between, the forced-guess
    boards met on the way (at most ``keep``)."""
    from ms_amd import EnvConfig, VecMinesweeper
    H, W, M = shape
    dev = torch.device("cuda", torch.cuda.current_device())
    vec = VecMinesweeper(n, EnvConfig(H=H, W=W, mine_count=M), seed=seed, device=dev)
    mask = vec.reset()["action_mask"]
    met_rev, met_num = [], []
    for t in range(steps + 1):
        tg = vec.expert_targets(budget=BUDGET, method="grouped", hidden=mask)
        snap = vec.snapshot_tensors()
        g = tg["kind"] == 2
        if t == steps:
            break
        met_rev.append(snap["revealed"][g].cpu().numpy().astype(np.uint8))
        met_num.append(snap["counts"][g].cpu().numpy())
        a = torch.where(tg["kind"] != 0, tg["action"], vec.tape_actions(t))
        mask = vec.step(a)[0]["action_mask"]
    met_rev, met_num = np.concatenate(met_rev)[-keep:], np.concatenate(met_num)[-keep:]
    last_rev, last_num = snap["revealed"].cpu().numpy().astype(np.uint8), snap["counts"].cpu().numpy()
    last_g = g.cpu().numpy()
    rows, flags = [], []
    for i in range(max(len(met_rev), n)):
        if i < len(met_rev):
            rows.append((met_rev[i], met_num[i]))
            flags.append(True)
        if i < n and i % 3 == 0:
            rows.append((last_rev[i], last_num[i]))
            flags.append(bool(last_g[i]))
    return np.stack([r for r, _ in rows]), np.stack([m for _, m in rows]), np.array(flags)


def _batch(shape, n):
    """n boards of the shape's pool: guess boards and others alternate (n = 1: a guess board)."""
    rev, num, guess = _small_pool(shape) if shape[0] * shape[1] <= 64 else _env_pool(shape)
    g, o = np.flatnonzero(guess), np.flatnonzero(~guess)
    assert g.size >= 3 and o.size >= 1, (shape, g.size, o.size)
    if n >= 100:
        idx = np.arange(n) % rev.shape[0]
    else:
        idx = np.array([g[(i // 2) % g.size] if i % 2 == 0 else o[(i // 2) % o.size] for i in range(n)])
    return rev[idx], num[idx], int(guess[idx].sum())


def _both(gpu, rev, num, M, K, margin, method, cap, budget=BUDGET):
    from ms_amd.lookahead import lookahead_host, lookahead_states
    from ms_amd.posterior import posterior_states
    r, m = torch.from_numpy(rev).to(gpu), torch.from_numpy(num).to(gpu)
    base = posterior_states(r, m, M, budget=budget, method=method)
    got = lookahead_states(r, m, M, base, K=K, margin=margin, budget=budget, method=method, cap=cap)
    want = lookahead_host(rev, num, M, {k: v.cpu().numpy() for k, v in base.items()}, K=K, margin=margin,
                          budget=budget, method=method, cap=cap)
    return {k: v.cpu().numpy() for k, v in got.items()}, want, got


def _assert_equal(got, want, tag):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k)
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    gs, ws = got["score"], want["score"]
    assert gs.shape == ws.shape and np.array_equal(np.isnan(gs), np.isnan(ws)), (tag, gs, ws)
    ok = ~np.isnan(ws)
    assert np.array_equal(gs[ok].view(np.uint64), ws[ok].view(np.uint64)), (tag, gs, ws)


# (shape, n, K, margin, method, cap or None for n): every n, board, K, margin, method and cap of the
# issue's lists occurs, the large n on every path-changing size (one 64-cell slice, several, 480 cells)
CASES = [
    ((4, 4, 3), 1, 1, 0.0, "enumerate", 1),
    ((4, 4, 3), 3, 2, 0.1, "grouped", 2),
    ((4, 4, 3), 130, 16, 1.0, "enumerate", None),
    ((5, 5, 5), 5, 8, 1.0, "enumerate", None),
    ((5, 5, 5), 130, 16, 0.1, "grouped", None),
    ((5, 5, 5), 130, 8, 0.0, "grouped", 2),
    ((1, 7, 2), 5, 16, 1.0, "enumerate", 2),
    ((1, 7, 2), 130, 2, 0.1, "grouped", None),
    ((5, 1, 1), 3, 2, 0.0, "grouped", 1),
    ((5, 1, 1), 5, 8, 1.0, "enumerate", None),
    ((9, 9, 10), 130, 8, 0.1, "enumerate", None),
    ((9, 9, 10), 5, 16, 1.0, "grouped", 1),
    ((16, 16, 40), 130, 8, 0.1, "grouped", None),
    ((16, 16, 40), 5, 16, 0.0, "enumerate", 2),
    ((16, 16, 40), 3, 1, 1.0, "grouped", None),
    ((16, 30, 99), 130, 8, 0.1, "grouped", None),
    ((16, 30, 99), 3, 2, 0.0, "enumerate", 1),
    ((16, 30, 99), 1, 16, 1.0, "grouped", 1),
]


@pytest.mark.parametrize("shape,n,K,margin,method,cap", CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-n{n}-K{K}-m{m}-{me}-cap{c}" for s, n, K, m, me, c in CASES])
def test_device_equals_host_twin_bitwise(gpu, shape, n, K, margin, method, cap):
    rev, num, n_guess = _batch(shape, n)
    cap = n if cap is None else cap
    got, want, _ = _both(gpu, rev, num, shape[2], K, margin, method, cap)
    _assert_equal(got, want, (shape, n, K, margin, method, cap))
    # the slots are the first `cap` guess boards in board order, `count` has them all
    if shape[0] * shape[1] <= 64:
        assert got["count"][0] == n_guess  # the pool's flags come from the brute-force reference
    n_guess = int(got["count"][0])  # (an env pool's from the grouped counting: enumeration may decide fewer)
    assert n_guess >= 1
    used = min(cap, n_guess)
    assert np.array_equal(got["slot"][got["slot"] >= 0], np.arange(used))
    assert ((got["slot"] >= 0) == (got["action"] >= 0)).all()
    assert (got["cand"][:used, 0] >= 0).all() and (got["cand"][used:] == -1).all()
    assert np.isnan(got["score"][used:]).all()
    sl = got["slot"][got["slot"] >= 0]
    rows = np.flatnonzero(got["slot"] >= 0)
    assert all(got["action"][r] in got["cand"][s] for r, s in zip(rows, sl))
    if K == 1:
        assert not got["changed"].any()
    print(f"{shape} n {n}: {n_guess} guess boards, {used} slots, {int(got['changed'].sum())} changed, "
          f"{int((got['cand'] >= 0).sum() - got['n_scored'].sum())} unscored candidates")


def test_cap_below_the_number_of_guess_boards(gpu):
    rev, num, n_guess = _batch((5, 5, 5), 130)
    full, _, _ = _both(gpu, rev, num, 5, 8, 0.1, "grouped", 130)
    assert n_guess >= 10
    for cap in (1, 2, 7):
        got, want, _ = _both(gpu, rev, num, 5, 8, 0.1, "grouped", cap)
        _assert_equal(got, want, cap)
        first = np.flatnonzero(full["slot"] >= 0)[:cap]
        assert np.array_equal(np.flatnonzero(got["slot"] >= 0), first) and got["count"][0] == n_guess
        rest = np.setdiff1d(np.arange(130), first)
        assert (got["slot"][rest] == -1).all() and (got["action"][rest] == -1).all()
        assert not got["changed"][rest].any() and not got["n_scored"][rest].any()
        assert np.array_equal(got["action"][first], full["action"][first])
        assert np.array_equal(got["cand"], full["cand"][:cap])


def test_no_guess_board_and_determinism(gpu):
    rev, num, guess = _small_pool((4, 6, 5))
    calm = np.flatnonzero(~guess)[:7]
    got, want, _ = _both(gpu, rev[calm], num[calm], 5, 8, 0.1, "enumerate", 7)
    _assert_equal(got, want, "calm")
    assert got["count"][0] == 0 and (got["action"] == -1).all() and (got["slot"] == -1).all()
    assert (got["cand"] == -1).all() and np.isnan(got["score"]).all() and not got["changed"].any()
    rev, num, _ = _batch((16, 16, 40), 130)
    _, _, a = _both(gpu, rev, num, 40, 8, 0.1, "grouped", 130)
    _, _, b = _both(gpu, rev, num, 40, 8, 0.1, "grouped", 130)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_budget_one_on_the_device(gpu):
    """At one node per query most outcome searches stop: the candidates they leave unscored and
    the greedy fallback are the twin's."""
    rev, num, _ = _batch((5, 5, 5), 130)
    from ms_amd.lookahead import lookahead_host, lookahead_states
    from ms_amd.posterior import posterior_states
    r, m = torch.from_numpy(rev).to(gpu), torch.from_numpy(num).to(gpu)
    base = posterior_states(r, m, 5, budget=1 << 16)
    got = {k: v.cpu().numpy() for k, v in lookahead_states(r, m, 5, base, K=8, margin=0.1, budget=1).items()}
    want = lookahead_host(rev, num, 5, {k: v.cpu().numpy() for k, v in base.items()}, K=8, margin=0.1, budget=1)
    _assert_equal(got, want, "budget 1")
    assert int((got["cand"] >= 0).sum() - got["n_scored"].sum()) > 0


def _vec(gpu, n, min_guess, seed=3, steps=80):
    """9x9x10 envs played by the greedy posterior player until at least ``min_guess`` of them face a
    forced guess at the same time (forced guesses are under 1 % of this player's boards)."""
    from ms_amd import EnvConfig, VecMinesweeper
    vec = VecMinesweeper(n, EnvConfig(H=9, W=9, mine_count=10), seed=seed, device=gpu)
    mask = vec.reset()["action_mask"]
    for t in range(steps):
        tg = vec.expert_targets(budget=BUDGET, hidden=mask)
        if t >= 6 and int((tg["kind"] == 2).sum()) >= min_guess:
            return vec, mask
        mask = vec.step(torch.where(tg["kind"] != 0, tg["action"], vec.tape_actions(t)))[0]["action_mask"]
    raise AssertionError(f"no step with {min_guess} forced guesses among {n} envs")


def test_expert_targets_with_lookahead(gpu):
    vec, mask = _vec(gpu, n=1024, min_guess=3)
    plain = vec.expert_targets(budget=BUDGET, hidden=mask)
    got = vec.expert_targets(budget=BUDGET, hidden=mask, lookahead=8, margin=0.1)
    res = got["lookahead"]
    rows = (plain["kind"] == 2) & (res["slot"] >= 0)
    assert torch.equal(rows, plain["kind"] == 2) and int(rows.sum()) >= 3  # cap = n: every guess row has a slot
    for k in plain:
        assert torch.equal(got[k][~rows], plain[k][~rows]), k
    for k in ("kind", "labels", "status", "prob"):
        assert torch.equal(got[k], plain[k]), k
    act = got["action"][rows]
    assert torch.equal(act, res["action"][rows])
    assert (got["best"][rows].sum(dim=1) == 1).all() and (got["n_best"][rows] == 1).all()
    assert (got["best"][rows].gather(1, act[:, None]) == 1).all()
    assert (res["cand"][res["slot"][rows].long()] == act[:, None].int()).any(dim=1).all()
    assert mask[rows].gather(1, act[:, None]).all()  # a hidden cell
    # the twin on the same boards
    from ms_amd.lookahead import lookahead_host
    snap = vec.snapshot_tensors()
    vec.set_posterior_budget(BUDGET)
    post = {k: v.cpu().numpy() for k, v in vec.mine_posterior(resolve=False, method="grouped").items()}
    assert np.array_equal(post["prob"], plain["prob"].cpu().numpy())
    want = lookahead_host(snap["revealed"].cpu().numpy(), snap["counts"].cpu().numpy(), 10, post, K=8, margin=0.1,
                          budget=BUDGET, method="grouped")
    for k in KEYS:
        assert np.array_equal(want[k], res[k].cpu().numpy()), k


def _fields(buf):
    return {k: getattr(buf, k).clone() for k in buf.FIELDS}


def test_collect_expert_default_is_unchanged_and_lookahead_plays_the_twins_choice(gpu):
    """64 envs x 16 steps of 9x9x10, continued twice. lookahead=0 is bitwise the call without the
    argument. With lookahead=8 (explore 0, so every move with a target is the teacher's) the buffer's
    ``best`` on a guess row is one-hot at the cell the host twin chooses on that row's board, and the
    next row of that env shows the cell revealed unless the click lost the game."""
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.imitate import collect_expert
    from ms_amd.lookahead import lookahead_host
    from ms_amd.posterior import posterior_host
    cfg = EnvConfig(H=9, W=9, mine_count=10)
    N, T = 64, 16

    def run(**kw):
        vec = VecMinesweeper(N, cfg, seed=5, device=gpu)
        out, buf = [], None
        for it in range(3):
            buf = collect_expert(vec, T, budget=BUDGET, method="grouped", explore=0.0, seed=40 + it, buffer=buf,
                                 reset=it == 0, **kw)
            out.append(_fields(buf))
        return out
    base, zero, look = run(), run(lookahead=0), run(lookahead=8, margin=0.1)
    for a, b in zip(base, zero):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    guess_rows = changed = 0
    for f in look:
        codes = f["codes"].cpu().numpy()
        rev, num = (codes > 0).astype(np.uint8), np.where(codes > 0, codes - 1, 0).astype(np.uint8)
        kind, best = f["kind"].cpu().numpy(), f["best"].cpu().numpy()
        rows = np.flatnonzero(kind == 2)
        post = posterior_host(rev[rows], num[rows], 10, host_budget=BUDGET, method="grouped")
        assert (post["status"] == 1).all()
        want = lookahead_host(rev[rows], num[rows], 10, post, K=8, margin=0.1, budget=BUDGET, method="grouped")
        assert (want["slot"] >= 0).all()
        assert (best[rows].sum(axis=1) == 1).all()
        assert np.array_equal(best[rows].argmax(axis=1), want["action"])
        guess_rows += rows.size
        changed += int(want["changed"].sum())
        nxt = rows[rows + N < N * T]
        cell = best[nxt].argmax(axis=1)
        after = codes.reshape(N * T, -1)[nxt + N]
        over = (after > 0).sum(axis=1) < (codes.reshape(N * T, -1)[nxt] > 0).sum(axis=1)  # the game ended: a fresh board
        assert ((after[np.arange(nxt.size), cell] > 0) | over).all()
    print(f"{guess_rows} guess rows, {changed} where the lookahead's choice is not the greedy cell")
    assert guess_rows >= 5  # not vacuous: forced guesses are about 0.5 % of the 3,072 rows


def test_evaluate_vec_with_the_lookahead_player(gpu):
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.posterior import PosteriorModel
    cfg = EnvConfig(H=9, W=9, mine_count=10)

    def run(**kw):
        m = PosteriorModel(10, method="grouped", **kw).to(gpu)
        return evaluate_vec(m, cfg, episodes=64, seed=0, num_envs=64), m
    (a, ma), (b, mb) = run(lookahead=8), run(lookahead=8)
    ca, cb = ma.lookahead_counters(), mb.lookahead_counters()
    assert ca == cb and ca["guess_boards"] > 0 and ca["overflow"] == 0 and 0 <= ca["changed"] <= ca["guess_boards"]
    assert a["invalid_rate"] == 0 and a["episodes"] == 64
    same = lambda x, y: x == y or (x != x and y != y)  # noqa: E731
    assert a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    (g0, m0), (g1, _) = run(lookahead=0), run()
    assert g0.keys() == g1.keys() and all(same(g0[k], g1[k]) for k in g0)
    assert m0.lookahead_counters() == dict.fromkeys(PosteriorModel.COUNTERS, 0)
    print(f"9x9x10, 64 episodes: greedy {g0['win_rate']:.3f}, lookahead {a['win_rate']:.3f}, counters {ca}")
    capped, mc = run(lookahead=8, lookahead_cap=1)
    cc = mc.lookahead_counters()
    assert capped["invalid_rate"] == 0 and cc["overflow"] > 0
