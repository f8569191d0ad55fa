"""The exact posterior with grouped counting on device (k_posterior<*, true> of
csrc/msposterior.hip through the entry points of include/msposterior_grouped.h) against its host
twin (every output, prob and configs bitwise), against the enumerating kernel (bitwise wherever
both decide), and through VecMinesweeper, collect_rollout, PosteriorModel and evaluate_vec."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import posterior_ref as R
from test_posterior_grouped_host import BOARDS, BUDGET, bits, fixture_host, stripe

pytestmark = pytest.mark.gpu


def _cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _states(rev, number, M, gpu, **kw):
    from ms_amd.posterior import posterior_states
    return _cpu(posterior_states(torch.from_numpy(np.ascontiguousarray(rev)).to(gpu),
                                 torch.from_numpy(np.ascontiguousarray(number)).to(gpu), M, **kw))


def _assert_same(got, want, where, rows=slice(None)):
    for k in ("status", "max_nodes"):
        assert np.array_equal(got[k][rows], want[k][rows]), (where, k)
    for k in ("prob", "configs"):
        assert np.array_equal(bits(got[k][rows]), bits(want[k][rows])), (where, k)


def _assert_equals_host(got, host, where):
    """Device against host where the combine is not exact arithmetic (C(U, r) past 2^53): status
    and node counts exactly, prob and configs within the bound of tests/test_posterior_gpu.py,
    1e-12 (absolute on p <= 1, relative on configs). The counts are the same integers on both
    sides; the device contracts each multiply-add of the f64 combine into an FMA, the host rounds
    twice, so a sum of at most 513 non-negative terms per fold, over at most 256 folds, differs by
    a few hundred units of 2^-53 = 1.1e-16 relative at the very most."""
    for k in ("status", "max_nodes"):
        assert np.array_equal(got[k], host[k]), (where, k)
    dp = float(np.abs(got["prob"] - host["prob"]).max())
    dz = float((np.abs(got["configs"] - host["configs"]) / host["configs"]).max())
    print(f"{where}: worst |p - host| {dp:.3g}, worst relative configs difference {dz:.3g}")
    assert dp <= 1e-12 and dz <= 1e-12, where


@pytest.mark.parametrize("n", [1, 3, 67])
def test_device_equals_host_on_the_oracle_set(gpu, n):
    from ms_amd.posterior import posterior_host
    for (H, W, M), (rev, number, p, configs) in R.by_shape(R.oracle_states()).items():
        idx = (np.arange(n) * 5 + n) % len(rev)
        got = _states(rev[idx], number[idx], M, gpu, method="grouped")
        assert (got["status"] == 1).all(), (H, W, M, got["status"])
        _assert_same(got, posterior_host(rev[idx], number[idx], M, method="grouped"), (H, W, M))
        assert np.abs(got["prob"] - p[idx]).max() <= 1e-12, (H, W, M)


@pytest.mark.parametrize("W,n", [(30, 67), (36, 1), (60, 2)])
def test_device_equals_host_on_the_stripes(gpu, W, n):
    """One component of 2 W free cells in W groups (W = 60: 120 cells, near MS_AVOID_MAX_VARS, so 16
    queries at a time; W = 30 in a batch of 67 boards: 31 queries on 32 lanes, idle lanes beside
    them). Enumeration cannot finish any of them."""
    from ms_amd.posterior import posterior_host
    rev, num = stripe(W)
    rev, num = np.repeat(rev, n, axis=0), np.repeat(num, n, axis=0)
    got = _states(rev, num, W, gpu, budget=BUDGET, method="grouped")
    host = posterior_host(rev, num, W, host_budget=BUDGET, method="grouped")
    print(f"W = {W}: status {got['status'][0]}, configs {got['configs'][0]!r}, largest query {got['max_nodes'][0]}")
    _assert_same(got, host, W)
    assert (got["status"] == 1).all() and (got["configs"] == 2.0 ** W).all() and (got["max_nodes"] < 1000).all()
    assert np.array_equal(bits(got["prob"]), bits(np.where(rev.reshape(n, -1) != 0, 0.0, 0.5)))
    plain = _states(rev[:1], num[:1], W, gpu, budget=1 << 10)
    assert plain["status"].tolist() == [2] and not plain["prob"].any()


@pytest.mark.parametrize("board", BOARDS)
def test_fixture_states_on_device(gpu, board):
    """Budget 2^16: the device decides all states with grouping, equals the host twin in every
    output (status and node counts exactly, the f64 outputs as _assert_equals_host says), and is
    bitwise the enumerating kernel wherever that decides."""
    z, num, host = fixture_host(board, "grouped")
    got = _states(z["rev"], num, z["K"], gpu, budget=BUDGET, method="grouped")
    plain = _states(z["rev"], num, z["K"], gpu, budget=BUDGET)
    both = plain["status"] == 1
    print(f"{board}: grouped leaves {int((got['status'] != 1).sum())} of {z['S']} undecided (largest query "
          f"{int(got['max_nodes'].max())}), enumerate {int((~both).sum())}")
    assert (got["status"] == 1).all()
    _assert_equals_host(got, host, board)
    assert both.any()
    for k in ("prob", "configs"):
        assert np.array_equal(bits(got[k][both]), bits(plain[k][both])), k


def test_budget_live_and_blank_boards(gpu):
    """Budget 1: the stripe is undecided with zero outputs and at most one node, never a guess.
    Rows that are not live or have nothing revealed are skipped as by the enumerating kernel; an
    inconsistent board is undecided with zeros."""
    rev, num = stripe(30)
    got = _states(rev, num, 30, gpu, budget=1, method="grouped")
    assert got["status"].tolist() == [2] and not got["prob"].any() and not got["configs"].any()
    assert 0 <= got["max_nodes"][0] <= 1
    rev = np.zeros((4, 2, 2), dtype=np.uint8)
    rev[:3, 1] = 1
    num = np.ones((4, 2, 2), dtype=np.uint8)
    num[1] = 3  # no layout gives a 3 with two hidden neighbours
    live = torch.tensor([1, 1, 0, 1], device=gpu)
    got = _states(rev, num, 1, gpu, live=live, method="grouped")
    assert got["status"].tolist() == [1, 2, 0, 0]
    assert got["prob"][0].tolist() == [0.5, 0.5, 0, 0] and got["configs"][0] == 2
    assert not got["prob"][1:].any() and not got["configs"][1:].any() and not got["max_nodes"][1:].any()
    assert np.isfinite(got["prob"]).all()
    plain = _states(rev, num, 1, gpu, live=live)
    for k in ("status", "prob", "configs"):
        assert np.array_equal(got[k], plain[k]), k


def _vec(gpu, board, n=256, seed=3):
    from ms_amd import EnvConfig, VecMinesweeper
    H, W, K = (int(v) for v in board.split("x"))
    vec = VecMinesweeper(n, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)
    vec.reset()
    return vec, K


def _tbits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    """Equal, floating-point tensors bit for bit."""
    return torch.equal(_tbits(a), _tbits(b)) if a.is_floating_point() else torch.equal(a, b)


@pytest.mark.parametrize("board", ["16x16x40", "9x9x10"])
def test_handle_path(gpu, board):
    """256 envs after 15 uniform tape steps, budget 2^12: the handle call is the states call on a
    snapshot, equals the enumerating handle call bitwise wherever both decide, gives identical
    bits twice, and leaves env state and RNG streams alone."""
    from ms_amd import _lib as L
    from ms_amd.posterior import posterior_states
    vec, K = _vec(gpu, board)
    for t in range(15):
        vec.step(vec.tape_actions(t, L.MS_TAPE_UNIFORM))
    vec.set_posterior_budget(1 << 12)
    rng0 = vec.rng_state().copy()
    snap0 = {k: v.clone() for k, v in vec.snapshot_tensors().items() if torch.is_tensor(v)}
    got = vec.mine_posterior(method="grouped", resolve=False)
    again = vec.mine_posterior(method="grouped", resolve=False)
    plain = vec.mine_posterior(resolve=False)
    snap = vec.snapshot_tensors()
    want = posterior_states(snap["revealed"], snap["counts"], K, live=snap["first_click"], budget=1 << 12,
                            method="grouped")
    for k in want:
        assert _same(got[k], want[k]) and _same(got[k], again[k]), k
    both = (got["status"] == 1) & (plain["status"] == 1)
    print(f"{board}: decided grouped {int((got['status'] == 1).sum())}, enumerate {int((plain['status'] == 1).sum())}, "
          f"largest query {int(got['max_nodes'].max())} / {int(plain['max_nodes'].max())}")
    assert int(both.sum()) > 0
    for k in ("prob", "configs"):
        assert torch.equal(_tbits(got[k][both]), _tbits(plain[k][both])), k
    assert np.array_equal(vec.rng_state(), rng0)
    for k, v in snap0.items():
        assert torch.equal(vec.snapshot_tensors()[k], v), k


def test_posterior_labels_grouped(gpu):
    """ms_posterior_labels_grouped against its parts at budgets 2^12 and 8: valid is mine_labels',
    source 0 rows are zero, source 2 rows the mine mask bit for bit, source 1 rows (float) of the
    f64 grouped posterior; rows both methods decide are bitwise equal."""
    from ms_amd import _lib as L
    seen = {s: 0 for s in (0, 1, 2)}
    for board, budget in (("9x9x10", 1 << 12), ("16x16x40", 8)):
        vec, K = _vec(gpu, board, n=67)
        vec.set_posterior_budget(budget)
        n, A = vec.num_envs, vec.H * vec.W
        for t in range(8):
            a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
            if t in (0, 3, 7):
                post = vec.mine_posterior(method="grouped", resolve=False)
                hard, hvalid = vec.mine_labels()
                labels, valid, source = vec.posterior_labels(budget=budget, method="grouped")
                plabels, pvalid, psource = vec.posterior_labels(budget=budget)
                assert torch.equal(valid, hvalid) and torch.equal(valid, pvalid), (board, t)
                assert torch.equal(source, post["status"]), (board, t)
                lab, hd = labels.reshape(n, A), hard.reshape(n, A)
                assert not lab[source == 0].any()
                assert torch.equal(_tbits(lab[source == 2]), _tbits(hd[source == 2])), (board, t)
                assert torch.equal(_tbits(lab[source == 1]), _tbits(post["prob"][source == 1].to(torch.float32)))
                both = (source == 1) & (psource == 1)
                assert torch.equal(_tbits(lab[both]), _tbits(plabels.reshape(n, A)[both])), (board, t)
                for s in seen:
                    seen[s] += int((source == s).sum())
            vec.step(a)
    print("boards by source:", seen)
    assert all(v > 0 for v in seen.values())


def test_rollout_grouped_targets(gpu):
    """collect_rollout(posterior_method="grouped") fills the slots the enumerating rollout fills,
    from a twin env's posterior_labels(method="grouped"); the default call's buffer is bitwise
    the one of posterior_method="enumerate" passed explicitly."""
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.posterior import TRAIN_BUDGET
    from test_posterior_labels_gpu import _BUFFER_TENSORS, _rollout
    buf, _, (H, W, K, N, T) = _rollout(gpu, belief_targets="posterior", posterior_method="grouped")
    default, _, _ = _rollout(gpu, belief_targets="posterior")
    explicit, _, _ = _rollout(gpu, belief_targets="posterior", posterior_method="enumerate")
    for k in _BUFFER_TENSORS + ("mine_source",):
        assert _same(getattr(default, k), getattr(explicit, k)), k
    twin = VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=5, device=gpu)
    twin.reset()
    acts = buf.actions.view(T, N)
    for t in range(T):
        rows = slice(t * N, (t + 1) * N)
        labels, valid, source = twin.posterior_labels(budget=TRAIN_BUDGET, method="grouped")
        assert torch.equal(_tbits(buf.mine_labels[rows]), _tbits(labels)), t
        assert torch.equal(buf.mine_valid[rows], valid) and torch.equal(buf.mine_source[rows], source), t
        twin.step(acts[t])
    assert bool((buf.mine_source[N:] == 1).any())
    for k in _BUFFER_TENSORS:  # everything but the targets is the enumerating rollout's
        if k != "mine_labels":
            assert torch.equal(getattr(buf, k), getattr(default, k)), k
    both = (buf.mine_source == 1) & (default.mine_source == 1)
    assert torch.equal(_tbits(buf.mine_labels[both]), _tbits(default.mine_labels[both]))


@functools.lru_cache(maxsize=None)
def _model_run(method):
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.posterior import PosteriorModel
    gpu = torch.device("cuda:0")
    return evaluate_vec(PosteriorModel(10, method=method).to(gpu), EnvConfig(H=9, W=9, mine_count=10), episodes=64,
                        seed=0, num_envs=64)


def test_posterior_model_plays_the_same_games(gpu):
    """At 9x9 both methods decide every board with bitwise equal probabilities, so the greedy
    player's games, and with them every metric, are the same to the last bit."""
    got, want = _model_run("grouped"), _model_run("enumerate")
    assert set(got) == set(want)
    differ = {k: (got[k], want[k]) for k in got if got[k] != want[k] and not (math.isnan(got[k]) and math.isnan(want[k]))}
    assert not differ, differ
    assert got["episodes"] == 64
