"""The exact posterior on device (csrc/msposterior.hip through ms_posterior / ms_posterior_states,
VecMinesweeper.mine_posterior, PosteriorModel and evaluate_vec(posterior=True)) against
brute-force enumeration (posterior_ref.py), the host twin, and the fixture states of
tests/golden/avoid_states.npz."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import avoid_fixture as F
import posterior_ref as R
from test_posterior_host import _numbers

BOARDS = ["9x9x10", "16x16x40", "30x16x99", "16x30x99"]


def _cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _states(rev, number, M, gpu, **kw):
    from ms_amd.posterior import posterior_states
    return _cpu(posterior_states(torch.from_numpy(np.ascontiguousarray(rev)).to(gpu),
                                 torch.from_numpy(np.ascontiguousarray(number)).to(gpu), M, **kw))


@functools.lru_cache(maxsize=None)
def _fixture_host(board):
    """The host twin on the fixture states, once per session: the device's reference."""
    from ms_amd.posterior import posterior_host
    z = F.load(board)
    num = _numbers(z["mine"])
    host = posterior_host(z["rev"], num, z["K"], host_budget=1 << 26)
    for v in host.values():
        v.setflags(write=False)
    return z, num, host


def _assert_equals_host(got, host, rows, where):
    assert (host["status"][rows] == 1).all(), where
    assert np.array_equal(got["max_nodes"][rows], host["max_nodes"][rows]), where
    assert np.abs(got["prob"][rows] - host["prob"][rows]).max(initial=0.0) <= 1e-12, where
    rel = np.abs(got["configs"][rows] - host["configs"][rows]) / host["configs"][rows]
    assert rel.max(initial=0.0) <= 1e-12, where


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 67])
def test_oracle_on_device(gpu, n):
    """The brute-force states at the default budget, n different boards of one shape per launch
    (the shape's states repeated in order until there are n)."""
    from ms_amd.posterior import posterior_host
    worst = 0.0
    for (H, W, M), (rev, number, p, configs) in R.by_shape(R.oracle_states()).items():
        idx = (np.arange(n) * 5 + n) % len(rev)
        got = _states(rev[idx], number[idx], M, gpu)
        assert (got["status"] == 1).all(), (H, W, M, got["status"])
        worst = max(worst, float(np.abs(got["prob"] - p[idx]).max()))
        assert np.abs(got["prob"] - p[idx]).max() <= 1e-12, (H, W, M)
        assert (np.abs(got["configs"] - configs[idx]) <= 1e-12 * configs[idx]).all(), (H, W, M)
        host = posterior_host(rev[idx], number[idx], M)
        assert np.array_equal(got["max_nodes"], host["max_nodes"]), (H, W, M)
    print(f"n = {n}: worst |p - oracle| on device {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("board", BOARDS)
def test_fixture_on_device(gpu, board):
    """Default budget: wherever the device decides, p and max_nodes are the host's. The small
    boards are all decided; at expert density at most a quarter of the states may run out."""
    z, num, host = _fixture_host(board)
    got = _states(z["rev"], num, z["K"], gpu)
    dec = got["status"] == 1
    share = float((~dec).mean())
    print(f"{board}: {int((~dec).sum())} of {z['S']} states undecided on device ({share:.1%}), "
          f"largest decided query {int(got['max_nodes'][dec].max())} nodes")
    assert (dec | (got["status"] == 2)).all()
    _assert_equals_host(got, host, np.flatnonzero(dec), board)
    assert not got["prob"][~dec].any() and not got["configs"][~dec].any()
    if board in ("9x9x10", "16x16x40"):
        assert dec.all()
    else:
        assert share <= 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("board", BOARDS)
def test_tight_budget_is_undecided_never_wrong(gpu, board):
    z, num, host = _fixture_host(board)
    got = _states(z["rev"], num, z["K"], gpu, budget=8)
    und = got["status"] == 2
    assert und.any() and ((got["status"] == 1) | und).all()
    assert not got["prob"][und].any() and not got["configs"][und].any()
    assert (got["max_nodes"][und] == 8).all()
    assert (host["max_nodes"][~und] <= 8).all()
    _assert_equals_host(got, host, np.flatnonzero(~und), f"{board} budget 8")


@pytest.mark.gpu
def test_device_edge_cases(gpu):
    """Skipped rows, an inconsistent board (undecided, zeros, never a NaN), a board of more than
    512 cells (undecided), live masks, wrong shapes."""
    from ms_amd.posterior import posterior_states
    rev = np.zeros((4, 2, 2), dtype=np.uint8)
    rev[:3, 1] = 1
    num = np.ones((4, 2, 2), dtype=np.uint8)
    num[1] = 3  # no layout gives a 3 with two hidden neighbours
    got = _states(rev, num, 1, gpu, live=torch.tensor([1, 1, 0, 1], device=gpu))
    assert got["status"].tolist() == [1, 2, 0, 0]
    assert got["prob"][0].tolist() == [0.5, 0.5, 0, 0] and got["configs"][0] == 2
    assert not got["prob"][1:].any() and not got["configs"][1:].any() and not got["max_nodes"][1:].any()
    assert np.isfinite(got["prob"]).all()
    wide = np.zeros((1, 20, 30), dtype=np.uint8)  # 600 cells: more than the device analyses
    wide[0, :, :3] = 1
    big = _states(wide, np.zeros_like(wide), 50, gpu)
    assert big["status"].tolist() == [2] and not big["prob"].any() and not big["configs"].any()
    t = torch.zeros((2, 3, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        posterior_states(t, t[:, :2], 1)
    with pytest.raises(ValueError):
        posterior_states(t, t, 1, live=torch.ones(3, device=gpu))
    with pytest.raises(ValueError):
        posterior_states(t.cpu(), t.cpu(), 1)


def _vec(gpu, board, n=256, seed=3):
    from ms_amd import EnvConfig, VecMinesweeper
    H, W, K = (int(v) for v in board.split("x"))
    vec = VecMinesweeper(n, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)
    vec.reset()
    return vec, K


@pytest.mark.gpu
@pytest.mark.parametrize("board", ["9x9x10", "8x8x4", "16x16x40"])
def test_handle_path_matches_states_and_disturbs_nothing(gpu, board):
    """256 envs, 24 safe-biased tape steps: at each step ms_posterior on the handle equals
    ms_posterior_states on a snapshot bit for bit (the same kernel on the same data), and the
    step after it equals that of a twin env that was never analysed (outputs and RNG streams).
    Budget 2^12: random tape clicks leave components with too many solutions to enumerate, and
    such a board costs its whole budget."""
    from ms_amd import _lib as L
    from ms_amd.posterior import posterior_states
    (vec, K), (twin, _) = _vec(gpu, board), _vec(gpu, board)
    vec.set_posterior_budget(1 << 12)
    gen = torch.Generator().manual_seed(1)
    analysed = searched = 0
    for t in range(24):
        a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
        live = None if t % 3 else (torch.rand(vec.num_envs, generator=gen) < 0.7).to(gpu)
        got = _cpu(vec.mine_posterior(live=live, resolve=False))
        snap = vec.snapshot_tensors()
        lv = snap["first_click"] if live is None else snap["first_click"] & live
        want = _cpu(posterior_states(snap["revealed"], snap["counts"], K, live=lv, budget=1 << 12))
        for k in want:
            assert np.array_equal(got[k], want[k]), (t, k)
        assert np.array_equal(got["status"] == 0, ~lv.cpu().numpy()), t
        dec = got["status"] == 1
        assert np.abs(got["prob"][dec].sum(1) - K).max(initial=0.0) <= 1e-9, t
        mine = snap["mine"].reshape(vec.num_envs, -1).cpu().numpy() & ~snap["revealed"].reshape(vec.num_envs, -1).cpu().numpy()
        assert (got["prob"][dec][mine[dec]] > 0).all(), t
        analysed += int(dec.sum())
        searched += int((got["max_nodes"] > 0).sum())
        b1, r1, d1, i1 = vec.step(a)
        b2, r2, d2, i2 = twin.step(a)
        assert torch.equal(b1["obs"], b2["obs"]) and torch.equal(b1["action_mask"], b2["action_mask"]), t
        assert torch.equal(r1, r2) and torch.equal(d1, d2), t
        assert all(torch.equal(i1.tensors[k], i2.tensors[k]) for k in i1.tensors), t
    assert np.array_equal(vec.rng_state(), twin.rng_state())
    assert analysed > 1000 and searched > 0


@pytest.mark.gpu
@pytest.mark.parametrize("board", ["9x9x10", "16x16x40"])
def test_host_fallback_resolves_undecided(gpu, board):
    """A handle with budget 8 leaves boards undecided; mine_posterior(resolve=True) re-solves
    them on the host and equals the states path at the default budget: status and node counts
    exactly (the host runs with the device's default budget here, so a board whose component has
    too many solutions to enumerate, which random tape clicks produce, is undecided on both)."""
    from ms_amd import _lib as L
    from ms_amd.posterior import posterior_states
    vec, K = _vec(gpu, board, n=512)
    vec.set_posterior_budget(8)
    undecided = 0
    for t in range(14):
        a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
        if t >= 10:
            raw = _cpu(vec.mine_posterior(resolve=False))
            undecided += int((raw["status"] == 2).sum())
            version = vec._version
            got = _cpu(vec.mine_posterior(resolve=True, host_budget=L.MS_POSTERIOR_DEFAULT_BUDGET))
            assert vec._version == version
            snap = vec.snapshot_tensors()
            want = _cpu(posterior_states(snap["revealed"], snap["counts"], K, live=snap["first_click"]))
            dec = want["status"] == 1
            assert dec.sum() >= 256, t
            for k in ("status", "max_nodes"):
                assert np.array_equal(got[k], want[k]), (t, k)
            assert np.abs(got["prob"] - want["prob"]).max() <= 1e-12, t
            assert (np.abs(got["configs"] - want["configs"]) <= 1e-12 * want["configs"]).all(), t
            assert (got["configs"][dec] >= 1).all() and not got["configs"][~dec].any(), t
        vec.step(a)
    print(f"{board}: {undecided} boards went through the host fallback")
    assert undecided >= 1, "the fallback was not exercised"


_OLD_KEYS = ("win_rate", "win_ci_low", "win_ci_high", "avg_steps", "avg_progress", "invalid_rate", "belief_auroc",
             "belief_ece", "wins", "episodes")
_NEW_KEYS = ("belief_posterior_mae", "belief_posterior_kl", "chosen_mine_prob", "guess_regret", "optimal_pick_rate",
             "posterior_undecided", "posterior_max_nodes")
_CFG = dict(episodes=256, seed=0, num_envs=256)


@functools.lru_cache(maxsize=None)
def _rule_run(posterior):
    from eval_model import RuleModel
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    gpu = torch.device("cuda:0")
    return evaluate_vec(RuleModel().to(gpu), EnvConfig(H=9, W=9, mine_count=10), posterior=posterior, **_CFG)


@pytest.mark.gpu
def test_evaluate_vec_posterior_keys(gpu):
    """posterior=False returns the parent's dict (its keys and values are those of the reference
    fixture run); posterior=True leaves every old key as it was and adds seven finite ones."""
    import os
    from eval_model import DetModel, RuleModel
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    plain, got = _rule_run(False), _rule_run(True)
    z = np.load(os.path.join(F.GOLDEN, "eval_vec_9x9x10.npz"))
    ref = dict(zip([str(k) for k in z["keys"]], z["values"]))
    assert set(plain) == set(ref)  # the parent's key set
    det = evaluate_vec(DetModel().to(gpu), EnvConfig(H=9, W=9, mine_count=10), episodes=int(z["episodes"]), seed=0,
                       num_envs=int(z["num_envs"]))  # ... and the values the parent gave on the recorded run
    for k in _OLD_KEYS:
        tol = {"belief_ece": 1e-6, "belief_auroc": 2e-3}.get(k, 1e-12)
        assert det[k] == pytest.approx(ref[k], abs=tol), k
    assert set(got) == set(plain) | set(_NEW_KEYS)
    for k in plain:
        assert got[k] == plain[k] or (math.isnan(got[k]) and math.isnan(plain[k])), k
    print({k: got[k] for k in _NEW_KEYS})
    assert all(math.isfinite(got[k]) for k in _NEW_KEYS)
    assert 0.0 <= got["guess_regret"] <= got["chosen_mine_prob"] <= 1.0
    assert 0.0 <= got["optimal_pick_rate"] <= 1.0 and got["belief_posterior_mae"] >= 0.0
    assert got["belief_posterior_kl"] >= 0.0 and got["posterior_undecided"] == 0
    # the same env stream through the diagnostics path: the nine keys are untouched by posterior=True
    both = evaluate_vec(RuleModel().to(gpu), EnvConfig(H=9, W=9, mine_count=10), posterior=True, diagnostics=True, **_CFG)
    only = evaluate_vec(RuleModel().to(gpu), EnvConfig(H=9, W=9, mine_count=10), diagnostics=True, **_CFG)
    assert all(both[k] == only[k] or (math.isnan(both[k]) and math.isnan(only[k])) for k in only)
    assert all(both[k] == got[k] for k in _NEW_KEYS)


@pytest.mark.gpu
def test_evaluate_vec_posterior_model(gpu):
    """The exact-inference greedy player scored against its own posterior: no regret, every pick
    optimal, beliefs equal to p up to the logit clamp and float32; a second run is identical."""
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.posterior import PosteriorModel
    cfg = EnvConfig(H=9, W=9, mine_count=10)
    got = evaluate_vec(PosteriorModel(10).to(gpu), cfg, posterior=True, **_CFG)
    print({k: got[k] for k in ("win_rate", "belief_ece", "belief_auroc") + _NEW_KEYS})
    assert got["posterior_undecided"] == 0
    assert 0.0 <= got["guess_regret"] <= 1e-9
    assert got["optimal_pick_rate"] == 1.0
    assert got["belief_posterior_mae"] <= 1e-6
    assert got["invalid_rate"] == 0.0
    again = evaluate_vec(PosteriorModel(10).to(gpu), cfg, posterior=True, **_CFG)
    assert set(again) == set(got)
    differ = {k: (got[k], again[k]) for k in got if again[k] != got[k] and not (math.isnan(again[k]) and math.isnan(got[k]))}
    assert not differ, differ
    assert got["win_rate"] > _rule_run(False)["win_rate"]  # exact inference beats the single-point rules
