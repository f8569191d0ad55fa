"""The avoidability analysis on device (csrc/mssolve.hip through ms_avoid / ms_avoid_states,
VecMinesweeper.avoidability and evaluate_vec(diagnostics=True)) against the reference's
analyze_avoidability (tests/golden/avoid_states.npz) and the reference's evaluate_vec metric
dicts (tests/golden/eval_vec_*.npz, whose nine avoidability keys no other test reads)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import avoid_fixture as F

BOARDS = ["9x9x10", "16x16x40", "30x16x99", "16x30x99"]


def _cpu(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _states(z, gpu, budget=None):
    from ms_amd.avoid import avoid_states
    kw = {} if budget is None else {"budget": budget}
    return _cpu(avoid_states(torch.from_numpy(z["rev"].copy()).to(gpu), torch.from_numpy(z["mine"].copy()).to(gpu),
                             torch.from_numpy(z["chosen"].copy()).to(gpu), **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("board", BOARDS)
def test_fixture_on_device(gpu, board):
    """Default budget: every fixture state is decided and equals the reference on every output;
    the node counts are the host solver's."""
    from ms_amd.avoid import avoid_host
    z = F.load(board)
    got = _states(z, gpu)
    print(f"{board}: device max_nodes {int(got['max_nodes'].max())}, reference's {int(z['ref_nodes'].max())}")
    assert (got["status"] == 1).all(), np.flatnonzero(got["status"] != 1)
    F.assert_matches_reference(got, z, where=board)
    host = avoid_host(z["rev"], z["mine"], z["chosen"])
    assert np.array_equal(got["max_nodes"], host["max_nodes"])
    assert int(got["max_nodes"].max()) * 8 <= 1 << 18  # mssolve.h: the default budget keeps 8x headroom


@pytest.mark.gpu
@pytest.mark.parametrize("board", BOARDS)
def test_tight_budget_is_undecided_never_wrong(gpu, board):
    z = F.load(board)
    got = _states(z, gpu, budget=8)
    und = got["status"] == 2
    searched = z["cls"] != F.CLS_PROP
    assert und.any() and not und[~searched].any()  # only states that needed the search can run out
    assert ((got["status"] == 1) | und).all()
    F.assert_matches_reference(got, z, rows=np.flatnonzero(~und), where=f"{board} budget 8")
    for k in ("avoidable", "n_safe", "chosen_safe"):
        assert not got[k][und].any(), k
    assert not got["safe_mask"][und].any() and (got["max_nodes"][und] == 8).all()
    full = _states(z, gpu)
    for k in ("chosen_comp", "n_comp", "n_frontier", "comp_size"):  # still valid when undecided
        assert np.array_equal(got[k], full[k]), k


def _vec(gpu, board, n=256, seed=3):
    from ms_amd import EnvConfig, VecMinesweeper
    H, W, K = (int(v) for v in board.split("x"))
    vec = VecMinesweeper(n, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)
    vec.reset()
    return vec


@pytest.mark.gpu
@pytest.mark.parametrize("board", ["9x9x10", "16x16x40"])
def test_host_fallback_resolves_undecided(gpu, board):
    """A handle with budget 8 leaves boards undecided; avoidability(resolve=True) re-solves them
    on the host and equals the states path at the default budget, node counts included."""
    from ms_amd import _lib as L
    from ms_amd.avoid import avoid_states
    vec = _vec(gpu, board, n=1024)
    vec.set_avoid_budget(8)
    undecided = 0
    for t in range(16):
        a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
        if t >= 10:
            raw = _cpu(vec.avoidability(a, resolve=False))
            undecided += int((raw["status"] == 2).sum())
            version = vec._version
            got = _cpu(vec.avoidability(a, resolve=True))
            assert vec._version == version
            snap = vec.snapshot_tensors()
            want = _cpu(avoid_states(snap["revealed"], snap["mine"], a, first_click=snap["first_click"]))
            assert (want["status"] != 2).all()
            for k in want:
                assert np.array_equal(got[k], want[k]), (t, k)
        vec.step(a)
    print(f"{board}: {undecided} boards went through the host fallback")
    assert undecided >= 1, "the fallback was not exercised"


@pytest.mark.gpu
@pytest.mark.parametrize("board", ["9x9x10", "8x8x4", "16x16x40", "30x16x99"])
def test_handle_path_matches_states_and_disturbs_nothing(gpu, board):
    """256 envs, 40 safe-biased tape steps: at each step ms_avoid on the handle equals
    ms_avoid_states on a snapshot, and the step after it equals that of a twin env that was
    never analysed (outputs and RNG streams)."""
    from ms_amd import _lib as L
    from ms_amd.avoid import avoid_states
    vec, twin = _vec(gpu, board), _vec(gpu, board)
    gen = torch.Generator().manual_seed(1)
    analysed = searched = 0
    for t in range(40):
        a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
        live = None if t % 3 else (torch.rand(vec.num_envs, generator=gen) < 0.7).to(gpu)
        got = _cpu(vec.avoidability(a, live=live, resolve=False))
        snap = vec.snapshot_tensors()
        want = _cpu(avoid_states(snap["revealed"], snap["mine"], a, first_click=snap["first_click"], live=live))
        for k in want:
            assert np.array_equal(got[k], want[k]), (t, k)
        assert (got["status"] != 2).all(), t
        skipped = ~snap["first_click"].cpu().numpy() if live is None else \
            ~(snap["first_click"] & live).cpu().numpy()
        assert np.array_equal(got["status"] == 0, skipped), t
        analysed += int((got["status"] == 1).sum())
        searched += int((got["max_nodes"] > 0).sum())
        b1, r1, d1, i1 = vec.step(a)
        b2, r2, d2, i2 = twin.step(a)
        assert torch.equal(b1["obs"], b2["obs"]) and torch.equal(b1["action_mask"], b2["action_mask"]), t
        assert torch.equal(r1, r2) and torch.equal(d1, d2), t
        assert all(torch.equal(i1.tensors[k], i2.tensors[k]) for k in i1.tensors), t
    assert np.array_equal(vec.rng_state(), twin.rng_state())
    assert analysed > 1000 and searched > 0


_OLD_KEYS = ("win_rate", "win_ci_low", "win_ci_high", "avg_steps", "avg_progress", "invalid_rate", "wins", "episodes")
_NINE = ("forced_guess_rate", "forced_guess_success_rate", "forced_guess_episode_rate", "safe_option_rate",
         "safe_option_miss_rate", "safe_option_pick_rate", "avg_safe_options_per_turn",
         "avg_frontier_component_size", "avg_selected_component_size")


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["8x8x4", "9x9x10", "16x16x40", "rule_16x16x40", "rule_30x16x99"])
def test_evaluate_vec_diagnostics_match_reference(gpu, run):
    from eval_model import DetModel, RuleModel
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    H, W, K = (int(v) for v in run.replace("rule_", "").split("x"))
    z = np.load(os.path.join(F.GOLDEN, f"eval_vec_{run}.npz"))
    ref = dict(zip([str(k) for k in z["keys"]], z["values"]))
    model = (RuleModel if run.startswith("rule_") else DetModel)().to(gpu)
    kw = dict(episodes=int(z["episodes"]), seed=0, num_envs=int(z["num_envs"]))
    got = evaluate_vec(model, EnvConfig(H=H, W=W, mine_count=K), diagnostics=True, **kw)
    print(run, {k: got[k] for k in _NINE + ("avoid_undecided", "avoid_max_nodes")})
    for k in _NINE:
        assert got[k] == pytest.approx(ref[k], abs=1e-12, nan_ok=True), k
    for k in _OLD_KEYS:
        assert got[k] == pytest.approx(ref[k], abs=1e-12), k
    assert got["belief_ece"] == pytest.approx(ref["belief_ece"], abs=1e-6)
    assert got["belief_auroc"] == pytest.approx(ref["belief_auroc"], abs=2e-3)
    assert got["avoid_undecided"] == 0
    plain = evaluate_vec(model, EnvConfig(H=H, W=W, mine_count=K), **kw)
    assert all(np.isnan(plain[k]) for k in _NINE)
    assert set(plain) == set(ref) and all(plain[k] == got[k] for k in _OLD_KEYS)


@pytest.mark.gpu
def test_evaluate_vec_diagnostics_through_host_fallback(gpu):
    """The same run on an env stream whose device search is cut at 8 nodes: the undecided boards
    go through the host solver inside evaluate_vec and the nine keys still equal the reference's."""
    from eval_model import RuleModel
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.eval import evaluate_vec
    z = np.load(os.path.join(F.GOLDEN, "eval_vec_rule_16x16x40.npz"))
    ref = dict(zip([str(k) for k in z["keys"]], z["values"]))
    cfg = EnvConfig(H=16, W=16, mine_count=40)
    vec = VecMinesweeper(int(z["num_envs"]), cfg, seed=0, device=gpu)
    vec.set_avoid_budget(8)
    got = evaluate_vec(RuleModel().to(gpu), cfg, episodes=int(z["episodes"]), seed=0, num_envs=int(z["num_envs"]),
                       vec=vec, diagnostics=True)
    print("boards through the host fallback:", got["avoid_undecided"])
    assert got["avoid_undecided"] >= 1 and got["avoid_max_nodes"] == 8
    for k in _NINE + _OLD_KEYS:
        assert got[k] == pytest.approx(ref[k], abs=1e-12, nan_ok=True), k
