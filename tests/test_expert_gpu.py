"""Expert targets on the device (csrc/msexpert.hip k_expert via ms_amd/expert.py) against the host
twin, bitwise: the hand-made rows of tests/expert_rows.py at every size and at row counts that
leave the grid a partial tail; then through VecMinesweeper.expert_targets on live boards: the
action is a legal cell of least mine probability, a provably safe move never loses, an undecided
board carries no target and the handle's posterior budget is put back."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import expert_rows as X

pytestmark = pytest.mark.gpu


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("A", X.SIZES)
def test_device_equals_host_bitwise(gpu, A):
    from ms_amd.expert import expert_targets, expert_targets_host
    for n in (1, 3, 65, 257):
        status, prob, hidden = X.tiled(A, n)
        want = expert_targets_host({"status": status, "prob": prob}, hidden)
        post = {"status": torch.from_numpy(status).to(gpu), "prob": torch.from_numpy(prob).to(gpu)}
        got = expert_targets(post, torch.from_numpy(hidden).to(gpu))
        again = expert_targets(post, torch.from_numpy(hidden).to(gpu) != 0)  # a bool mask, and determinism
        for k in X.OUTPUTS:
            g = got[k].cpu().numpy()
            assert g.dtype == want[k].dtype and g.shape == want[k].shape, (A, n, k)
            assert np.array_equal(_bits(g), _bits(want[k])), (A, n, k)
            assert torch.equal(got[k], again[k]), (A, n, k)
    assert int((want["kind"] == 1).sum()) and int((want["kind"] == 2).sum()) and int((want["kind"] == 0).sum())


def test_null_outputs_and_wrong_inputs(gpu):
    from ms_amd import _lib as L
    from ms_amd.expert import expert_targets
    lib = L.load()
    status, prob, hidden = (torch.from_numpy(a).to(gpu) for a in X.tiled(65, 5))
    want = expert_targets({"status": status, "prob": prob}, hidden)
    for k, (name, dt, cells) in enumerate(L.EXPERT_OUTPUTS):  # one output at a time, the others NULL
        out = torch.empty((5, 65) if cells else (5,), dtype=getattr(torch, dt), device=gpu)
        ptrs = [None] * 5
        ptrs[k] = L.ptr(out)
        L.check(lib.ms_expert_targets(L.ptr(status), L.ptr(prob), L.ptr(hidden), 5, 65, *ptrs, L.stream_ptr(gpu)))
        assert torch.equal(out, want[name]), name
    with pytest.raises(ValueError):
        expert_targets({"status": status, "prob": prob.float()}, hidden)
    with pytest.raises(ValueError):
        expert_targets({"status": status, "prob": prob}, hidden[:, :64])
    with pytest.raises(ValueError):
        expert_targets({"status": status.cpu(), "prob": prob.cpu()}, hidden.cpu())


def _vec(gpu, n=64, seed=3):
    from ms_amd import EnvConfig, VecMinesweeper
    vec = VecMinesweeper(n, EnvConfig(H=9, W=9, mine_count=10), seed=seed, device=gpu)
    mask = vec.reset()["action_mask"]
    return vec, mask


def test_handle_path_after_tape_steps(gpu):
    """9x9x10, 64 envs, 10 uniform tape steps: every board with a target gets a legal action whose
    mine probability is the minimum over its hidden cells; the outputs are the host twin's on the
    device posterior; the action mask and the boards' own revealed plane give the same result."""
    from ms_amd.expert import expert_targets_host
    vec, mask = _vec(gpu)
    for t in range(10):
        mask = vec.step(vec.tape_actions(t))[0]["action_mask"]
    got = vec.expert_targets(budget=1 << 12, method="grouped", hidden=mask)
    own = vec.expert_targets(budget=1 << 12, method="grouped")
    for k in got:
        assert torch.equal(got[k], own[k]), k
    g = {k: v.cpu().numpy() for k, v in got.items()}
    hidden = mask.cpu().numpy()
    want = expert_targets_host(g, hidden)
    for k in X.OUTPUTS:
        assert np.array_equal(_bits(g[k]), _bits(want[k])), k
    has = g["kind"] != 0
    print(f"kinds {np.bincount(g['kind'], minlength=3).tolist()}, "
          f"status {np.bincount(g['status'], minlength=3).tolist()}")
    assert has.sum() >= 32 and (g["kind"] == 1).any()
    rows = np.flatnonzero(has)
    act = g["action"][rows]
    assert hidden[rows, act].all()
    pmin = np.where(hidden, g["prob"], np.inf).min(axis=1)
    assert (g["prob"][rows, act] == pmin[rows]).all()
    assert ((g["status"] == 1) | ~has).all() and (g["action"][~has] == -1).all()


def test_safe_moves_never_lose(gpu):
    """64 envs, 40 steps: boards with a provably safe move (kind 1) take it, the others a uniform
    legal action. No step that took a kind-1 action ends its episode in a loss."""
    from ms_amd import _lib as L
    from ms_amd.rollout import sample_masked
    vec, mask = _vec(gpu, seed=11)
    zeros = torch.zeros((64, 81), device=gpu)
    lost = torch.zeros((), dtype=torch.int64, device=gpu)
    safe_moves = torch.zeros((), dtype=torch.int64, device=gpu)
    losses = torch.zeros((), dtype=torch.int64, device=gpu)
    for t in range(40):
        tg = vec.expert_targets(budget=1 << 12, hidden=mask)
        uniform, _ = sample_masked(zeros, mask, 5, t)
        safe = tg["kind"] == 1
        batch, _, _, infos = vec.step(torch.where(safe, tg["action"], uniform))
        mask = batch["action_mask"]
        loss = infos.tensors["outcome"] == L.MS_OUTCOME_LOSS
        lost += (safe & loss).sum()
        safe_moves += safe.sum()
        losses += loss.sum()
    lost, safe_moves, losses = int(lost), int(safe_moves), int(losses)
    print(f"{safe_moves} provably safe moves, {lost} of them lost; {losses} losses on the other moves")
    assert safe_moves >= 200 and losses >= 1  # the other moves do hit mines: the check can fail
    assert lost == 0


def test_undecided_boards_carry_no_target_and_the_budget_is_put_back(gpu):
    from ms_amd import _lib as L
    vec, mask = _vec(gpu, seed=7)
    for t in range(6):
        mask = vec.step(vec.tape_actions(t))[0]["action_mask"]
    vec.set_posterior_budget(1 << 14)
    before = vec.mine_posterior(resolve=False, method="grouped")
    starved = vec.expert_targets(budget=1, hidden=mask)
    st = starved["status"]
    assert int((st == L.MS_AVOID_UNDECIDED).sum()) >= 1
    none = starved["kind"] == 0
    assert torch.equal(none, st != L.MS_AVOID_DECIDED)
    assert not starved["best"][none].any() and not starved["labels"][none].any()
    assert (starved["action"][none] == -1).all() and (starved["n_best"][none] == 0).all()
    after = vec.mine_posterior(resolve=False, method="grouped")  # at the handle's own budget again
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert int((after["status"] == L.MS_AVOID_DECIDED).sum()) > int((st == L.MS_AVOID_DECIDED).sum())
    with pytest.raises(ValueError, match="method"):
        vec.expert_targets(method="bogus")
