"""The exact posterior as belief targets: ms_posterior_labels (csrc/msposterior.hip's search with
the label output stage) through VecMinesweeper.posterior_labels, collect_rollout(belief_targets=
"posterior") and the trainer. The kernel is checked against its parts, which have tests of their
own: ms_posterior (tests/test_posterior_gpu.py) and ms_labels (tests/test_env_gpu.py)."""
from __future__ import annotations

import csv

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOARDS = ["9x9x10", "8x8x4", "16x16x40"]


def _vec(gpu, board, n=67, seed=3):
    from ms_amd import EnvConfig, VecMinesweeper
    H, W, K = (int(v) for v in board.split("x"))
    vec = VecMinesweeper(n, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)
    vec.reset()
    return vec, K


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_labels_equal_their_parts(gpu):
    """67 envs, 12 safe-biased tape steps, budgets 2^12 and 8, the handle's budget set to the same:
    valid is ms_labels' everywhere; labels are ms_posterior's p rounded to f32 where it decided
    (bitwise), ms_labels' 0 / 1 mask where it did not (bitwise), 0 before the first click. On a
    decided board sum(labels * valid) is the mine count within 1e-4 (f32 rounding of at most 480
    terms in [0, 1]: 480 * 2^-25 = 1.4e-5). Every class of board has to occur."""
    from ms_amd import _lib as L
    seen = {(b, s): 0 for b in (1 << 12, 8) for s in (0, 1, 2)}
    step0_source0 = 0
    for board in BOARDS:
        for budget in (1 << 12, 8):
            vec, K = _vec(gpu, board)
            vec.set_posterior_budget(budget)
            n, A = vec.num_envs, vec.H * vec.W
            for t in range(12):
                where = (board, budget, t)
                a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
                post = vec.mine_posterior(resolve=False)
                hard, hvalid = vec.mine_labels()
                labels, valid, source = vec.posterior_labels(budget=budget)
                assert labels.dtype == torch.float32 and valid.dtype == torch.bool and source.dtype == torch.uint8
                assert labels.shape == valid.shape == (n, vec.H, vec.W) and source.shape == (n,)
                assert torch.equal(valid, hvalid), where
                assert torch.equal(source, post["status"]), where
                st = post["status"]
                lab, hd = labels.reshape(n, A), hard.reshape(n, A)
                want = torch.where((st == 1)[:, None], post["prob"].to(torch.float32), hd)
                want = torch.where((st == 0)[:, None], torch.zeros_like(want), want)
                assert torch.equal(_bits(lab), _bits(want)), where
                assert not lab[st == 0].any(), where
                dec = st == 1
                total = (lab.double() * valid.reshape(n, A)).sum(1)
                if bool(dec.any()):
                    assert float((total[dec] - K).abs().max()) <= 1e-4, where
                assert bool(((lab >= 0) & (lab <= 1)).all()), where
                for s in (0, 1, 2):
                    seen[(budget, s)] += int((source == s).sum())
                if t == 0:
                    step0_source0 += int((source == 0).sum())
                    assert bool((source == 0).all()), where
                vec.step(a)
    print("boards by (budget, source):", seen)
    assert step0_source0 > 0
    assert seen[(8, 2)] > 0, "no board ran out of a budget of 8 nodes"
    assert seen[(8, 1)] > 0 and seen[(1 << 12, 1)] > 0
    soft = 0  # the targets are not hard labels in disguise: some decided cell is strictly inside (0, 1)
    vec, K = _vec(gpu, "9x9x10")
    for t in range(3):
        vec.step(vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED))
    labels, _, source = vec.posterior_labels()
    soft = int(((labels > 0) & (labels < 1)).reshape(vec.num_envs, -1)[source == 1].sum())
    assert soft > 0


def test_labels_in_place_and_read_only(gpu):
    """Outputs that are views into a canary-filled RolloutBuffer (slot 1 of 3): nothing outside the
    slot is written. The step after the call is that of a twin env that was never analysed; the
    handle's own budget is not touched; each output may be NULL; a budget out of range is
    MS_EINVAL and launches nothing."""
    from ms_amd import _lib as L
    from ms_amd.buffers import RolloutBuffer
    (vec, K), (twin, _) = _vec(gpu, "9x9x10"), _vec(gpu, "9x9x10")
    n, H, W = vec.num_envs, vec.H, vec.W
    for t in range(5):
        a = vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED)
        vec.step(a)
        twin.step(a)
    vec.set_posterior_budget(8)
    before = vec.mine_posterior(resolve=False)
    buf = RolloutBuffer(n, 3, (10, H, W), H * W, gpu, with_mine_labels=True, with_mine_source=True)
    buf.mine_labels.fill_(-7.0)
    buf.mine_valid.view(torch.uint8).fill_(0xAB)
    buf.mine_source.fill_(0xCD)
    s = buf.slot(1)
    got = vec.posterior_labels(s["mine_labels"], s["mine_valid"], s["mine_source"], budget=1 << 12)
    assert got[0].data_ptr() == s["mine_labels"].data_ptr() and got[2].data_ptr() == s["mine_source"].data_ptr()
    fresh = vec.posterior_labels(budget=1 << 12)
    for g, f in zip(got, fresh):
        assert torch.equal(g, f)
    for k in (0, 2):
        rows = slice(k * n, (k + 1) * n)
        assert bool((buf.mine_labels[rows] == -7.0).all())
        assert bool((buf.mine_valid.view(torch.uint8)[rows] == 0xAB).all())
        assert bool((buf.mine_source[rows] == 0xCD).all())
    assert bool((buf.mine_source[n:2 * n] <= 2).all())
    after = vec.mine_posterior(resolve=False)  # still the handle's budget of 8
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # max_nodes as ms_posterior's at the same budget; NULL outputs one at a time
    lib, stream = L.load(), L.stream_ptr(gpu)
    full = [torch.empty((n, H, W), dtype=torch.float32, device=gpu), torch.empty((n, H, W), dtype=torch.uint8, device=gpu),
            torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(n, dtype=torch.int32, device=gpu)]
    L.check(lib.ms_posterior_labels(vec._h, 8, *(L.ptr(x) for x in full), stream))
    assert torch.equal(full[3], before["max_nodes"]) and torch.equal(full[2], before["status"])
    for skip in range(4):
        outs = [torch.empty_like(x) for x in full]
        L.check(lib.ms_posterior_labels(vec._h, 8, *(None if i == skip else L.ptr(x) for i, x in enumerate(outs)), stream))
        for i in range(4):
            if i != skip:
                assert torch.equal(outs[i], full[i]), (skip, i)
    L.check(lib.ms_posterior_labels(vec._h, 8, None, None, None, None, stream))
    for bad in (0, (1 << 30) + 1, -1):
        canary = torch.full((n,), 0xCD, dtype=torch.uint8, device=gpu)
        assert lib.ms_posterior_labels(vec._h, bad, None, None, L.ptr(canary), None, stream) == 1  # MS_EINVAL
        assert b"budget" in lib.ms_last_error()
        with pytest.raises(L.MsEnvError):
            vec.posterior_labels(budget=bad)
        assert bool((canary == 0xCD).all())
    assert lib.ms_posterior_labels(None, 8, None, None, None, None, stream) == 1
    # the analysed env goes on exactly as its twin
    a = vec.tape_actions(5, L.MS_TAPE_SAFE_BIASED)
    b1, r1, d1, _ = vec.step(a)
    b2, r2, d2, _ = twin.step(a)
    assert torch.equal(b1["obs"], b2["obs"]) and torch.equal(b1["action_mask"], b2["action_mask"])
    assert torch.equal(r1, r2) and torch.equal(d1, d2)
    assert np.array_equal(vec.rng_state(), twin.rng_state())


def _rollout(gpu, seed=5, **kw):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.models import build_model
    from ms_amd.rollout import collect_rollout
    H, W, K, N, T = 8, 8, 10, 64, 6
    vec = VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)
    torch.manual_seed(0)
    model = build_model("cnn_residual", obs_shape=(10, H, W),
                        model_cfg=dict(stem_channels=16, blocks=1, dropout=0.0, value_hidden=16)).to(gpu).eval()
    buf, aux = collect_rollout(vec, model, T, gpu, aux_mine_weight=0.05, amp_dtype=None, sample_seed=9, **kw)
    return buf, aux, (H, W, K, N, T)


_BUFFER_TENSORS = ("obs", "action_mask", "actions", "logp", "rewards", "dones", "values", "mine_labels", "mine_valid")


@pytest.mark.parametrize("budget", [None, 16])
def test_rollout_posterior_targets(gpu, budget):
    """8x8x10, 64 envs x 6 steps: the buffer's targets at each step are those of a twin env that
    replays the recorded actions; everything else in the buffer is the hard-mode rollout's."""
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.posterior import TRAIN_BUDGET
    buf, _, (H, W, K, N, T) = _rollout(gpu, belief_targets="posterior", posterior_budget=budget)
    assert buf.mine_source is not None and buf.mine_source.shape == (T * N,) and buf.mine_source.dtype == torch.uint8
    assert set(buf.slot(0)) >= {"mine_labels", "mine_valid", "mine_source"}
    twin = VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=5, device=gpu)
    twin.reset()
    acts = buf.actions.view(T, N)
    for t in range(T):
        rows = slice(t * N, (t + 1) * N)
        labels, valid, source = twin.posterior_labels(budget=TRAIN_BUDGET if budget is None else budget)
        assert torch.equal(_bits(buf.mine_labels[rows]), _bits(labels)), t
        assert torch.equal(buf.mine_valid[rows], valid), t
        assert torch.equal(buf.mine_source[rows], source), t
        twin.step(acts[t])
    assert bool((buf.mine_source[:N] == 0).all()) and bool((buf.mine_source[N:] == 1).any())
    hard, _, _ = _rollout(gpu)
    for k in _BUFFER_TENSORS:
        if k != "mine_labels":
            assert torch.equal(getattr(buf, k), getattr(hard, k)), k


def test_rollout_hard_targets_unchanged(gpu):
    """belief_targets="hard" is the call without the argument, tensor for tensor, and carries no
    mine_source; a buffer of the other mode is not reused."""
    plain, aux0, _ = _rollout(gpu)
    hard, aux1, _ = _rollout(gpu, belief_targets="hard", posterior_budget=4)
    assert plain.mine_source is None and hard.mine_source is None
    assert "mine_source" not in hard.slot(0)
    for k in _BUFFER_TENSORS:
        assert torch.equal(getattr(plain, k), getattr(hard, k)), k
    assert torch.equal(aux0["last_values"], aux1["last_values"]) and torch.equal(aux0["last_obs"], aux1["last_obs"])
    assert bool(((plain.mine_labels == 0) | (plain.mine_labels == 1)).all())
    soft, _, _ = _rollout(gpu, belief_targets="posterior")
    back, _, _ = _rollout(gpu, belief_targets="hard", buffer=soft)
    assert back is not soft and back.mine_source is None
    again, _, _ = _rollout(gpu, belief_targets="posterior", buffer=soft)
    assert again is soft
    with pytest.raises(ValueError):
        _rollout(gpu, belief_targets="soft")


_CFG = """
env: {{H: 8, W: 8, mine_count: 10}}
model: {{name: cnn_residual, stem_channels: 96, blocks: 1, dropout: 0.05, value_hidden: 32}}
ppo: {{num_envs: 64, steps_per_env: 8, mini_batches: 2, ppo_epochs: 1, total_updates: 2, lr: 0.0003,
      aux_mine_weight: 0.05, aux_mine_calib_weight: 0.01}}
training: {{early_stop_patience: 100{extra}}}
"""
# Trainer.update's keys and the header of train_metrics.csv as the commit before this feature
# writes them for this configuration (belief losses on, no profiling)
_PARENT_STATS = ["aux_bce", "aux_calib", "aux_weight", "ent_coef", "entropy", "loss", "policy_loss", "value_loss"]
_PARENT_CSV = ["aux_bce", "aux_calib", "aux_weight", "ent_coef", "entropy", "loss", "policy_loss", "quick_belief_auroc",
               "quick_belief_ece", "quick_forced_guess_rate", "quick_guess_success", "quick_guesses_per_ep",
               "quick_safe_option_pick_rate", "quick_score", "quick_win_rate", "seconds", "steps", "update",
               "value_loss"]
_MAIN = ["--eval_quick_episodes", "0", "--skip_final_eval", "--save_every", "100"]


def _train(tmp_path, name, extra, flags=()):
    from ms_amd.train import main
    cfg = tmp_path / f"{name}.yaml"
    cfg.write_text(_CFG.format(extra=extra))
    out = tmp_path / name
    main(["--config", str(cfg), "--out", str(out), *_MAIN, *flags])
    with open(out / "train_metrics.csv") as f:
        r = csv.DictReader(f)
        return list(r.fieldnames), list(r)


def test_trainer_posterior_targets(gpu, tmp_path):
    """Two updates at 8x8x10 with belief_targets: posterior (from the flag over a YAML that says
    hard; then one update with the key and a budget from the YAML): finite losses, belief_exact_frac in (0, 1], the CSV has the column.
    Default mode: stats keys and CSV header are the parent's, literally."""
    from ms_amd.train import Trainer, load_config
    header, rows = _train(tmp_path, "flag", ", belief_targets: hard", ("--belief_targets", "posterior"))
    assert header == sorted(_PARENT_CSV + ["belief_exact_frac"])
    assert len(rows) == 2
    for r in rows:
        assert 0.0 < float(r["belief_exact_frac"]) <= 1.0, r
        assert all(np.isfinite(float(r[k])) for k in _PARENT_STATS), r
    header, rows = _train(tmp_path, "default", "")
    assert header == _PARENT_CSV and len(rows) == 2
    cfg, env_d, model_d, extras = load_config(str(tmp_path / "default.yaml"))
    tr = Trainer(cfg, env_d, model_d, extras, seed=0, device=gpu)
    assert tr.belief_targets == "hard"
    st = tr.update(0)
    assert sorted(st) == _PARENT_STATS and tr.buffer.mine_source is None
    (tmp_path / "yaml.yaml").write_text(_CFG.format(extra=", belief_targets: posterior, posterior_budget: 64"))
    cfg, env_d, model_d, extras = load_config(str(tmp_path / "yaml.yaml"))
    tr = Trainer(cfg, env_d, model_d, extras, seed=0, device=gpu)
    assert (tr.belief_targets, tr.posterior_budget) == ("posterior", 64)
    st = tr.update(0)
    assert sorted(st) == sorted(_PARENT_STATS + ["belief_exact_frac"])
    assert all(np.isfinite(v) for v in st.values()) and 0.0 < st["belief_exact_frac"] <= 1.0
    src = tr.buffer.mine_source
    assert st["belief_exact_frac"] == pytest.approx(float((src == 1).sum()) / float((src != 0).sum()), abs=1e-6)
