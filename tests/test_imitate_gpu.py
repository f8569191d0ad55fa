"""Imitation warm start end to end (ms_amd/imitate.py, pretrain_il.py): collect_expert is
reproducible and labels every row as VecMinesweeper.expert_targets does; behaviour cloning on a
fixed minibatch lowers the cross entropy; the fp16 fused path stays finite; the checkpoint loads
through Trainer.load_init and through ms_amd.eval."""
from __future__ import annotations

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 9
K = 10
N, T = 64, 8


def _vec(gpu, seed=0):
    from ms_amd import EnvConfig, VecMinesweeper
    return VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)


def _collect(gpu, explore=0.0, seed=3):
    from ms_amd.imitate import collect_expert
    return collect_expert(_vec(gpu), T, budget=1 << 12, method="grouped", explore=explore, seed=seed)


@pytest.fixture(scope="module")
def expert_buffer(gpu):
    """64 envs x 8 steps of the posterior player on 9x9x10, collected once for the module."""
    return _collect(gpu)


def test_collect_is_reproducible_and_explore_changes_it(gpu, expert_buffer):
    again, other = _collect(gpu), _collect(gpu, explore=1.0)
    for k in expert_buffer.FIELDS:
        assert torch.equal(getattr(expert_buffer, k), getattr(again, k)), k
    assert not torch.equal(other.codes, expert_buffer.codes)
    # step 0 is the same under any explore: the boards before their first click carry no target
    for k in expert_buffer.FIELDS:
        assert torch.equal(other.slot(0)[k], expert_buffer.slot(0)[k]), k
    assert not expert_buffer.slot(0)["kind"].any() and not expert_buffer.slot(0)["best"].any()


def test_buffer_rows_are_the_experts_targets(gpu, expert_buffer):
    """Rows are consistent: best within the mask, kind 0 rows empty, labels 0 at revealed cells and
    0 exactly where a safe row's best is set; codes 0 (hidden) exactly at the legal cells; the shares
    add up; a twin env driven by the buffer's own transitions reproduces step 1's targets."""
    b = expert_buffer
    best, mask, kind = b.best.bool(), b.mask, b.kind
    assert len(b) == N * T and not (best & ~mask).any()
    assert torch.equal(best.any(1), kind != 0)
    assert not b.labels[~mask].any() and not b.labels[kind == 0].any()
    assert not b.labels[best & (kind == 1)[:, None]].any() and (b.labels[best & (kind == 2)[:, None]] > 0).all()
    assert torch.equal(b.codes.reshape(len(b), -1) == 0, mask)
    sh = b.kind_shares()
    print(sh)
    assert abs(sum(sh.values()) - 1.0) < 1e-9 and sh["kind_safe"] > 0.25 and sh["kind_none"] >= 1.0 / T
    from ms_amd.rollout import sample_masked
    twin = _vec(gpu)
    m0 = twin.reset()["action_mask"]
    uniform, _ = sample_masked(torch.zeros((N, H * W), device=gpu), m0, 3, 0)
    m1 = twin.step(uniform)[0]["action_mask"]
    assert torch.equal(m1, b.slot(1)["mask"])
    tg = twin.expert_targets(budget=1 << 12, hidden=m1)
    for k in ("best", "kind", "labels"):
        assert torch.equal(tg[k], b.slot(1)[k]), k


def test_continued_collection_starts_where_the_last_one_stopped(gpu):
    from ms_amd.imitate import collect_expert
    vec = _vec(gpu)
    buf = collect_expert(vec, 4, budget=1 << 12, seed=3)
    first = {k: getattr(buf, k).clone() for k in buf.FIELDS}
    _, codes, mask = buf.carry
    codes, mask = codes.clone(), mask.clone()
    whole = _collect(gpu)  # 8 steps from the same reset: its rows 0-3 are the first call's
    for k in buf.FIELDS:
        assert torch.equal(first[k], getattr(whole, k)[:4 * N]), k
    assert torch.equal(codes, whole.slot(4)["codes"]) and torch.equal(mask, whole.slot(4)["mask"])
    buf = collect_expert(vec, 4, budget=1 << 12, seed=4, buffer=buf, reset=False)
    s0 = buf.slot(0)
    assert torch.equal(s0["codes"], codes) and torch.equal(s0["mask"], mask)
    for k in ("best", "kind", "labels"):  # the same boards, so the same targets
        assert torch.equal(s0[k], whole.slot(4)[k]), k
    assert (s0["kind"] != 0).sum() >= N // 2
    with pytest.raises(ValueError, match="continues"):
        collect_expert(_vec(gpu), 4, budget=1 << 12, seed=4, buffer=buf, reset=False)


def _fixed_rows(buf, n=256):
    """The first n rows that carry a target (a fixed minibatch)."""
    rows = torch.nonzero(buf.kind != 0).reshape(-1)[:n]
    assert rows.numel() == n
    return buf.gather(rows)


def test_behaviour_cloning_lowers_the_cross_entropy(gpu, expert_buffer):
    """CNNPolicy, fp32, one fixed minibatch of 256 rows, 40 steps: policy_ce ends strictly below
    step 0 and agree is not lower."""
    from ms_amd.imitate import BCConfig, bc_step
    from ms_amd.models import build_model
    torch.manual_seed(0)
    model = build_model("cnn", obs_shape=(10, H, W), model_cfg={}).to(gpu).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True)
    cfg = BCConfig(aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    batch = _fixed_rows(expert_buffer)
    hist = [bc_step(model, batch, opt, cfg, None, None) for _ in range(40)]
    first = {k: float(v) for k, v in hist[0].items()}
    last = {k: float(v) for k, v in hist[-1].items()}
    print("step 0:", first, "\nstep 39:", last)
    assert all(float(h["bad_rows"]) == 0.0 for h in hist)
    assert last["policy_ce"] < first["policy_ce"]
    assert last["agree"] >= first["agree"]


def test_fp16_residual_model_and_checkpoint(gpu, expert_buffer, tmp_path):
    """The residual model under fp16 autocast (fused trunk and heads) with a GradScaler through
    bc_update: finite loss, bad_rows 0. The Trainer's checkpoint of it loads through
    Trainer.load_init and through ms_amd.eval's command line."""
    from ms_amd import eval as E
    from ms_amd.imitate import BCConfig, bc_losses, bc_update
    from ms_amd.train import PPOTrainConfig, Trainer
    cfg = PPOTrainConfig(H=H, W=W, mine_count=K, num_envs=N, steps_per_env=T, aux_mine_weight=0.05,
                         aux_mine_calib_weight=0.01)
    model_d = {"name": "cnn_residual", "stem_channels": 96, "blocks": 1, "dropout": 0.05, "value_hidden": 32}
    tr = Trainer(cfg, {}, model_d, {}, seed=0, amp="fp16", device=gpu)
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    bc = BCConfig(mini_batches=2, epochs=2, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    st = bc_update(tr.model, expert_buffer, tr.opt, bc, tr.amp_dtype, tr.scaler)
    print(st)
    assert set(st) == {"policy_ce", "agree", "entropy", "aux_bce", "aux_calib", "loss", "bad_rows"}
    assert all(v == v and abs(v) != float("inf") for v in st.values()) and st["bad_rows"] == 0.0
    assert any(not torch.equal(before[k], v) for k, v in tr.model.state_dict().items())
    ckpt = os.path.join(tmp_path, "ckpt_final.pt")
    tr.checkpoint(ckpt)
    fresh = Trainer(cfg, {}, model_d, {}, seed=1, amp="fp16", device=gpu)
    fresh.load_init(ckpt)
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, fresh.model.state_dict()[k]), k
    # the checkpoint is the model that was trained: the fused forward of the live model (its cached
    # 16-bit weight re-layouts) and of the freshly loaded one give the same loss, and not the
    # untrained model's
    batch = _fixed_rows(expert_buffer)
    losses = []
    for m in (tr.model, fresh.model, Trainer(cfg, {}, model_d, {}, seed=0, amp="fp16", device=gpu).model):
        m.eval()
        with torch.no_grad():
            losses.append(float(bc_losses(m, batch, bc, torch.float16)["loss"]))
    print("loss of the live, the reloaded and the untrained model:", losses)
    assert losses[0] == losses[1] and abs(losses[0] - losses[2]) > 1e-3
    conf = os.path.join(tmp_path, "env.yaml")
    with open(conf, "w") as f:
        f.write(f"env:\n  H: {H}\n  W: {W}\n  mine_count: {K}\n")
    E.main(["--ckpt", ckpt, "--config", conf, "--episodes", "16", "--num_envs", "16"])
