"""On-policy collection end to end (ms_amd/dagger.py collect_dagger, pretrain_il.py): at beta 1 it
is collect_expert bit for bit and calls no model; at beta 0 a twin env stepped with the model's
greedy legal move reproduces every state and every teacher label; the two collectors continue each
other's games; the fp16 fused forward inside the collector sees the weights bc_update just
trained; pretrain_il's beta schedule reaches the CSV. 9x9x10, 64 envs x 8 steps, budget 2^12,
grouped counting, as tests/test_imitate_gpu.py."""
from __future__ import annotations

import csv
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 9
K = 10
N, T = 64, 8
BUDGET = 1 << 12


def _vec(gpu, seed=0):
    from ms_amd import EnvConfig, VecMinesweeper
    return VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=seed, device=gpu)


class Stub(torch.nn.Module):
    """Logits that are a fixed function of the cell codes, one distinct value per cell and board."""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, codes, return_mine=False):
        assert codes.dtype == torch.uint8 and not torch.is_grad_enabled() and not self.training
        self.calls += 1
        x = codes.reshape(codes.shape[0], -1).float()
        cell = torch.arange(x.shape[1], device=x.device, dtype=torch.float32)
        logits = torch.sin(cell * 0.37 + (x * (cell + 1.0)).sum(1, keepdim=True) * 0.11)
        return logits, torch.zeros(x.shape[0], device=x.device)


class Raises(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("the model must not be called at beta 1")


def _dagger(gpu, model, steps=T, **kw):
    from ms_amd.dagger import collect_dagger
    kw = dict(dict(beta=0.0, budget=BUDGET, method="grouped", explore=0.0, seed=3), **kw)
    return collect_dagger(kw.pop("vec", None) or _vec(gpu), model, steps, **kw)


@pytest.fixture(scope="module")
def expert_buffer(gpu):
    from ms_amd.imitate import collect_expert
    return collect_expert(_vec(gpu), T, budget=BUDGET, method="grouped", explore=0.0, seed=3)


@pytest.fixture(scope="module")
def learner_buffer(gpu):
    """beta 0, explore 0 with the stub: collected once for the module, left unchanged."""
    model = Stub().train()
    buf = _dagger(gpu, model)
    assert model.training and model.calls == T  # one forward per step, and train() is put back
    return buf


def test_beta_one_is_collect_expert_and_calls_no_model(gpu, expert_buffer):
    from ms_amd.dagger import dagger_shares
    buf = _dagger(gpu, Raises(), beta=1.0)
    for k in buf.FIELDS:
        assert torch.equal(getattr(buf, k), getattr(expert_buffer, k)), k
    assert buf.carry[0] is not expert_buffer.carry[0]
    assert torch.equal(buf.carry[1], expert_buffer.carry[1]) and torch.equal(buf.carry[2], expert_buffer.carry[2])
    # and the envs behind the carry stand where the expert's stand: one more step is the same step
    from ms_amd.rollout import sample_masked
    a, _ = sample_masked(torch.zeros((N, H * W), device=gpu), buf.carry[2], 1, 0)  # a legal click per board
    (b0, r0, d0, _), (b1, r1, d1, _) = buf.carry[0].step(a), expert_buffer.carry[0].step(a)
    assert torch.equal(b0["obs"], b1["obs"]) and torch.equal(r0, r1) and torch.equal(d0, d1)
    assert torch.equal(buf.source, (buf.kind != 0).to(torch.uint8))  # the teacher wherever it has a target
    assert (buf.learner_action == -1).all() and not buf.learner_agree.any()
    sh = dagger_shares(buf)
    print(sh)
    assert sh["share_learner"] == 0.0 and sh["on_policy_agree"] == 0.0
    assert abs(sh["share_expert"] + sh["share_uniform"] - 1.0) < 1e-12 and sh["share_uniform"] >= 1.0 / T


def test_beta_zero_plays_the_models_greedy_move_on_every_board(gpu, learner_buffer):
    from ms_amd.dagger import dagger_shares
    from ms_amd.fused import obs_encode
    b = learner_buffer
    assert (b.source == 2).all()
    model = Stub().eval()
    twin = _vec(gpu)
    first = twin.reset()
    codes, mask = torch.empty((N, H, W), dtype=torch.uint8, device=gpu), first["action_mask"]
    obs_encode(first["obs"], codes)
    rewards = torch.empty(N, dtype=torch.float32, device=gpu)
    dones = torch.empty(N, dtype=torch.bool, device=gpu)
    for t in range(T):
        s = b.slot(t)
        assert torch.equal(s["codes"], codes) and torch.equal(s["mask"], mask), t
        tg = twin.expert_targets(budget=BUDGET, method="grouped", hidden=mask)
        for k in ("best", "kind", "labels"):
            assert torch.equal(s[k], tg[k]), (k, t)
        with torch.no_grad():
            logits = model(codes)[0]
        action = logits.masked_fill(~mask, -1e9).argmax(dim=-1)  # evaluate_vec's rule
        rows = slice(t * N, (t + 1) * N)
        assert torch.equal(b.learner_action[rows], action), t
        has = tg["kind"] != 0
        agree = tg["best"].gather(1, action[:, None])[:, 0]
        assert torch.equal(b.learner_agree[rows][has], agree[has]) and not b.learner_agree[rows][~has].any()
        codes, mask = torch.empty_like(codes), torch.empty_like(mask)
        twin.step(action, out={"codes": codes, "action_mask": mask, "rewards": rewards, "dones": dones})
    assert torch.equal(b.carry[1], codes) and torch.equal(b.carry[2], mask)
    sh = dagger_shares(b)
    print(sh)
    assert sh["share_learner"] == 1.0 and sh["share_expert"] == 0.0 and sh["share_uniform"] == 0.0
    has = b.kind != 0
    assert sh["on_policy_agree"] == int(b.learner_agree[has].sum()) / int(has.sum()) and sh["on_policy_agree"] < 1.0
    assert (b.kind != 0).sum() >= N  # the stub's clicks open boards: the teacher has targets to label


def test_continuation_within_and_across_the_two_collectors(gpu, learner_buffer, expert_buffer):
    from ms_amd.dagger import collect_dagger
    from ms_amd.imitate import collect_expert
    model = Stub()
    vec = _vec(gpu)
    buf = _dagger(gpu, model, steps=4, vec=vec)
    for k in buf.FIELDS:
        assert torch.equal(getattr(buf, k), getattr(learner_buffer, k)[:4 * N]), k
    # the counter restarts with every call, so only a greedy learner at explore 0 continues bitwise
    buf = _dagger(gpu, model, steps=4, vec=vec, buffer=buf, reset=False, seed=99)
    for k in buf.FIELDS:
        assert torch.equal(getattr(buf, k), getattr(learner_buffer, k)[4 * N:]), k
    assert torch.equal(buf.carry[1], learner_buffer.carry[1]) and torch.equal(buf.carry[2], learner_buffer.carry[2])
    with pytest.raises(ValueError, match="continues"):
        _dagger(gpu, model, steps=4, buffer=buf, reset=False)
    # an expert round, then a DAgger round on the same vec and buffer: the same games go on
    vec = _vec(gpu)
    buf = collect_expert(vec, 4, budget=BUDGET, method="grouped", explore=0.0, seed=3)
    assert torch.equal(buf.codes, expert_buffer.codes[:4 * N])
    buf = collect_dagger(vec, model, 4, beta=0.5, explore=0.3, budget=BUDGET, seed=4, buffer=buf, reset=False)
    s0, e4 = buf.slot(0), expert_buffer.slot(4)
    for k in buf.FIELDS:  # the boards the expert round stopped at, with the targets they have
        assert torch.equal(s0[k], e4[k]), k
    assert (s0["kind"] != 0).sum() >= N // 2 and len(set(buf.source.tolist())) == 3
    # and back: collect_expert continues a DAgger round's carry
    codes, mask = buf.carry[1].clone(), buf.carry[2].clone()
    buf = collect_expert(vec, 4, budget=BUDGET, method="grouped", seed=5, buffer=buf, reset=False)
    assert torch.equal(buf.slot(0)["codes"], codes) and torch.equal(buf.slot(0)["mask"], mask)


def test_the_models_mode_is_restored(gpu):
    for training in (True, False):
        model = Stub().train(training)
        _dagger(gpu, model, steps=1, beta=0.5)
        assert model.training is training and model.calls == 1

    class Fails(Stub):
        def forward(self, codes, return_mine=False):
            raise RuntimeError("boom")

    model = Fails().train()
    with pytest.raises(RuntimeError, match="boom"):
        _dagger(gpu, model, steps=1)
    assert model.training


def test_fp16_collector_sees_the_weights_just_trained(gpu):
    """cnn_residual (96 channels, 1 block) under fp16 autocast: the no-grad forward inside the
    collector is the fused one, whose 16-bit weight re-layouts bc_step drops after every optimizer
    step. Same envs, same seeds: the learner's moves before and after bc_update differ only if the
    second collection's forward ran on the new weights."""
    from ms_amd.imitate import BCConfig, bc_update
    from ms_amd.train import PPOTrainConfig, Trainer
    cfg = PPOTrainConfig(H=H, W=W, mine_count=K, num_envs=N, steps_per_env=T, aux_mine_weight=0.05,
                         aux_mine_calib_weight=0.01)
    model_d = {"name": "cnn_residual", "stem_channels": 96, "blocks": 1, "dropout": 0.05, "value_hidden": 32}
    tr = Trainer(cfg, {}, model_d, {}, seed=0, amp="fp16", device=gpu)
    tr.model.train()
    first = _dagger(gpu, tr.model, amp=torch.float16)
    again = _dagger(gpu, tr.model, amp=torch.float16)
    assert tr.model.training
    assert torch.equal(first.learner_action, again.learner_action) and torch.equal(first.codes, again.codes)
    assert ((first.learner_action >= 0) & (first.learner_action < H * W)).all()
    assert first.mask.gather(1, first.learner_action[:, None]).all()  # legal moves
    bc = BCConfig(mini_batches=2, epochs=2, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    st = bc_update(tr.model, first, tr.opt, bc, tr.amp_dtype, tr.scaler)
    print(st)
    assert st["bad_rows"] == 0.0 and all(v == v and abs(v) != float("inf") for v in st.values())
    second = _dagger(gpu, tr.model, amp=torch.float16)
    changed = int((second.learner_action != first.learner_action).sum())
    print("learner moves changed by one bc_update:", changed, "of", len(first))
    assert changed > 0
    assert torch.equal(second.slot(0)["codes"], first.slot(0)["codes"])  # from the same reset


def test_pretrain_il_beta_schedule(gpu, tmp_path):
    from ms_amd import eval as E
    from ms_amd.imitate import main
    conf = os.path.join(tmp_path, "il.yaml")
    with open(conf, "w") as f:
        f.write(f"env:\n  H: {H}\n  W: {W}\n  mine_count: {K}\n"
                "model:\n  name: cnn_residual\n  stem_channels: 96\n  blocks: 1\n  dropout: 0.05\n  value_hidden: 32\n"
                "ppo:\n  lr: 0.0003\n  aux_mine_weight: 0.05\n  aux_mine_calib_weight: 0.01\n"
                f"imitation:\n  num_envs: {N}\n  steps_per_env: {T}\n  mini_batches: 2\n  budget: {BUDGET}\n")
    out = os.path.join(tmp_path, "run")
    main(["--config", conf, "--out", out, "--iters", "3", "--beta_start", "1", "--beta_end", "0",
          "--beta_decay_iters", "2"])
    with open(os.path.join(out, "train_metrics.csv")) as f:
        rows = list(csv.DictReader(f))
    assert [int(r["iter"]) for r in rows] == [1, 2, 3]
    assert [float(r["beta"]) for r in rows] == [1.0, 0.5, 0.0]
    for k in ("share_learner", "share_expert", "share_uniform", "on_policy_agree"):
        assert k in rows[0], k
    share = [float(r["share_learner"]) for r in rows]
    print("share_learner per round:", share, "on_policy_agree:", [r["on_policy_agree"] for r in rows])
    assert share[0] == 0.0 and 0.0 < share[1] < share[2] and share[2] > 0.9  # explore keeps 5 %
    assert all(0.0 <= float(r["on_policy_agree"]) <= 1.0 for r in rows[1:])
    assert float(rows[0]["bad_rows"]) == 0.0 and float(rows[2]["bad_rows"]) == 0.0
    E.main(["--ckpt", os.path.join(out, "ckpt_final.pt"), "--config", conf, "--episodes", "16", "--num_envs", "16"])
