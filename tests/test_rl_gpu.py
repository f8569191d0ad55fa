"""GPU checks of the rollout side: GAE kernel (bit-exact vs the reference
golden and the oracle), masked sampler, on-device collect_rollout replayed
through the oracle, and one PPO update of the trainer."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import oracle as O

pytestmark = pytest.mark.gpu


def test_gae_kernel_golden_bitexact(gpu):
    from ms_amd.buffers import RolloutBuffer
    z = golden("gae.npz")
    T, N = int(z["T"]), int(z["N"])
    b = RolloutBuffer(N, T, (10, 4, 4), 16, gpu)
    b.rewards.copy_(torch.from_numpy(z["rewards"]))
    b.values.copy_(torch.from_numpy(z["values"]))
    b.dones.copy_(torch.from_numpy(z["dones"]))
    b.compute_gae(torch.from_numpy(z["last_values"]).to(gpu), gamma=float(z["gamma"]), lam=float(z["lam"]))
    assert np.array_equal(b.advantages.cpu().numpy(), z["advantages"])
    assert np.array_equal(b.returns.cpu().numpy(), z["returns"])


def test_gae_kernel_vs_oracle_full_size(gpu):
    from ms_amd.buffers import RolloutBuffer
    T, N = 64, 4096
    g = torch.Generator().manual_seed(1)
    r, v = torch.randn(T * N, generator=g), torch.randn(T * N, generator=g)
    d, lv = torch.rand(T * N, generator=g) < 0.3, torch.randn(N, generator=g)
    b = RolloutBuffer(N, T, (10, 1, 1), 1, gpu)
    b.rewards.copy_(r)
    b.values.copy_(v)
    b.dones.copy_(d)
    b.compute_gae(lv.to(gpu))
    adv, ret = O.gae(r.view(T, N).numpy(), v.view(T, N).numpy(), d.view(T, N).numpy(), lv.numpy())
    assert np.array_equal(b.advantages.cpu().numpy(), adv.reshape(-1))
    assert np.array_equal(b.returns.cpu().numpy(), ret.reshape(-1))


def test_sampler_logp_and_mask(gpu):
    from ms_amd.rollout import sample_masked
    g = torch.Generator(device=gpu).manual_seed(0)
    N, A = 4096, 256
    logits = torch.randn(N, A, device=gpu, generator=g) * 3
    mask = torch.rand(N, A, device=gpu, generator=g) < 0.3
    mask[0] = False  # all-invalid row -> treated as all valid (train_rl.py:166-168)
    a, lp = sample_masked(logits, mask, seed=5, counter=0)
    m2 = mask.clone()
    m2[0] = True
    assert bool(m2.gather(1, a[:, None]).all())
    ref = torch.log_softmax(logits.masked_fill(~m2, -float("inf")), -1).gather(1, a[:, None]).squeeze(1)
    torch.testing.assert_close(lp, ref, rtol=1e-5, atol=1e-5)


def _sampler_masks(N, A, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(N, A, generator=g) * 3
    mask = torch.rand(N, A, generator=g) < 0.5
    mask[0] = False  # all-False row: sampled as all valid
    mask[1] = False  # single-True row
    mask[1, A // 2] = True
    return logits, mask


@pytest.mark.parametrize("N,A", [(5, 1), (7, 81), (6, 480), (3, 65)])
def test_sampler_edge_shapes(gpu, N, A):
    """A not a multiple of 64, N not a multiple of 4 (the rows of a workgroup), an all-False and a
    single-True row: every action legal, logp the f64 masked log_softmax at it within 1e-5."""
    from ms_amd.rollout import sample_masked
    logits, mask = _sampler_masks(N, A, seed=N * 1000 + A)
    a, lp = sample_masked(logits.to(gpu), mask.to(gpu), seed=5, counter=2)
    a, lp = a.cpu(), lp.cpu()
    m2 = mask.clone()
    m2[~mask.any(1)] = True  # row 0, and any row the random draw left empty (A = 1)
    assert not bool(mask[0].any()) and int(mask[1].sum()) == 1
    assert int(a.min()) >= 0 and int(a.max()) < A
    assert bool(m2.gather(1, a[:, None]).all())
    ref = torch.log_softmax(logits.double().masked_fill(~m2, -float("inf")), -1).gather(1, a[:, None]).squeeze(1)
    assert float((lp.double() - ref).abs().max()) <= 1e-5


def test_sampler_is_gumbel_argmax_of_documented_hash(gpu):
    """The action is the arg-max of l - log(-log u) with u the documented hash (tests/sampler_ref.py,
    f64 on the host): its key is within 1e-4 of the row maximum (the margin absorbs logf
    differences), and it is the f64 arg-max wherever the runner-up is more than 1e-3 below. With
    24-bit uniforms about 1 % of the rows are such near-ties; here the filter leaves out 0 of the
    64 rows (at most 5 % allowed; tests/test_ppo_loss_ref.py counts them without a GPU)."""
    from ms_amd.rollout import sample_masked
    import sampler_ref as S
    logits, mask = S.sampler_case()
    N = logits.shape[0]
    a, _ = sample_masked(logits.to(gpu), mask.to(gpu), seed=5, counter=3)
    a = a.cpu().numpy()
    keys = S.gumbel_keys(logits.numpy(), mask.numpy(), seed=5, counter=3)
    assert np.all(keys[np.arange(N), a] >= keys.max(1) - 1e-4)
    near = S.near_tie_rows(keys)
    assert near.sum() <= 0.05 * N
    assert np.array_equal(a[~near], keys.argmax(1)[~near])


def test_sampler_shard_invariance(gpu):
    """Rows [k, k + n) sampled alone with row_begin = k: exactly the full call's."""
    from ms_amd.rollout import sample_masked
    N, A, k, n = 11, 81, 4, 5
    logits, mask = _sampler_masks(N, A, seed=3)
    logits, mask = logits.to(gpu), mask.to(gpu)
    a, lp = sample_masked(logits, mask, seed=7, counter=1)
    a2, lp2 = sample_masked(logits[k:k + n], mask[k:k + n], seed=7, counter=1, row_begin=k)
    assert torch.equal(a2, a[k:k + n]) and torch.equal(lp2, lp[k:k + n])
    a3, _ = sample_masked(logits[k:k + n], mask[k:k + n], seed=7, counter=1, row_begin=0)
    assert not torch.equal(a3, a[k:k + n])  # the offset is what selects the stream


def test_sampler_logp_is_the_loss_kernels_logp(gpu):
    """The sampler's (actions, logp) fed back as actions / old_logp on the same logits and mask:
    ratio = 1, so policy_loss = -mean(adv) and its gradient is -(adv / M)(delta_ja - p_j)."""
    from types import SimpleNamespace
    from ms_amd.loss import ppo_loss_terms
    from ms_amd.ppo import PPOConfig
    from ms_amd.rollout import sample_masked
    M, A = 33, 81
    g = torch.Generator(device="cpu").manual_seed(17)
    logits = torch.randn(M, A, generator=g) * 3
    mask = torch.rand(M, A, generator=g) < 0.5
    mask[torch.arange(M), torch.randint(0, A, (M,), generator=g)] = True  # no all-False row
    adv = torch.randn(M, generator=g)
    lg = logits.to(gpu).requires_grad_(True)
    a, lp = sample_masked(lg, mask.to(gpu), seed=2, counter=9)
    z = torch.zeros(M, device=gpu)
    b = SimpleNamespace(action_mask=mask.to(gpu), actions=a, old_logp=lp, advantages=adv.to(gpu), values=z, returns=z)
    t = ppo_loss_terms(lg, z.clone().requires_grad_(True), None, b, PPOConfig(), None, 1, None)
    assert float(t[0]) == pytest.approx(-float(adv.double().mean()), rel=1e-5)
    t[0].backward()
    p = torch.softmax(logits.double().masked_fill(~mask, -float("inf")), -1)
    onehot = torch.zeros(M, A, dtype=torch.float64)
    onehot[torch.arange(M), a.cpu()] = 1.0
    want = -(adv.double() / M)[:, None] * (onehot - p)
    got = lg.grad.double().cpu()
    assert float((got - want).norm() / want.norm()) <= 1e-5
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_sampler_distribution(gpu):
    from ms_amd.rollout import sample_masked
    A = 16
    logits = torch.linspace(-2, 2, A, device=gpu).repeat(20000, 1)
    mask = torch.ones_like(logits, dtype=torch.bool)
    mask[:, 3] = False
    counts = torch.zeros(A, device=gpu)
    for c in range(10):
        a, _ = sample_masked(logits, mask, seed=9, counter=c)
        counts += torch.bincount(a, minlength=A).float()
    p = torch.softmax(logits[0].masked_fill(~mask[0], -float("inf")), -1)
    n = counts.sum()
    assert counts[3] == 0
    exp = p * n
    chi2 = float((((counts - exp) ** 2) / exp.clamp_min(1e-9))[mask[0]].sum())
    assert chi2 < 45.0, chi2  # 14 dof; p ~ 5e-5


def test_collect_rollout_replays_through_oracle(gpu):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.models import build_model
    from ms_amd.rollout import collect_rollout
    H, W, K, N, T = 9, 9, 10, 256, 24
    vec = VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=3)
    torch.manual_seed(0)
    model = build_model("cnn_residual", obs_shape=(10, H, W),
                        model_cfg=dict(stem_channels=16, blocks=1, dropout=0.0, value_hidden=16)).to(gpu).eval()
    buf, aux = collect_rollout(vec, model, T, gpu, aux_mine_weight=0.05, amp_dtype=None)
    o = O.OracleVec(H, W, K, N, seed=3)
    obs0, _ = o.reset()
    assert np.array_equal(buf.obs[:N].cpu().numpy(), obs0)
    acts = buf.actions.view(T, N).cpu().numpy()
    for t in range(T):
        lab, val = o.labels()
        assert np.array_equal(buf.mine_labels[t * N:(t + 1) * N].cpu().numpy(), lab), t
        assert np.array_equal(buf.mine_valid[t * N:(t + 1) * N].cpu().numpy(), val), t
        ref = o.step(acts[t])
        assert np.array_equal(buf.rewards[t * N:(t + 1) * N].cpu().numpy(), ref["reward"]), t
        assert np.array_equal(buf.dones[t * N:(t + 1) * N].cpu().numpy(), ref["done"]), t
        nxt = buf.obs[(t + 1) * N:(t + 2) * N] if t + 1 < T else aux["last_obs"]
        assert np.array_equal(nxt.cpu().numpy(), ref["obs"]), t
    # stored logp / values are the model's on the stored obs (fp32, eval mode)
    with torch.no_grad():
        lg, v = model(buf.obs)
    lp = torch.log_softmax(lg.masked_fill(~buf.action_mask, -1e9), -1).gather(1, buf.actions[:, None]).squeeze(1)
    torch.testing.assert_close(buf.logp, lp, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(buf.values, v, rtol=1e-4, atol=1e-4)
    assert bool(buf.action_mask.gather(1, buf.actions[:, None]).all())


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_trainer_update_runs(gpu, amp):
    """Trainer updates under the default fp16 autocast + GradScaler (the reference's) and
    under bf16: finite stats, parameters move. A GradScaler step skipped for overflow (its
    scale then halves) is the reference's behaviour too, so 4 updates leave room for it."""
    from ms_amd.train import Trainer, load_config
    import os
    cfg, env_d, model_d, extras = load_config(os.path.join(ROOT, "configs", "16x16x40_medium.yaml"))
    cfg.num_envs, cfg.steps_per_env, cfg.total_updates = 256, 8, 4
    model_d = dict(model_d, stem_channels=32, blocks=2, value_hidden=32)
    tr = Trainer(cfg, env_d, model_d, extras, seed=0, device=gpu, amp=amp)
    assert (tr.scaler is not None) == (amp == "fp16")
    before = [p.detach().clone() for p in tr.model.parameters()]
    for u in range(4):
        st = tr.update(u)
        assert all(np.isfinite(v) for v in st.values()), st
        assert {"loss", "policy_loss", "value_loss", "entropy", "aux_bce", "aux_calib"} <= set(st)
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.model.parameters()))
