"""Pins the test references on the CPU. tests/ppo_loss_ref.py (the f64 loss with gradients that
the HIP loss kernels are compared with) against the PyTorch branch of ms_amd.ppo.ppo_losses, which
the G6 golden updates pin to the reference project: terms and the gradients of ``loss`` w.r.t.
logits / value / mine logits at rel 1e-5, on a random case and on the directed tie batch.
tests/sampler_ref.py (the sampler's hash stream on the host): its uniforms are well-formed and
the arg-max test's near-tie filter leaves out at most 5 % of the rows."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import ppo_loss_ref as R
import sampler_ref as S

KEYS = {"policy_loss": 0, "value_loss": 1, "entropy": 2, "aux_bce": 3, "aux_calib": 4, "loss": 5}


def _torch_path(logits, value, mine, batch, cfg):
    from ms_amd.ppo import ppo_losses
    lg = logits.clone().requires_grad_(True)
    v = value.clone().requires_grad_(True)
    mi = mine.clone().requires_grad_(True)

    def model(obs, return_mine=True):
        return (lg, v, mi) if return_mine else (lg, v)
    out = ppo_losses(model, batch, cfg, amp_dtype=None)
    out["loss"].backward()
    return out, lg.grad, v.grad, mi.grad


def _check(logits, value, mine, batch, cfg):
    out, dl, dv, dm = _torch_path(logits, value, mine, batch, cfg)
    terms, leaves = R.ref_terms(logits, value, mine, batch, cfg)
    for k, t in out.items():
        assert float(t) == pytest.approx(float(terms[KEYS[k]]), rel=1e-5, abs=1e-6), k
    gl, gv, gm = R.ref_grads(terms, leaves, [0, 0, 0, 0, 0, 1])
    assert R.rel_l2(dl, gl) <= 1e-5, "dlogits"
    assert R.rel_l2(dv, gv) <= 1e-5, "dvalue"
    assert R.rel_l2(dm, gm.reshape(dm.shape)) <= 1e-5, "dmine"
    assert float(gl[~batch.action_mask].abs().max()) == 0.0
    return terms, (gl, gv, gm)


def test_reference_matches_ppo_losses_random():
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.003, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    logits, value, mine, batch = R.make_outputs(37, 81, torch.float32, seed=5)
    _check(logits, value, mine, batch, cfg)


@pytest.mark.parametrize("clip_eps", [0.25, 0.0])
def test_reference_matches_ppo_losses_on_ties(clip_eps):
    from ms_amd.ppo import PPOConfig
    logits, value, mine, batch, kw = R.tie_batch(clip_eps)
    cfg = PPOConfig(ent_coef=0.01, aux_mine_weight=0.05, aux_mine_calib_weight=0.01, **kw)
    terms, (gl, gv, gm) = _check(logits, value, mine, batch, cfg)
    M = logits.shape[0]
    # the value rows' hand-derived gradients: d loss / dv = vf_coef * TIE_DV / M
    want = torch.tensor([R.TIE_DV[i % 4] for i in range(M)], dtype=torch.float64) * cfg.vf_coef / M
    assert torch.allclose(gv, want, rtol=1e-6, atol=0)
    assert float(gl[0].abs().max()) == 0.0 and float(gl[6].abs().max()) == 0.0  # one legal cell; all masked
    assert float(gl[1].abs().max()) <= cfg.ent_coef  # advantage 0: only the entropy term is left
    # row 8: ratio exactly 1 (on both closed edges when clip_eps = 0) keeps its whole policy gradient
    terms2, leaves = R.ref_terms(logits, value, mine, batch, cfg)
    pl = R.ref_grads(terms2, leaves, [1, 0, 0, 0, 0, 0])[0]
    w8 = torch.zeros(8, dtype=torch.float64)
    w8[5], w8[2] = -0.5 / M, 0.5 / M
    assert torch.allclose(pl[8], w8, rtol=1e-12, atol=0)
    assert bool(torch.isfinite(gl).all()) and all(bool(torch.isfinite(t)) for t in terms)


def test_reference_16bit_convention():
    """amp16 rounds the mine logits and pos_weight, keeps the sigmoid exact, identity gradient."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    logits, value, mine, batch = R.make_outputs(9, 16, torch.float32, seed=2)
    a, _ = R.ref_terms(logits, value, mine, batch, cfg, amp16=torch.float16)
    b, _ = R.ref_terms(logits, value, mine.half().float(), batch, cfg, amp16=torch.float16)
    c, _ = R.ref_terms(logits, value, mine, batch, cfg)
    assert float(a[3]) == float(b[3]) and float(a[4]) == float(b[4])
    assert float(a[3]) != float(c[3])


def test_sampler_host_stream():
    u = S.uniform01(5, 0, np.arange(64), np.arange(81))
    assert u.shape == (64, 81) and u.min() > 0.0 and u.max() < 1.0
    assert np.all((u * 16777216.0 - 0.5) == np.round(u * 16777216.0 - 0.5))  # 24-bit lattice
    assert len(np.unique(u)) > 0.99 * u.size and abs(u.mean() - 0.5) < 0.02
    assert not np.array_equal(u, S.uniform01(5, 1, np.arange(64), np.arange(81)))
    # splitmix64 of 0 (the published first output of the generator seeded with 0)
    assert int(S.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF


def test_sampler_near_tie_filter_leaves_out_at_most_5_percent():
    logits, mask = S.sampler_case()
    keys = S.gumbel_keys(logits.numpy(), mask.numpy(), seed=5, counter=3)
    out = int(S.near_tie_rows(keys).sum())
    assert out <= 0.05 * keys.shape[0], out
