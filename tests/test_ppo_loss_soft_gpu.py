"""The PPO loss on soft belief targets: labels anywhere in [0, 1] (the exact posterior of
VecMinesweeper.posterior_labels) instead of 0 / 1. The HIP loss (csrc/msppo.hip) and the PyTorch
ops of ms_amd/ppo.py go against the f64 reference of tests/ppo_loss_ref.py, whose ref_terms takes
any y, with the bounds and comparisons tests/test_ppo_loss_gpu.py uses for hard labels (imported
from there): f32 terms rel 1e-5 / abs 1e-6, each gradient tensor rel-L2 1e-5; 16-bit: the fused
path's error at most twice the PyTorch path's own (or its measured floor)."""
from __future__ import annotations

import pytest
import torch

import ppo_loss_ref as R
from test_ppo_loss_gpu import _CFG, _against_reference, _bound16, _run

pytestmark = pytest.mark.gpu

_LOSS, _BCE, _CAL = [0, 0, 0, 0, 0, 1.0], [0, 0, 0, 1.0, 0, 0], [0, 0, 0, 0, 1.0, 0]


def _soft_outputs(A):
    """make_outputs(M = 9) with uniform [0, 1) labels; in every row some are exactly 0, exactly 1
    and 2^-24 (half an f32 ulp of 1: 1 - y rounds to 1), on valid and on not-valid cells alike."""
    logits, value, mine, b = R.make_outputs(9, A, torch.float32, seed=300 + A)
    g = torch.Generator(device="cpu").manual_seed(A)
    y = torch.rand(9, A, generator=g)
    y[:, 0::9] = 0.0
    y[:, 1::9] = 1.0
    y[:, 2::9] = 2.0 ** -24
    assert bool(((y > 2.0 ** -24) & (y < 1)).any()) and float(y.min()) == 0.0 and float(y.max()) == 1.0
    for v in (0.0, 1.0, 2.0 ** -24):
        assert bool(((y == v) & b.mine_valid).any())
    b.mine_labels = y
    return logits, value, mine, b


@pytest.mark.parametrize("A", [81, 256, 480], ids=["9x9", "16x16", "30x16"])
def test_fused_loss_soft_labels_vs_f64(gpu, A):
    """f32: the six terms and the gradients of loss, aux_bce and aux_calib one at a time."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b = _soft_outputs(A)
    _against_reference(gpu, logits, value, mine, b, PPOConfig(**_CFG), [_LOSS, _BCE, _CAL])


@pytest.mark.parametrize("A", [81, 256, 480], ids=["9x9", "16x16", "30x16"])
def test_fused_loss_soft_labels_fp16_vs_f64(gpu, A):
    """amp16 = float16: fused and PyTorch paths each against the f64 reference of the rounded inputs."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b = _soft_outputs(A)
    _bound16(gpu, logits, value, mine, b, PPOConfig(**_CFG), torch.float16)


@pytest.mark.parametrize("A", [81, 256, 480], ids=["9x9", "16x16", "30x16"])
def test_torch_loss_soft_labels_vs_f64(gpu, A):
    """The PyTorch-ops path (ms_amd.loss.FUSED_LOSS off) in f32 against the same reference, at the
    same tolerances."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(**_CFG)
    logits, value, mine, b = _soft_outputs(A)
    terms, rleaves = R.ref_terms(logits, value, mine, b, cfg)
    want = R.ref_grads(terms, rleaves, _LOSS)
    out, dl, dv, dm = _run(False, logits.to(gpu), value.to(gpu), mine.to(gpu), R.batch_to(b, gpu), cfg, None, scale=1.0)
    for k, name in enumerate(R.TERMS):
        assert out[name] == pytest.approx(float(terms[k]), rel=1e-5, abs=1e-6), name
    for name, a, w in zip(("dlogits", "dvalue", "dmine"), (dl, dv, dm), want):
        assert R.rel_l2(a, w.reshape(a.shape)) <= 1e-5, name
