"""The HIP PPO loss (csrc/msppo.hip via ms_amd/loss.py) against ms_amd/ppo.py's PyTorch ops of the
same loss (ppo.py:33-87) on the same model outputs: the loss terms and the gradients of the
scaled loss w.r.t. the policy logits, the value prediction and the belief logits.

Tolerances: f32 everywhere (fp32 path): terms rel 1e-5, gradients rel-norm 1e-5 per tensor.
Under 16-bit autocast the value gradient is rounded to the value's type and the belief-logit
gradient passes through the 16-bit casts as autocast's do: rel-norm 2e-3 there (a few 16-bit
roundings placed differently), f32 tolerances elsewhere. The G6 golden updates run through this
path too (tests/test_parity_gpu.py).

And against an independent f64 reference with gradients (tests/ppo_loss_ref.py, pinned to
ppo_losses' PyTorch branch on the CPU by tests/test_ppo_loss_ref.py), in fp32 mode at the same
tolerances (terms rel 1e-5 / abs 1e-6, each gradient tensor rel-L2 1e-5, masked cells' dlogits
exactly 0): the backward of every single output and of a random combination of the six; the
grid-stride loop (M = 16,391 rows, three passes); both sides of the NQ dispatch (A = 64 ... 257);
a directed batch of bitwise ties, closed clamp edges, an all-masked row and +-60 logits; a
globally empty valid set. With 16-bit logits / value / mine logits, the fused path's error against
the f64 reference is at most twice the PyTorch path's own. Then the defects once recorded in
ADVICE.md: no BCE gradient without a BCE weight (fp16 pos_weight = inf), NaN-propagating
min / max / clamp, masks of any dtype, out-of-range actions counted in out[6]."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ppo_loss_ref as R

pytestmark = pytest.mark.gpu


def _outputs(M, A, dev, vdt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = (torch.randn(M, A, generator=g) * 3).to(dev)
    mask = torch.rand(M, A, generator=g) < 0.7
    actions = torch.randint(0, A, (M,), generator=g)
    mask[torch.arange(M), actions] = True
    mask[0] = False  # a row whose only legal cell is the action
    mask[0, actions[0]] = True
    value = (torch.randn(M, generator=g)).to(vdt).to(dev)
    mine = (torch.randn(M, 1, A, generator=g) * 2).to(dev)
    labels = (torch.rand(M, A, generator=g) < 0.15).float()
    valid = torch.rand(M, A, generator=g) < 0.6
    if M > 1:
        valid[1] = False  # a row with no valid cell
    # old log-probs near the current ones: ratios on both sides of the clip range
    with torch.no_grad():
        lp = torch.log_softmax(logits.cpu().masked_fill(~mask, -1e9), -1)[torch.arange(M), actions]
    old = lp + torch.randn(M, generator=g) * 0.3
    batch = SimpleNamespace(obs=torch.zeros(M, 1, device=dev), action_mask=mask.to(dev), actions=actions.to(dev),
                            old_logp=old.to(dev), advantages=torch.randn(M, generator=g).to(dev),
                            values=(value.float().cpu() + torch.randn(M, generator=g) * 0.3).to(dev),
                            returns=(value.float().cpu() + torch.randn(M, generator=g)).to(dev),
                            mine_labels=labels.to(dev), mine_valid=valid.to(dev))
    return logits, value, mine, batch


def _run(fused, logits, value, mine, batch, cfg, amp, scale=1024.0):
    from ms_amd import loss as LS
    from ms_amd.ppo import ppo_losses
    lg = logits.clone().requires_grad_(True)
    v = value.clone().requires_grad_(True)
    mi = mine.clone().requires_grad_(True)

    def model(obs, return_mine=True):
        return (lg, v, mi) if return_mine else (lg, v)
    old = LS.FUSED_LOSS
    LS.FUSED_LOSS = fused
    try:
        out = ppo_losses(model, batch, cfg, amp_dtype=amp)
    finally:
        LS.FUSED_LOSS = old
    (out["loss"] * scale).backward()
    return {k: float(t) for k, t in out.items()}, lg.grad, v.grad, mi.grad


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("A", [81, 256, 480], ids=["9x9", "16x16", "30x16"])
@pytest.mark.parametrize("amp", [None, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_fused_loss_matches_torch(gpu, A, amp):
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.003, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    vdt = amp or torch.float32
    logits, value, mine, batch = _outputs(2048 + 37, A, gpu, vdt, seed=A)
    ctx = torch.autocast("cuda", dtype=amp) if amp else torch.autocast("cuda", enabled=False)
    with ctx:
        f = _run(True, logits, value, mine, batch, cfg, amp)
        t = _run(False, logits, value, mine, batch, cfg, amp)
    assert set(f[0]) == set(t[0]) == {"loss", "policy_loss", "value_loss", "entropy", "aux_bce", "aux_calib"}
    for k in t[0]:
        assert f[0][k] == pytest.approx(t[0][k], rel=1e-5, abs=1e-6), k
    assert _rel(f[1], t[1]) <= 1e-5, "dlogits"
    assert f[2].dtype == t[2].dtype == vdt
    assert _rel(f[2], t[2]) <= (1e-5 if amp is None else 2e-3), "dvalue"
    assert _rel(f[3], t[3]) <= (1e-5 if amp is None else 2e-3), "dmine"
    assert float(f[1][~batch.action_mask].abs().max()) == 0.0  # masked cells get no gradient


def test_fused_loss_without_belief_terms(gpu):
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.01)
    logits, value, mine, batch = _outputs(1000, 256, gpu, torch.float32, seed=3)
    f = _run(True, logits, value, mine, batch, cfg, None)
    t = _run(False, logits, value, mine, batch, cfg, None)
    assert set(f[0]) == set(t[0]) == {"loss", "policy_loss", "value_loss", "entropy"}
    for k in t[0]:
        assert f[0][k] == pytest.approx(t[0][k], rel=1e-5, abs=1e-6), k
    assert _rel(f[1], t[1]) <= 1e-5 and _rel(f[2], t[2]) <= 1e-5
    assert f[3] is None and t[3] is None


def test_fused_loss_deterministic(gpu):
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.003, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    logits, value, mine, batch = _outputs(32768, 256, gpu, torch.float16, seed=7)
    with torch.autocast("cuda", dtype=torch.float16):
        a = _run(True, logits, value, mine, batch, cfg, torch.float16)
        b = _run(True, logits, value, mine, batch, cfg, torch.float16)
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


def _torch_terms(logits, value, mine, b, cfg, world, counts):
    """ppo.py:33-87 in f64 from the same inputs (the data-parallel belief scale world / count)."""
    x = logits.double().masked_fill(~b.action_mask, -1e9)
    lp = torch.log_softmax(x, -1)
    r = (lp.gather(1, b.actions.view(-1, 1)).squeeze(1) - b.old_logp.double()).exp()
    A = b.advantages.double()
    pol = -torch.min(r * A, r.clamp(1 - cfg.clip_eps, 1 + cfg.clip_eps) * A).mean()
    v, V, R = value.double().view(-1), b.values.double(), b.returns.double()
    vc = V + (v - V).clamp(-cfg.clip_eps_v, cfg.clip_eps_v)
    val = 0.5 * torch.max((v - R) ** 2, (vc - R) ** 2).mean()
    ent = -(lp.exp() * lp).sum(-1).mean()
    lf, y = mine.double().reshape(b.mine_labels.shape), b.mine_labels.double()
    vm = torch.ones_like(y) if getattr(b, "mine_valid", None) is None else b.mine_valid.double()
    pos, cnt = counts[0].double(), counts[1].double()
    pw = (cnt - pos + 1e-6) / (pos + 1e-6)
    scale = world / cnt.clamp_min(1.0)
    bce = (torch.nn.functional.binary_cross_entropy_with_logits(lf, y, pos_weight=pw, reduction="none") * vm).sum() * scale
    cal = (((torch.sigmoid(lf) - y) ** 2) * vm).sum() * scale
    return [pol, val, ent, bce, cal]


@pytest.mark.parametrize("M,A,world,valid", [(1, 1, 1, False), (3, 5, 2, True), (517, 81, 4, False), (64, 512, 2, True)],
                         ids=["1x1", "3x5-world2", "517x81-world4-novalid", "64x512-world2"])
def test_fused_loss_edge_shapes_and_world(gpu, M, A, world, valid):
    """Odd shapes (one row, one action, the 512-cell maximum), no valid mask, and the data-parallel
    belief scale world / global count, against an f64 restatement: terms rel 1e-5."""
    from ms_amd.loss import ppo_loss_terms
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.003, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    logits, value, mine, b = _outputs(M, A, gpu, torch.float32, seed=M + A)
    if not valid:
        b.mine_valid = None
    vm = torch.ones_like(b.mine_labels) if b.mine_valid is None else b.mine_valid.float()
    counts = torch.stack([(b.mine_labels * vm).sum(), vm.sum()]) * 1.5  # a "global" count (other ranks)
    t = ppo_loss_terms(logits, value, mine, b, cfg, counts, world, None)
    ref = _torch_terms(logits, value, mine, b, cfg, world, counts)
    for k in range(5):
        assert float(t[k]) == pytest.approx(float(ref[k]), rel=1e-5, abs=1e-6), k
    w = [1.0, cfg.vf_coef, -cfg.ent_coef, cfg.aux_mine_weight, cfg.aux_mine_calib_weight]
    assert float(t[5]) == pytest.approx(sum(wk * float(rk) for wk, rk in zip(w, ref)), rel=1e-5, abs=1e-6)


# ---------------------------------------------------------------------------------------------
# The kernels against the f64 reference with gradients (tests/ppo_loss_ref.py), fp32 mode
# ---------------------------------------------------------------------------------------------
_CFG = dict(ent_coef=0.003, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)


def _fused(logits, value, mine, b, cfg, dev, counts=None, world=1, amp16=None):
    """ppo_loss_terms on device copies -> (f32 [8], (logits, value, mine) leaves)."""
    from ms_amd.loss import ppo_loss_terms
    bg = R.batch_to(b, dev)
    lg = logits.to(dev).requires_grad_(True)
    v = value.to(dev).requires_grad_(True)
    mi = mine.to(dev).requires_grad_(True) if mine is not None else None
    c = None
    if mi is not None:
        c = (R.local_counts(bg) if counts is None else counts.to(dev))
    return ppo_loss_terms(lg, v, mi, bg, cfg, c, world, amp16), (lg, v, mi)


def _grads(t, leaves, w):
    w8 = torch.zeros(8, device=t.device)
    w8[:6] = torch.as_tensor(w, dtype=torch.float32)
    ls = [x for x in leaves if x is not None]
    gs = list(torch.autograd.grad((w8[:6] * t[:6]).sum(), ls, retain_graph=True))
    return [gs.pop(0) if x is not None else None for x in leaves]


def _assert_terms(t, terms):
    got = t.detach().double().cpu()
    for k in range(6):
        assert float(got[k]) == pytest.approx(float(terms[k]), rel=1e-5, abs=1e-6), R.TERMS[k]


def _assert_grads(t, leaves, terms, rleaves, w, mask):
    got, want = _grads(t, leaves, w), R.ref_grads(terms, rleaves, w)
    for name, a, b in zip(("dlogits", "dvalue", "dmine"), got, want):
        if a is not None:
            assert R.rel_l2(a, b.reshape(a.shape)) <= 1e-5, (name, list(w))
    assert float(got[0][~mask.to(got[0].device)].abs().max()) == 0.0  # masked cells get no gradient
    return got


def _against_reference(gpu, logits, value, mine, b, cfg, ws, counts=None, world=1):
    t, leaves = _fused(logits, value, mine, b, cfg, gpu, counts, world)
    terms, rleaves = R.ref_terms(logits, value, mine, b, cfg, world, counts)
    _assert_terms(t, terms)
    assert float(t[6]) == 0.0 and float(t[7]) == 0.0
    return [_assert_grads(t, leaves, terms, rleaves, w, b.action_mask) for w in ws], t


def test_fused_loss_per_term_cotangents_vs_f64(gpu):
    """Backward of (w . out[:6]).sum() for a random w with six non-zero entries and for the six
    one-hot w, against the f64 autograd of the same combination (M = 37, A = 81)."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b = R.make_outputs(37, 81, torch.float32, seed=41)
    g = torch.Generator().manual_seed(1)
    w = (torch.rand(6, generator=g) + 0.25) * torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, 1.0])
    ws = [w.tolist()] + [[1.0 if i == k else 0.0 for i in range(6)] for k in range(6)]
    _against_reference(gpu, logits, value, mine, b, PPOConfig(**_CFG), ws)


@pytest.mark.parametrize("A,valid", [(5, True), (81, False)], ids=["A5-valid", "A81-novalid"])
def test_fused_loss_grid_stride_vs_f64(gpu, A, valid):
    """M = 2 * 8,192 + 7: every wave takes a third row and the row workspace is indexed past row
    8,191; the single-legal-cell row and the no-valid-cell row sit in the second pass."""
    from ms_amd.ppo import PPOConfig
    M = 2 * 8192 + 7
    logits, value, mine, b = R.make_outputs(M, A, torch.float32, seed=A, special=(8192 + 5, 12000))
    if not valid:
        b.mine_valid = None
    _against_reference(gpu, logits, value, mine, b, PPOConfig(**_CFG), [[0, 0, 0, 0, 0, 1.0]])


@pytest.mark.parametrize("A", [64, 65, 128, 129, 256, 257])
def test_fused_loss_template_boundaries_vs_f64(gpu, A):
    """Both sides of the NQ dispatch (A <= 128 / <= 256 / else) and of one / two lane rounds."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b = R.make_outputs(7, A, torch.float32, seed=100 + A)
    _against_reference(gpu, logits, value, mine, b, PPOConfig(**_CFG), [[0, 0, 0, 0, 0, 1.0]])


@pytest.mark.parametrize("clip_eps", [0.25, 0.0])
def test_fused_loss_directed_ties_and_edges(gpu, clip_eps):
    """ppo_loss_ref.tie_batch: bitwise ties of min / max, the clamps' closed edges, advantage 0,
    ratios clipped both ways for both advantage signs, an all-masked row and logits of range +-60."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b, kw = R.tie_batch(clip_eps)
    cfg = PPOConfig(ent_coef=0.01, aux_mine_weight=0.05, aux_mine_calib_weight=0.01, **kw)
    ws = [[0, 0, 0, 0, 0, 1.0], [1.0, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0]]
    got, t = _against_reference(gpu, logits, value, mine, b, cfg, ws)
    assert bool(torch.isfinite(t).all())
    M = logits.shape[0]
    want = torch.tensor([R.TIE_DV[i % 4] for i in range(M)], dtype=torch.float64) / M
    assert torch.allclose(got[2][1].double().cpu(), want, rtol=1e-6, atol=0)  # d value_loss / dv by hand
    for dl, _, _ in got:
        assert bool(torch.isfinite(dl).all())
        assert float(dl[0].abs().max()) == 0.0 and float(dl[6].abs().max()) == 0.0  # one legal cell; all masked
    assert float(got[1][0][1].abs().max()) == 0.0  # advantage 0: no policy gradient
    # row 8: ratio exactly 1 (on both closed edges when clip_eps = 0) keeps its whole gradient
    w8 = torch.zeros(8, dtype=torch.float64)
    w8[5], w8[2] = -0.5 / M, 0.5 / M
    assert torch.allclose(got[1][0][8].double().cpu(), w8, rtol=1e-6, atol=0)


def test_fused_loss_empty_valid_set(gpu):
    """mine_valid all False, counts (0, 0): both belief terms 0, dmine all 0, a finite loss."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b = R.make_outputs(9, 16, torch.float32, seed=8)
    b.mine_valid = torch.zeros_like(b.mine_valid)
    (got,), t = _against_reference(gpu, logits, value, mine, b, PPOConfig(**_CFG), [[0, 0, 0, 0, 0, 1.0]],
                                   counts=torch.zeros(2))
    assert float(t[3]) == 0.0 and float(t[4]) == 0.0 and bool(torch.isfinite(t[5]))
    assert float(got[2].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# 16-bit logits / value / mine logits under the matching autocast
# ---------------------------------------------------------------------------------------------
_SCALE = 1024.0
# Floors of the 2x bound below, for the six terms only: the PyTorch path's own absolute error
# against the f64 reference, the largest over the four (type, A) cases of
# test_fused_loss_16bit_vs_f64 as measured on an MI355X. Both paths compute the terms in f32 from
# the same rounded inputs, so a term's error is an f32 summation-order lottery (about one ulp) and
# the PyTorch path sometimes lands on the exact value. The gradient tensors need no floor.
_FLOOR16 = {"policy_loss": 5.086e-08, "value_loss": 2.023e-08, "entropy": 1.411e-07, "aux_bce": 1.433e-07,
            "aux_calib": 9.744e-06, "loss": 9.423e-08}


def _run16(gpu, fused, logits, value, mine, b, cfg, dt):
    bg = R.batch_to(b, gpu)
    with torch.autocast("cuda", dtype=dt):
        out, dl, dv, dm = _run(fused, logits.to(gpu), value.to(gpu), mine.to(gpu), bg, cfg, dt, scale=_SCALE)
    return out, dl, dv, dm


def _errors16(res, terms, rgrads):
    out, dl, dv, dm = res
    e = {k: abs(out[k] - float(terms[R.TERMS.index(k)])) for k in out}
    for name, a, g in zip(("dlogits", "dvalue", "dmine"), (dl, dv, dm), rgrads):
        e[name] = R.rel_l2(a, g.reshape(a.shape) * _SCALE)
    return e


def _bound16(gpu, logits, value, mine, b, cfg, dt, only=None):
    """Fused path and PyTorch path each against the f64 reference of the same rounded inputs
    (mask_fill -1e4): fused error <= 2 x max(PyTorch path's error, its measured floor)."""
    l16, v16, m16 = logits.to(dt), value.to(dt), mine.to(dt)
    terms, rleaves = R.ref_terms(l16.float(), v16.float(), m16.float(), b, cfg, mask_fill=-1e4, amp16=dt)
    rg = R.ref_grads(terms, rleaves, [0, 0, 0, 0, 0, 1.0])
    f = _run16(gpu, True, l16, v16, m16, b, cfg, dt)
    t = _run16(gpu, False, l16, v16, m16, b, cfg, dt)
    assert set(f[0]) == set(t[0])
    assert f[1].dtype == t[1].dtype == dt and f[2].dtype == dt and f[3].dtype == t[3].dtype == dt
    ef, et = _errors16(f, terms, rg), _errors16(t, terms, rg)
    print("16-bit errors vs f64 (fused, torch):", dt, logits.shape[1], {k: (ef[k], et[k]) for k in ef})
    for k in ef:
        if only is None or k in only:
            assert ef[k] <= 2.0 * max(et[k], _FLOOR16.get(k, 0.0)), (k, ef[k], et[k])
    return f, t


@pytest.mark.parametrize("A", [81, 256])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_fused_loss_16bit_vs_f64(gpu, A, dt):
    """Logits, value and mine logits given in fp16 / bf16 (M = 64): mask_fill -1e4 and the
    cast-back of dlogits. Errors against the f64 reference measured on an MI355X, fused / torch
    (gradients rel-L2 of the 1024-scaled loss; terms absolute):
      fp16 A=81   dlogits 1.72e-4 / 1.88e-4  dvalue 2.51e-4 / 2.51e-4  dmine 3.12e-4 / 3.12e-4
      fp16 A=256  dlogits 2.15e-4 / 2.23e-4  dvalue 2.03e-4 / 2.03e-4  dmine 2.72e-4 / 2.73e-4
      bf16 A=81   dlogits 1.64e-3 / 1.75e-3  dvalue 1.95e-3 / 1.95e-3  dmine 2.31e-3 / 2.30e-3
      bf16 A=256  dlogits 1.37e-3 / 1.47e-3  dvalue 1.76e-3 / 1.76e-3  dmine 2.22e-3 / 2.20e-3
      terms: both paths within 1.5e-7 (aux_calib, whose sigmoid is 16-bit: 1.1e-6 fp16, 9.7e-6
      bf16), equal to each other in most cases; the largest gap is aux_bce at fp16 A=256,
      2.61e-7 / 2.28e-8, which the floor of _FLOOR16 (1.43e-7, bf16 A=256) covers."""
    from ms_amd.ppo import PPOConfig
    logits, value, mine, b = R.make_outputs(64, A, torch.float32, seed=200 + A)
    _bound16(gpu, logits, value, mine, b, PPOConfig(**_CFG), dt)


# ---------------------------------------------------------------------------------------------
# The four defects of ADVICE.md (round 6)
# ---------------------------------------------------------------------------------------------
def test_fused_loss_fp16_calibration_only_with_no_positive_label(gpu):
    """aux_mine_weight = 0, aux_mine_calib_weight > 0, fp16, no positive label among the valid
    cells: pos_weight rounds to inf, and the BCE gradient must not be formed (0 * NaN)."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.003, aux_mine_weight=0.0, aux_mine_calib_weight=0.01)
    logits, value, mine, b = R.make_outputs(64, 81, torch.float32, seed=77)
    b.mine_labels = b.mine_labels * (~b.mine_valid).float()  # labels 0 on every valid cell
    f, t = _bound16(gpu, logits, value, mine, b, cfg, torch.float16, only=("dmine", "loss", "aux_calib"))
    assert "aux_bce" not in f[0] and np.isfinite(f[0]["loss"])
    assert bool(torch.isfinite(f[3]).all()) and bool(torch.isfinite(t[3]).all())


def test_fused_loss_fp16_bce_only(gpu):
    """The mirror: aux_mine_weight > 0, aux_mine_calib_weight = 0, with saturated mine logits (the
    fp16 sigmoid is exactly 0 / 1 there): the calibration half adds nothing non-finite."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(ent_coef=0.003, aux_mine_weight=0.05, aux_mine_calib_weight=0.0)
    logits, value, mine, b = R.make_outputs(64, 81, torch.float32, seed=78)
    mine[:, 0, ::7] = 60.0
    mine[:, 0, 3::7] = -60.0
    f, t = _bound16(gpu, logits, value, mine, b, cfg, torch.float16, only=("dmine", "loss", "aux_bce"))
    assert "aux_calib" not in f[0] and np.isfinite(f[0]["loss"])
    assert bool(torch.isfinite(f[3]).all())


@pytest.mark.parametrize("what", ["vpred", "logit"])
def test_fused_loss_propagates_nan_like_torch(gpu, what):
    """A NaN value prediction (value_loss, loss) or a NaN logit at the action (policy_loss,
    entropy, loss) shows as NaN exactly where torch.clamp / min / max put it."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(**_CFG)
    logits, value, mine, b = R.make_outputs(13, 81, torch.float32, seed=9)
    if what == "vpred":
        value[4] = float("nan")
        nan_keys = {"value_loss", "loss"}
    else:
        logits[4, b.actions[4]] = float("nan")
        nan_keys = {"policy_loss", "entropy", "loss"}
    bg = R.batch_to(b, gpu)
    f = _run(True, logits.to(gpu), value.to(gpu), mine.to(gpu), bg, cfg, None)
    t = _run(False, logits.to(gpu), value.to(gpu), mine.to(gpu), bg, cfg, None)
    assert {k for k, x in t[0].items() if np.isnan(x)} == nan_keys
    for k in t[0]:
        if k in nan_keys:
            assert np.isnan(f[0][k]), k
        else:
            assert f[0][k] == pytest.approx(t[0][k], rel=1e-5, abs=1e-6), k


@pytest.mark.parametrize("mdt", [torch.uint8, torch.float32], ids=["uint8", "float32"])
def test_fused_loss_accepts_non_bool_masks(gpu, mdt):
    """action_mask / mine_valid of another dtype: bitwise the outputs and gradients of the bool call."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(**_CFG)
    logits, value, mine, b = R.make_outputs(19, 81, torch.float32, seed=12)
    t0, l0 = _fused(logits, value, mine, b, cfg, gpu)
    g0 = _grads(t0, l0, [0, 0, 0, 0, 0, 1.0])
    b.action_mask, b.mine_valid = b.action_mask.to(mdt), b.mine_valid.to(mdt)
    t1, l1 = _fused(logits, value, mine, b, cfg, gpu)
    g1 = _grads(t1, l1, [0, 0, 0, 0, 0, 1.0])
    assert torch.equal(t0, t1)
    for x, y in zip(g0, g1):
        assert torch.equal(x, y)


def test_fused_loss_flags_out_of_range_actions(gpu):
    """Actions -1 and A in two rows of nine: out[6] counts them, policy_loss and loss are NaN, the
    rows' dlogits are NaN at their legal cells, and the other rows are untouched. Only the HIP
    path runs on this input (torch's gather would trip a device-side assert)."""
    from ms_amd.ppo import PPOConfig
    cfg = PPOConfig(**_CFG)
    A = 81
    logits, value, mine, b = R.make_outputs(9, A, torch.float32, seed=14)
    good = b.actions.clone()
    t0, l0 = _fused(logits, value, mine, b, cfg, gpu)
    g0 = _grads(t0, l0, [0, 0, 0, 0, 0, 1.0])
    assert float(t0[6]) == 0.0 and bool(torch.isfinite(t0).all())
    b.actions = good.clone()
    b.actions[2], b.actions[6] = -1, A
    t1, l1 = _fused(logits, value, mine, b, cfg, gpu)
    g1 = _grads(t1, l1, [0, 0, 0, 0, 0, 1.0])
    assert float(t1[6]) == 2.0
    assert bool(torch.isnan(t1[0])) and bool(torch.isnan(t1[5]))
    assert torch.equal(t1[1:5], t0[1:5])
    bad = torch.tensor([2, 6], device=gpu)
    ok = torch.tensor([0, 1, 3, 4, 5, 7, 8], device=gpu)
    m = b.action_mask.to(gpu)
    assert bool(torch.isnan(g1[0][bad][m[bad]]).all()) and float(g1[0][bad][~m[bad]].abs().max()) == 0.0
    assert torch.equal(g1[0][ok], g0[0][ok])
    assert torch.equal(g1[1], g0[1]) and torch.equal(g1[2], g0[2])


def test_ppo_loss_c_api_rejects_bad_arguments(gpu):
    from ms_amd import _lib as L
    from ms_amd.loss import _Args
    lib = L.load()
    f = lib.mc_ppo_loss_fwd
    out = torch.empty(8, device=gpu)
    work = torch.empty(1 << 16, device=gpu)
    a = _Args()  # every pointer NULL
    a.M, a.A = 4, 16
    assert f(ctypes.byref(a), out.data_ptr(), work.data_ptr(), work.numel(), None) == 1  # MS_EINVAL
    assert b"bad argument" in lib.mc_last_error()
    assert f(None, out.data_ptr(), work.data_ptr(), work.numel(), None) == 1
