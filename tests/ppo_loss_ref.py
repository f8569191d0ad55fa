"""An f64 restatement of the PPO minibatch loss (ms_amd/ppo.py ppo_losses, reference ppo.py:33-87)
with gradients, as plain torch ops on the CPU. It is what the HIP loss kernels (csrc/msppo.hip)
are compared with; tests/test_ppo_loss_ref.py pins it to ppo_losses' PyTorch branch on the CPU.

``ref_terms`` makes f64 leaf copies of logits / value / mine logits and returns the six outputs
(policy_loss, value_loss, entropy, aux_bce, aux_calib, loss) as differentiable f64 scalars, so
``ref_grads`` of any weighted sum of them gives reference gradients.

16-bit convention (``amp16``): the mine logits and pos_weight are rounded to that type before
the f64 math, the sigmoid stays exact, and casts have identity gradient. Logits and the value are
taken as given (pass them already rounded)."""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

TERMS = ("policy_loss", "value_loss", "entropy", "aux_bce", "aux_calib", "loss")


def make_outputs(M, A, vdt, seed, special=(0, 1)):
    """A random minibatch on the CPU: logits [M, A], value [M] (vdt), mine logits [M, 1, A] and
    the batch. Row special[0] has the action as its only legal cell, row special[1] (when M > 1)
    no valid cell; old log-probs sit near the current ones, so ratios fall on both sides of the
    clip range."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(M, A, generator=g) * 3
    mask = torch.rand(M, A, generator=g) < 0.7
    actions = torch.randint(0, A, (M,), generator=g)
    mask[torch.arange(M), actions] = True
    mask[special[0]] = False
    mask[special[0], actions[special[0]]] = True
    value = torch.randn(M, generator=g).to(vdt)
    mine = torch.randn(M, 1, A, generator=g) * 2
    labels = (torch.rand(M, A, generator=g) < 0.15).float()
    valid = torch.rand(M, A, generator=g) < 0.6
    if M > 1:
        valid[special[1]] = False
    lp = torch.log_softmax(logits.masked_fill(~mask, -1e9), -1)[torch.arange(M), actions]
    old = lp + torch.randn(M, generator=g) * 0.3
    batch = SimpleNamespace(obs=torch.zeros(M, 1), action_mask=mask, actions=actions, old_logp=old,
                            advantages=torch.randn(M, generator=g),
                            values=value.float() + torch.randn(M, generator=g) * 0.3,
                            returns=value.float() + torch.randn(M, generator=g),
                            mine_labels=labels, mine_valid=valid)
    return logits, value, mine, batch


def batch_to(b, dev):
    return SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(b).items()})


def local_counts(b):
    """(sum labels * valid, sum valid) of this batch, f32 [2], as ppo_losses forms it."""
    y = b.mine_labels
    vmask = getattr(b, "mine_valid", None)
    vm = torch.ones_like(y) if vmask is None else vmask.to(y.dtype)
    return torch.stack([(y * vm).sum(), vm.sum()])


def ref_terms(logits, value, mine, b, cfg, world=1, counts=None, mask_fill=-1e9, amp16=None):
    """-> (six f64 scalars in TERMS order, (logits, value, mine) f64 leaves; mine None without
    belief logits). ``counts`` = global (sum labels * valid, sum valid); None: this batch's."""
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    lg = cpu(logits).double().requires_grad_(True)
    v = cpu(value).double().reshape(-1).requires_grad_(True)
    amask = cpu(b.action_mask).ne(0)
    x = lg.masked_fill(~amask, mask_fill)
    lp = torch.log_softmax(x, -1)
    lpa = lp.gather(1, cpu(b.actions).long().view(-1, 1)).squeeze(1)
    r = (lpa - cpu(b.old_logp).double()).exp()
    adv = cpu(b.advantages).double()
    pol = -torch.min(r * adv, r.clamp(1 - cfg.clip_eps, 1 + cfg.clip_eps) * adv).mean()
    V, R = cpu(b.values).double(), cpu(b.returns).double()
    vc = V + (v - V).clamp(-cfg.clip_eps_v, cfg.clip_eps_v)
    val = 0.5 * torch.max((v - R) ** 2, (vc - R) ** 2).mean()
    ent = -(lp.exp() * lp).sum(-1).mean()
    loss = pol + cfg.vf_coef * val - cfg.ent_coef * ent
    zero = torch.zeros((), dtype=torch.float64)
    bce = cal = zero
    mi = None
    if mine is not None:
        mi = cpu(mine).double().requires_grad_(True)
        y = cpu(b.mine_labels).double()
        lf = mi.reshape(y.shape)
        if amp16 is not None:  # the cast's value with an identity gradient
            lf = lf + (lf.detach().float().to(amp16).double() - lf.detach())
        vmask = getattr(b, "mine_valid", None)
        vm = torch.ones_like(y) if vmask is None else cpu(vmask).ne(0).double()
        c = cpu(local_counts(b) if counts is None else counts).float()
        pos, cnt = c[0], c[1]
        pw = (cnt - pos + 1e-6) / (pos + 1e-6)  # f32, as both implementations form it
        pw = (pw.to(amp16) if amp16 is not None else pw).double()
        scale = world / cnt.double().clamp_min(1.0)
        bce = (F.binary_cross_entropy_with_logits(lf, y, pos_weight=pw, reduction="none") * vm).sum() * scale
        cal = (((torch.sigmoid(lf) - y) ** 2) * vm).sum() * scale
        if cfg.aux_mine_weight > 0:
            loss = loss + cfg.aux_mine_weight * bce
        if cfg.aux_mine_calib_weight > 0:
            loss = loss + cfg.aux_mine_calib_weight * cal
    return [pol, val, ent, bce, cal, loss], (lg, v, mi)


def ref_grads(terms, leaves, w):
    """Gradients of sum_k w[k] terms[k] w.r.t. the leaves (zeros where nothing depends on one)."""
    total = sum(float(wk) * t for wk, t in zip(w, terms) if float(wk) != 0.0 and t.requires_grad)
    ls = [x for x in leaves if x is not None]
    gs = iter(torch.autograd.grad(total, ls, allow_unused=True, retain_graph=True))
    out = []
    for x in leaves:
        if x is None:
            out.append(None)
        else:
            g = next(gs)
            out.append(torch.zeros_like(x) if g is None else g)
    return out


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# The directed batch of ties and edges (A = 8, clip_eps = clip_eps_v = 0.25), every deciding
# value exactly representable so that the ties are bitwise whatever expf / logf return.
def tie_batch(clip_eps=0.25):
    """-> logits [M, 8], value [M], mine [M, 1, 8], batch, cfg-kwargs. Rows:
      0  one legal cell = the action, old_logp 0: log pi(a) = 0 and ratio = 1 exactly (inside the
         clip range, and on both closed edges at once when clip_eps = 0)
      1  advantage 0, ratio far above the range
      2, 3  ratio clipped high, advantage + / -      4, 5  ratio clipped low, advantage + / -
      6  every cell masked (the action's too): log pi = -log 8 over the fill value, dlogits 0
      7  logits spread over +-60: the softmax underflows to exact zeros
      8  two legal cells, logits 0 and -200 = the action, old_logp -200: the log-sum is log(1) = 0,
         so log pi(a) = -200 and ratio = 1 exactly as in row 0, but with p(a) = 0 the gradient
         is -(adv / M)(delta_ja - p_j) != 0: a tie rule that treated the closed edge as clipped
         (clip_eps = 0) would lose it
    Value rows (vp, V, R) cycle through (1.5, 1, 1.375) clipped with v1 == v2, (1.25, 1, 2) on the
    clamp's closed edge, (1, 1, 0.5) and (1.1, 1, 3) inside: per row d(0.5 max(v1, v2)) / dv =
    0.0625 (half of d1), -0.75, 0.5, -1.9, before the 1 / M of the mean (TIE_DV)."""
    A, M = 8, 9
    g = torch.Generator(device="cpu").manual_seed(11)
    logits = torch.randn(M, A, generator=g)
    mask = torch.ones(M, A, dtype=torch.bool)
    actions = torch.tensor([3, 1, 2, 5, 0, 7, 4, 6, 5])
    mask[0] = False
    mask[0, 3] = True
    mask[1, 4] = mask[2, 0] = mask[4, 6] = False  # ordinary rows carry masked cells too
    mask[6] = False
    mask[8] = False
    mask[8, 2] = mask[8, 5] = True
    logits[8, 2], logits[8, 5] = 0.0, -200.0
    logits[7] = torch.tensor([60.0, -60.0, 59.0, -59.5, 0.0, 30.0, -30.0, 58.0])
    lp = torch.log_softmax(logits.double().masked_fill(~mask, -1e9), -1)[torch.arange(M), actions].float()
    old = lp.clone()
    old[0] = 0.0
    old[1] = lp[1] - 3.0                      # ratio ~ 20
    old[2], old[3] = lp[2] - 1.0, lp[3] - 1.0  # ratio ~ 2.7
    old[4], old[5] = lp[4] + 1.0, lp[5] + 1.0  # ratio ~ 0.37
    old[7] = lp[7] + 0.1                       # inside the range
    old[8] = -200.0
    adv = torch.tensor([1.5, 0.0, 2.0, -2.0, 0.75, -0.75, 1.0, -1.25, 0.5])
    vrows = [(1.5, 1.0, 1.375), (1.25, 1.0, 2.0), (1.0, 1.0, 0.5), (1.1, 1.0, 3.0)]
    vp, V, R = (torch.tensor([vrows[i % 4][k] for i in range(M)], dtype=torch.float32) for k in range(3))
    mine = torch.randn(M, 1, A, generator=g) * 2
    labels = (torch.rand(M, A, generator=g) < 0.3).float()
    valid = torch.rand(M, A, generator=g) < 0.6
    batch = SimpleNamespace(obs=torch.zeros(M, 1), action_mask=mask, actions=actions, old_logp=old,
                            advantages=adv, values=V, returns=R, mine_labels=labels, mine_valid=valid)
    return logits, vp, mine, batch, dict(clip_eps=clip_eps, clip_eps_v=0.25)


# per-row d(0.5 max(v1, v2)) / d vpred of tie_batch's four value rows
TIE_DV = (0.0625, -0.75, 0.5, -1.9)
