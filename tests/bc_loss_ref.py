"""An f64 restatement of the behaviour-cloning minibatch loss of include/msbc.h with gradients, as
plain torch ops on the CPU: what the HIP passes (csrc/msbc.hip via ms_amd/bc_loss.py) are
compared with. Written from the header's formulas, not from the kernel.

``ref_terms`` makes f64 leaf copies of the logits and the belief logits and returns the seven
outputs (policy_ce, agree, entropy, aux_bce, aux_calib, loss, bad_rows) as f64 scalars;
``ppo_loss_ref.ref_grads`` of any weighted sum of them gives reference gradients."""
from __future__ import annotations

import torch
import torch.nn.functional as F

TERMS = ("policy_ce", "agree", "entropy", "aux_bce", "aux_calib", "loss", "bad_rows")


def make_batch(M, A, seed, w_zero_rows=(1,)):
    """A random minibatch on the CPU: logits [M, A], mine logits [M, 1, A], mask, best (a random
    non-empty subset of the legal cells), weight in {1, 0.5} with the ``w_zero_rows`` at 0, labels
    in [0, 1], valid. Row 0 has one legal cell."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(M, A, generator=g) * 3
    mask = torch.rand(M, A, generator=g) < 0.7
    first = torch.randint(0, A, (M,), generator=g)
    mask[torch.arange(M), first] = True
    mask[0] = False
    mask[0, first[0]] = True
    best = (torch.rand(M, A, generator=g) < 0.1) & mask
    best[torch.arange(M), first] = True
    weight = torch.where(torch.rand(M, generator=g) < 0.5, 1.0, 0.5)
    for r in w_zero_rows:
        if r < M:
            weight[r] = 0.0
    mine = torch.randn(M, 1, A, generator=g) * 2
    labels = torch.rand(M, A, generator=g) * (torch.rand(M, A, generator=g) < 0.5)
    valid = mask & (torch.rand(M, A, generator=g) < 0.8)
    return dict(logits=logits, mine=mine, mask=mask, best=best.to(torch.uint8), weight=weight, labels=labels,
                valid=valid)


def local_counts(b, with_mine=True):
    """f32 [3] = (sum weight, sum labels * valid, sum valid) of this batch."""
    w = b["weight"].float()
    if not with_mine:
        return torch.stack([w.sum(), w.new_zeros(()), w.new_zeros(())])
    y = b["labels"].float()
    vm = torch.ones_like(y) if b.get("valid") is None else b["valid"].ne(0).to(y.dtype)
    return torch.stack([w.sum(), (y * vm).sum(), vm.sum()])


def ref_terms(b, *, ent_coef=0.0, aux_mine_weight=0.0, aux_mine_calib_weight=0.0, world=1, counts=None,
              mask_fill=-1e9, with_mine=True):
    """-> (seven f64 scalars in TERMS order, (logits, mine) f64 leaves; mine None without belief
    logits). ``counts`` f32 [3] as the kernel takes it; None: this batch's."""
    cpu = lambda t: t.detach().cpu()  # noqa: E731
    lg = cpu(b["logits"]).double().requires_grad_(True)
    M, A = lg.shape
    amask = cpu(b["mask"]).ne(0)
    best = cpu(b["best"]).ne(0)
    w = cpu(b["weight"]).double()
    c = cpu(local_counts(b, with_mine) if counts is None else counts).float()
    x = lg.masked_fill(~amask, mask_fill)
    lp = torch.log_softmax(x, -1)
    nb = best.sum(1)
    bad = (w != 0) & ((nb == 0) | (best & ~amask).any(1))
    ce_row = -(lp * best).sum(1) / nb.double()  # 0 / 0 = NaN on an empty best
    ce_row = torch.where(bad, torch.full_like(ce_row, float("nan")), ce_row)
    ent_row = -(lp.exp() * lp).sum(1)
    idx = torch.arange(A).expand(M, A)
    mx = x.detach().max(1, keepdim=True).values
    am = torch.where(x.detach() == mx, idx, torch.full_like(idx, A)).min(1).values  # the lowest argmax
    agree_row = best[torch.arange(M), am].double()
    on = w != 0  # a row of weight 0 is excluded, whatever it holds
    zero = torch.zeros((), dtype=torch.float64)
    c0 = c[0].double()
    if float(c0) > 0:
        norm = world / c0
        ce = torch.where(on, w * ce_row, torch.zeros_like(ce_row)).sum() * norm
        agree = torch.where(on, w * agree_row, torch.zeros_like(agree_row)).sum() * norm
        ent = torch.where(on, w * ent_row, torch.zeros_like(ent_row)).sum() * norm
    else:
        ce, agree, ent = zero * lg.sum(), zero, zero * lg.sum()
    loss = ce - ent_coef * ent
    bce = cal = zero
    mi = None
    if with_mine:
        mi = cpu(b["mine"]).double().requires_grad_(True)
        y = cpu(b["labels"]).double()
        lf = mi.reshape(y.shape)
        vm = torch.ones_like(y) if b.get("valid") is None else cpu(b["valid"]).ne(0).double()
        pos, cnt = c[1], c[2]
        pw = ((cnt - pos + 1e-6) / (pos + 1e-6)).double()  # f32, as the kernel forms it
        scale = world / cnt.double().clamp_min(1.0)
        bce = (F.binary_cross_entropy_with_logits(lf, y, pos_weight=pw, reduction="none") * vm).sum() * scale
        cal = (((torch.sigmoid(lf) - y) ** 2) * vm).sum() * scale
        if aux_mine_weight > 0:
            loss = loss + aux_mine_weight * bce
        if aux_mine_calib_weight > 0:
            loss = loss + aux_mine_calib_weight * cal
    return [ce, agree.detach(), ent, bce, cal, loss, bad.double().sum()], (lg, mi)
