"""The behaviour-cloning minibatch loss on the GPU in two HIP passes (csrc/msbc.hip, C ABI
include/msbc.h), in the shape of ms_amd/loss.py.

``bc_loss_terms`` returns one f32 [8] tensor (``OUT_KEYS`` names its first seven entries): the
cross entropy of the masked policy against the expert's set of equally good cells, the weighted
agreement of the greedy pick with that set, the policy entropy, the two belief terms of the PPO
loss restricted to ``valid``, their weighted sum and the count of malformed rows. Its autograd
backward is the second pass (dlogits and dmine in one launch). There is no PyTorch-op path.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib as L

OUT_KEYS = ("policy_ce", "agree", "entropy", "aux_bce", "aux_calib", "loss", "bad_rows")
_Args = L.McBcLossArgs  # mc_bc_loss_args (include/msbc.h)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else L.ptr(t)


class _BcLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, mine, keep, args):
        # keep: the non-differentiable tensors the args point at (alive until backward)
        dev = logits.device
        lib = L.load()
        out = torch.empty(8, dtype=torch.float32, device=dev)
        nws = int(lib.mc_bc_loss_workspace(args.M))
        work = torch.empty(nws, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check_mc(lib.mc_bc_loss_fwd(ctypes.byref(args), L.ptr(out), L.ptr(work), nws, L.stream_ptr(dev)))
        ctx.save_for_backward(logits, mine, work)
        ctx.keep, ctx.args = keep, args
        return out

    @staticmethod
    def backward(ctx, gout):
        logits, mine, work = ctx.saved_tensors
        gout = gout.float().contiguous()
        dl = torch.empty_like(logits)
        dm = torch.empty_like(mine) if mine is not None else None
        with torch.cuda.device(logits.device):
            L.check_mc(L.load().mc_bc_loss_bwd(ctypes.byref(ctx.args), L.ptr(gout), L.ptr(work), work.numel(),
                                               L.ptr(dl), _p(dm), L.stream_ptr(logits.device)))
        return dl, dm, None, None


def bc_loss_terms(logits: torch.Tensor, mine_logits: Optional[torch.Tensor], action_mask: torch.Tensor,
                  best: torch.Tensor, weight: torch.Tensor, *, labels: Optional[torch.Tensor] = None,
                  valid: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                  ent_coef: float = 0.0, aux_mine_weight: float = 0.0, aux_mine_calib_weight: float = 0.0,
                  world: int = 1) -> torch.Tensor:
    """f32 [8] = (policy_ce, agree, entropy, aux_bce, aux_calib, loss, bad_rows, 0) of include/msbc.h.
    ``logits`` [M, A] (any float type; read as f32, masked cells filled with -1e4 when 16-bit, else
    -1e9, as the PPO loss does); ``action_mask`` / ``best`` / ``valid`` [M, A] of any dtype
    (non-zero = set); ``weight`` [M] >= 0, 0 excludes the row. ``mine_logits`` None: no belief
    terms; otherwise ``labels`` [M, A] in [0, 1] are needed. ``counts`` f32 [3] = the GLOBAL
    minibatch's (sum weight, sum labels * valid, sum valid); None: formed from this call's tensors."""
    if logits.dim() != 2 or logits.device.type != "cuda":
        raise ValueError("bc_loss_terms: logits must be a [M, A] tensor on a HIP device")
    n, A = logits.shape
    mask_fill = -1e4 if logits.dtype in (torch.float16, torch.bfloat16) else -1e9
    lg = logits.float().contiguous()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    as_bool = lambda t: (t if t.dtype == torch.bool else t.ne(0)).reshape(n, -1).contiguous()  # noqa: E731
    w = f32(weight.reshape(-1))
    mine = y = vm = None
    if mine_logits is not None:
        if labels is None:
            raise ValueError("bc_loss_terms: mine_logits need labels")
        mine = mine_logits.reshape(n, -1).float().contiguous()
        y = f32(labels.reshape(n, -1))
        vm = as_bool(valid) if valid is not None else None
    if counts is None:
        zero = w.new_zeros(())
        if mine is not None:
            v = torch.ones_like(y) if vm is None else vm.to(y.dtype)
            counts = torch.stack([w.sum(), (y * v).sum(), v.sum()])
        else:
            counts = torch.stack([w.sum(), zero, zero])
    keep = [as_bool(action_mask), as_bool(best), w, y, vm, f32(counts)]
    a = _Args()
    a.action_mask, a.best, a.weight, a.labels, a.valid, a.counts = [_p(t) for t in keep]
    a.logits, a.mine = L.ptr(lg), _p(mine)
    a.mask_fill, a.ent_coef = mask_fill, float(ent_coef)
    a.aux_mine_weight, a.aux_mine_calib_weight = float(aux_mine_weight), float(aux_mine_calib_weight)
    a.world, a.M, a.A = float(world), n, A
    return _BcLossFn.apply(lg, mine, keep, a)


__all__ = ["OUT_KEYS", "bc_loss_terms"]
