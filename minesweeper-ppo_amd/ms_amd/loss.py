"""The PPO minibatch loss on the GPU in two HIP passes (csrc/msppo.hip, C ABI include/msppo.h).

``ppo_loss_terms`` returns the reference's loss terms (minesweeper/ppo.py:33-87: policy, value,
entropy, belief BCE, calibration, and their weighted sum) as one f32 [8] tensor whose autograd
backward is the second pass: dlogits, dvalue and dmine in one launch instead of PyTorch's ~40
element-wise and reduction kernels each way. ms_amd/ppo.py ``ppo_losses`` takes this path on
CUDA (``FUSED_LOSS``; ``MS_FUSED_LOSS=0`` keeps the PyTorch ops, for A/B runs and parity tests).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _lib as L

FUSED_LOSS = os.environ.get("MS_FUSED_LOSS", "1") != "0"
MP_F32 = -1
_DT = {torch.float32: MP_F32, torch.bfloat16: L.MC_DTYPE_BF16, torch.float16: L.MC_DTYPE_F16}
OUT_KEYS = ("policy_loss", "value_loss", "entropy", "aux_bce", "aux_calib", "loss")
_Args = L.McPpoLossArgs  # mc_ppo_loss_args (include/msppo.h)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else L.ptr(t)


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, vpred, mine, keep, args):
        # keep: the non-differentiable row tensors the args point at (alive until backward)
        dev = logits.device
        lib = L.load()
        out = torch.empty(8, dtype=torch.float32, device=dev)
        nws = int(lib.mc_ppo_loss_workspace(args.M))
        work = torch.empty(nws, dtype=torch.float32, device=dev)
        L.check_mc(lib.mc_ppo_loss_fwd(ctypes.byref(args), L.ptr(out), L.ptr(work), nws, L.stream_ptr(dev)))
        ctx.save_for_backward(logits, vpred, mine, work)
        ctx.keep, ctx.args = keep, args
        return out

    @staticmethod
    def backward(ctx, gout):
        logits, vpred, mine, work = ctx.saved_tensors
        gout = gout.float().contiguous()
        dl = torch.empty_like(logits)
        dv = torch.empty_like(vpred)
        dm = torch.empty_like(mine) if mine is not None else None
        L.check_mc(L.load().mc_ppo_loss_bwd(ctypes.byref(ctx.args), L.ptr(gout), L.ptr(work), work.numel(), L.ptr(dl),
                                            L.ptr(dv), _p(dm), L.stream_ptr(logits.device)))
        return dl, dv, dm, None, None


def ppo_loss_terms(logits, value, mine_logits, batch, cfg, counts: Optional[torch.Tensor], world: int,
                   amp16: Optional[torch.dtype]) -> torch.Tensor:
    """f32 [8] = (policy_loss, value_loss, entropy, aux_bce, aux_calib, loss, bad_actions, 0) as
    ms_amd/ppo.py ppo_losses computes them (ppo.py:33-87); bad_actions counts the rows whose action
    is outside [0, A) (their log pi(a), hence policy_loss and loss, are NaN; 0 on clean input).
    ``action_mask`` / ``mine_valid`` may have any dtype (non-zero = set). ``mine_logits`` None: no belief terms;
    otherwise ``counts`` = global (sum labels * valid, sum valid). ``batch.mine_labels`` are targets
    in [0, 1]: 0 / 1 mine labels or posterior probabilities (``VecMinesweeper.posterior_labels``);
    counts[0] is then the expected positive count, and pos_weight is formed from it. ``amp16``:
    the 16-bit autocast type the reference rounds the belief logits to, or None."""
    n = logits.shape[0]
    A = logits.shape[-1]
    mask_fill = -1e4 if logits.dtype in (torch.float16, torch.bfloat16) else -1e9
    lg = logits.float().contiguous()
    vp = value.reshape(-1)
    if vp.dtype not in _DT:
        vp = vp.float()
    vp = vp.contiguous()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    # masks of any dtype, as the PyTorch ops take them (vmask.to(y.dtype)): non-zero = set
    as_bool = lambda t: (t if t.dtype == torch.bool else t.ne(0)).contiguous()  # noqa: E731
    keep = [as_bool(batch.action_mask), batch.actions.to(torch.int64).contiguous(), f32(batch.old_logp),
            f32(batch.advantages), f32(batch.values), f32(batch.returns)]
    mine = None
    if mine_logits is not None:
        mine = mine_logits.reshape(n, -1).float().contiguous()
        vmask = getattr(batch, "mine_valid", None)
        keep += [f32(batch.mine_labels.reshape(n, -1)),
                 as_bool(vmask.reshape(n, -1)) if vmask is not None else None, counts.float().contiguous()]
    else:
        keep += [None, None, None]
    a = _Args()
    (a.action_mask, a.actions, a.old_logp, a.advantages, a.values, a.returns, a.labels, a.valid, a.counts) = \
        [_p(t) for t in keep]
    a.logits, a.vpred, a.mine = L.ptr(lg), L.ptr(vp), _p(mine)
    a.vpred_dtype = _DT[vp.dtype]
    a.mine_round = _DT[amp16] if amp16 is not None else MP_F32
    a.clip_eps, a.clip_eps_v, a.vf_coef, a.ent_coef = cfg.clip_eps, cfg.clip_eps_v, cfg.vf_coef, cfg.ent_coef
    a.aux_mine_weight, a.aux_mine_calib_weight = cfg.aux_mine_weight, cfg.aux_mine_calib_weight
    a.mask_fill, a.world, a.M, a.A = mask_fill, float(world), n, A
    return _LossFn.apply(lg, vp, mine, keep, a)


__all__ = ["FUSED_LOSS", "OUT_KEYS", "ppo_loss_terms"]
