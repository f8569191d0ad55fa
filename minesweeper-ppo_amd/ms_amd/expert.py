"""Expert policy targets from an exact posterior result (include/msexpert.h).

``expert_targets`` (device tensors, one HIP launch, one wavefront per board) and
``expert_targets_host`` (numpy, the plain C++ twin; bitwise the same results) take the ``status``
and ``prob`` of any ``posterior_states`` / ``posterior_host`` / ``VecMinesweeper.mine_posterior``
call and a hidden-cell mask (the env's action mask), and return a dict:

  ``best`` u8 [n, A]      1 at the hidden cells of least mine probability (f64 ties all count);
  ``action`` i64 [n]      the lowest cell index in ``best`` (``PosteriorModel``'s greedy pick), or -1;
  ``kind`` u8 [n]         0 no target (board not decided, or nothing hidden), 1 a provably safe
                          move exists (p = 0), 2 forced guess (``best`` = the least dangerous cells);
  ``n_best`` i32 [n]      ``best.sum(1)``;
  ``labels`` f32 [n, A]   the mine probability at hidden cells rounded to f32, 0 elsewhere.

A board that is not decided is never a guess: it carries no target.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib as L

KIND_NONE, KIND_SAFE, KIND_GUESS = L.MS_EXPERT_NONE, L.MS_EXPERT_SAFE, L.MS_EXPERT_GUESS


def _check_A(A: int) -> None:
    if not 1 <= A <= L.MS_AVOID_MAX_CELLS:
        raise ValueError(f"expert targets need 1 <= cells <= {L.MS_AVOID_MAX_CELLS}, got {A}")


def expert_targets_host(post: Dict[str, np.ndarray], hidden) -> Dict[str, np.ndarray]:
    """ms_expert_targets_host on numpy arrays: ``post`` holds ``status`` [n] and ``prob`` [n, A],
    ``hidden`` [n, A] (or [n, H, W]) is non-zero at hidden cells."""
    status = np.ascontiguousarray(post["status"], dtype=np.uint8).reshape(-1)
    n = status.shape[0]
    prob = np.ascontiguousarray(post["prob"], dtype=np.float64).reshape(n, -1)
    A = prob.shape[1]
    _check_A(A)
    hid = np.ascontiguousarray(np.asarray(hidden).reshape(n, -1) != 0).view(np.uint8)
    if hid.shape != (n, A):
        raise ValueError(f"hidden: expected {n * A} cells, got shape {np.asarray(hidden).shape}")
    out = {k: np.zeros((n, A) if cells else (n,), dtype=dt) for k, dt, cells in L.EXPERT_OUTPUTS}
    L.check(L.load().ms_expert_targets_host(status.ctypes.data, prob.ctypes.data, hid.ctypes.data, n, A,
                                            *(out[k].ctypes.data for k, _, _ in L.EXPERT_OUTPUTS)))
    return out


def expert_targets(post: Dict[str, torch.Tensor], hidden: torch.Tensor) -> Dict[str, torch.Tensor]:
    """ms_expert_targets on device tensors: ``post`` holds ``status`` u8 [n] and ``prob`` f64 [n, A],
    ``hidden`` [n, A] (or [n, H, W]; bool or any integer type) is non-zero at hidden cells. One
    launch on the current stream, no host sync."""
    status, prob = post["status"], post["prob"]
    if prob.device.type != "cuda":
        raise ValueError("expert_targets: expected tensors on a HIP device (expert_targets_host takes numpy)")
    dev = prob.device
    n = status.numel()
    if status.dtype != torch.uint8 or prob.dtype != torch.float64:
        raise ValueError("expert_targets: status must be uint8 and prob float64 (a posterior result)")
    status = status.reshape(n).contiguous()
    prob = prob.reshape(n, -1).contiguous()
    A = prob.shape[1]
    _check_A(A)
    hid = torch.as_tensor(hidden, device=dev).reshape(n, -1)
    if tuple(hid.shape) != (n, A):
        raise ValueError(f"hidden: expected {n * A} cells, got shape {tuple(hidden.shape)}")
    hid = (hid if hid.dtype == torch.bool else hid.ne(0)).contiguous()
    out = {k: torch.empty((n, A) if cells else (n,), dtype=getattr(torch, dt), device=dev)
           for k, dt, cells in L.EXPERT_OUTPUTS}
    with torch.cuda.device(dev):
        L.check(L.load().ms_expert_targets(L.ptr(status), L.ptr(prob), L.ptr(hid), n, A,
                                           *(L.ptr(out[k]) for k, _, _ in L.EXPERT_OUTPUTS), L.stream_ptr(dev)))
    return out


__all__ = ["expert_targets", "expert_targets_host", "KIND_NONE", "KIND_SAFE", "KIND_GUESS"]
