"""Avoidability analysis (include/mssolve.h): was a provably safe cell on offer?

Reference: minesweeper/avoidability.py ``analyze_avoidability`` (eval.py:381-398 calls it in
Python once per env and step). Here it is one HIP kernel launch over all boards
(``avoid_states`` / ``VecMinesweeper.avoidability``) and a plain C++ solver on the host
(``avoid_host``): the exact fallback for the boards the bounded device search reports
undecided, and the only path that needs no device.

Every function returns the ten per-env outputs of mssolve.h as a dict: ``status`` (0 not
analysed, 1 decided, 2 undecided), ``avoidable``, ``n_safe``, ``chosen_safe``,
``chosen_comp`` (0 = the reference's None), ``n_comp``, ``n_frontier``, ``safe_mask`` [n, H*W],
``max_nodes`` and ``comp_size`` [n, H*W].
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L


def _np_u8(a, shape, name):
    a = np.asarray(a)
    if a.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
    return np.ascontiguousarray(a if a.dtype == np.uint8 else a != 0, dtype=np.uint8)


def avoid_host(revealed, mine, chosen, first_click=None, live=None) -> Dict[str, np.ndarray]:
    """ms_avoid_host on numpy arrays: revealed / mine [n, H, W] (bool or u8), chosen [n]."""
    revealed = np.asarray(revealed)
    if revealed.ndim != 3:
        raise ValueError(f"revealed: expected [n, H, W], got shape {revealed.shape}")
    n, H, W = revealed.shape
    rev = _np_u8(revealed, (n, H, W), "revealed")
    mn = _np_u8(mine, (n, H, W), "mine")
    ch = np.ascontiguousarray(chosen, dtype=np.int64)
    if ch.shape != (n,):
        raise ValueError(f"chosen: expected shape {(n,)}, got {ch.shape}")
    fc = None if first_click is None else _np_u8(first_click, (n,), "first_click")
    lv = None if live is None else _np_u8(live, (n,), "live")
    out = {k: np.zeros((n, H * W) if cells else (n,), dtype=dt) for k, dt, cells in L.AVOID_OUTPUTS}
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    L.check(L.load().ms_avoid_host(p(rev), p(mn), p(fc), p(ch), p(lv), n, H, W,
                                   *(p(out[k]) for k, _, _ in L.AVOID_OUTPUTS)))
    return out


def _alloc(n: int, A: int, device) -> Dict[str, torch.Tensor]:
    return {k: torch.empty((n, A) if cells else (n,), dtype=getattr(torch, dt), device=device)
            for k, dt, cells in L.AVOID_OUTPUTS}


def _dev_u8(t: Optional[torch.Tensor], shape, name, device):
    if t is None:
        return None
    t = torch.as_tensor(t, device=device)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    return (t != 0).to(torch.uint8).contiguous() if t.dtype != torch.uint8 else t.contiguous()


def avoid_states(revealed: torch.Tensor, mine: torch.Tensor, chosen: torch.Tensor,
                 first_click: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None,
                 budget: int = L.MS_AVOID_DEFAULT_BUDGET) -> Dict[str, torch.Tensor]:
    """ms_avoid_states on device tensors: revealed / mine [n, H, W] (bool or u8), chosen i64 [n].
    No host fallback: a board may come back with status 2."""
    if revealed.dim() != 3 or revealed.device.type != "cuda":
        raise ValueError("revealed: expected a [n, H, W] tensor on a HIP device")
    dev = revealed.device
    n, H, W = revealed.shape
    rev = _dev_u8(revealed, (n, H, W), "revealed", dev)
    mn = _dev_u8(mine, (n, H, W), "mine", dev)
    ch = torch.as_tensor(chosen, device=dev).to(torch.int64).contiguous()
    if tuple(ch.shape) != (n,):
        raise ValueError(f"chosen: expected shape {(n,)}, got {tuple(ch.shape)}")
    fc = _dev_u8(first_click, (n,), "first_click", dev)
    lv = _dev_u8(live, (n,), "live", dev)
    out = _alloc(n, H * W, dev)
    with torch.cuda.device(dev):
        L.check(L.load().ms_avoid_states(L.ptr(rev), L.ptr(mn), L.ptr(fc), L.ptr(ch), L.ptr(lv), n, H, W, int(budget),
                                         *(L.ptr(out[k]) for k, _, _ in L.AVOID_OUTPUTS), L.stream_ptr(dev)))
    return out


__all__ = ["avoid_host", "avoid_states"]
