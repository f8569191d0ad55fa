"""Board symmetries (include/mssym.h): a Minesweeper position and its mirror
images and rotations are the same problem, so a labelled state gives G labelled states and a
policy can be averaged over the group.

A group element ``g`` has three bits, applied in this order to an [H, W] plane ``X``:
``X = X.T if g & 4; X = X[::-1] if g & 1; X = X[:, ::-1] if g & 2``. The transpose needs a square
board: ``group_size(H, W)`` is 8 where H == W and 4 otherwise.

  ``cell_map(H, W, g)``   i32 [A] with ``T_g(X).flat[i] == X.flat[map[i]]`` (host, numpy)
  ``sym_gather(...)``     rows of the planes of an ``ExpertBuffer``, gathered and transformed in one launch
  ``sym_expand(codes)``   u8 [n, H, W] -> u8 [G, n, H, W], ``out[g] = T_g(codes)``
  ``sym_mean(x, H, W)``   f32 [G, n, A] -> f32 [n, A]: each image's per-cell output moved back to
                          the original cells and averaged in a fixed pairwise tree
  ``SymmetricModel(m)``   a policy averaged over the group, for ``evaluate_vec``

Everything on the device is a HIP kernel of csrc/mssym.hip on the current stream, no host sync.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L

PLANES = tuple(k for k, _, _ in L.SYM_PLANES)


def group_size(H: int, W: int) -> int:
    """The number of valid group elements of an [H, W] board: 8 if square, else 4."""
    return 8 if int(H) == int(W) else 4


def inverse(g: int) -> int:
    """The element that undoes ``g``: ``g`` itself below 4; with the transpose, the two reversals
    trade places (5 <-> 6)."""
    g = int(g)
    if not 0 <= g < 8:
        raise ValueError(f"g: expected 0..7, got {g}")
    return g if g < 4 else 4 | ((g & 1) << 1) | ((g >> 1) & 1)


def _check_shape(H: int, W: int) -> int:
    if H < 1 or W < 1 or H * W > L.MS_AVOID_MAX_CELLS:
        raise ValueError(f"symmetry: need 1 <= H, W and H*W <= {L.MS_AVOID_MAX_CELLS}, got {H}x{W}")
    return H * W


def cell_map(H: int, W: int, g: int) -> np.ndarray:
    """ms_sym_cell_map_host: i32 [H*W] with ``T_g(X).flat[i] == X.flat[map[i]]``."""
    out = np.empty(max(1, int(H) * int(W)), dtype=np.int32)  # a bad shape or g is refused by the call
    L.check(L.load().ms_sym_cell_map_host(int(H), int(W), int(g), out.ctypes.data))
    return out


def _device_of(*tensors) -> torch.device:
    for t in tensors:
        if t is not None:
            if t.device.type != "cuda":
                raise ValueError("symmetry: expected tensors on a HIP device")
            return t.device
    raise ValueError("symmetry: no tensor given")


def sym_gather(rows: Optional[torch.Tensor], g: torch.Tensor, H: int, W: int, *, codes=None, mask=None, best=None,
               labels=None, kind=None, status: bool = False,
               out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """ms_sym_gather: for each given source plane (``codes`` u8 [B, H, W], ``mask`` bool or u8
    [B, A], ``best`` u8 [B, A], ``labels`` f32 [B, A], ``kind`` u8 [B]) the tensor whose row i is
    ``T_{g[i]}`` of source row ``rows[i]`` (``kind``: copied). ``rows`` i64 [n], or None for the
    identity (n == B); ``g`` u8 [n]. A row whose index is outside [0, B) or whose ``g`` is not valid
    for the board comes back all zero with kind 0, and 1 in the u8 [n] ``status`` (returned with
    ``status=True``). ``out`` may hold preallocated contiguous outputs by the same names (a plane
    without a source is then skipped)."""
    A = _check_shape(int(H), int(W))
    src = dict(codes=codes, mask=mask, best=best, labels=labels, kind=kind)
    dev = _device_of(g, *src.values())
    if g.dtype != torch.uint8 or g.dim() != 1:
        raise ValueError("sym_gather: g must be uint8 [n]")
    n = g.shape[0]
    g = g.contiguous()
    if rows is not None:
        if rows.dtype != torch.int64 or tuple(rows.shape) != (n,):
            raise ValueError(f"sym_gather: rows must be int64 [{n}]")
        rows = rows.contiguous()
    B = None
    res: Dict[str, torch.Tensor] = {}
    ins = []
    for name, dt, cells in L.SYM_PLANES:
        t = src[name]
        if t is None:
            ins.append(None)
            continue
        want = (torch.uint8, torch.bool) if name == "mask" else (getattr(torch, dt),)
        if t.dtype not in want:
            raise ValueError(f"sym_gather: {name} must be {dt}, got {t.dtype}")
        B = t.shape[0] if B is None else B
        if t.shape[0] != B or t.numel() != B * (A if cells else 1):
            raise ValueError(f"sym_gather: {name} has shape {tuple(t.shape)}, expected {B} rows of {H}x{W}")
        t = t.contiguous()
        ins.append(t)
        if out is not None and name in out:
            o = out[name]
            if o.dtype != t.dtype or o.shape[0] != n or o.numel() != n * (A if cells else 1) or not o.is_contiguous():
                raise ValueError(f"sym_gather: out[{name!r}] must be contiguous {t.dtype} with {n} rows")
            res[name] = o
        elif out is None:
            res[name] = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
    if B is None:
        raise ValueError("sym_gather: no source plane given")
    st = torch.empty(n, dtype=torch.uint8, device=dev) if status else None
    with torch.cuda.device(dev):
        L.check(L.load().ms_sym_gather(L.ptr(rows), L.ptr(g), n, int(H), int(W), B, *(L.ptr(t) for t in ins),
                                       *(L.ptr(res.get(k)) for k in PLANES), L.ptr(st), L.stream_ptr(dev)))
    if status:
        res["status"] = st
    return res


def sym_expand(codes: torch.Tensor, G: Optional[int] = None) -> torch.Tensor:
    """ms_sym_expand: u8 [n, H, W] -> u8 [G, n, H, W] with ``out[g] = T_g(codes)``. ``G``: 1, 4 or
    8 (8 on square boards only); None takes ``group_size(H, W)``."""
    if codes.dtype != torch.uint8 or codes.dim() != 3:
        raise ValueError("sym_expand: codes must be uint8 [n, H, W]")
    dev = _device_of(codes)
    n, H, W = codes.shape
    _check_shape(H, W)
    G = group_size(H, W) if G is None else int(G)
    if G not in (1, 4, 8) or (G == 8 and H != W):
        raise ValueError(f"sym_expand: G must be 1, 4 or (square boards) 8, got {G} for {H}x{W}")
    codes = codes.contiguous()
    out = torch.empty((G, n, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().ms_sym_expand(L.ptr(codes), n, H, W, G, L.ptr(out), L.stream_ptr(dev)))
    return out


def sym_mean(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """ms_sym_mean: ``x`` f32 [G, n, H*W], ``x[g]`` a per-cell output for the boards transformed
    by ``g`` -> f32 [n, H*W], the mean over ``g`` of the entries that belong to each original cell.
    Fixed pairwise f32 tree and one multiply by 1/G: G equal terms give the term back exactly.
    ``H = W = 1`` averages a per-board scalar. Not differentiable."""
    H, W = int(H), int(W)
    A = _check_shape(H, W)
    if x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != A:
        raise ValueError(f"sym_mean: x must be float32 [G, n, {A}], got {x.dtype} {tuple(x.shape)}")
    dev = _device_of(x)
    G, n = x.shape[0], x.shape[1]
    if G not in (1, 4, 8) or (G == 8 and H != W):
        raise ValueError(f"sym_mean: G must be 1, 4 or (square boards) 8, got {G} for {H}x{W}")
    x = x.detach().contiguous()
    out = torch.empty((n, A), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().ms_sym_mean(L.ptr(x), n, H, W, G, L.ptr(out), L.stream_ptr(dev)))
    return out


class SymmetricModel(torch.nn.Module):
    """``model`` averaged over the symmetry group of the board: one forward on the G images of
    every board (``sym_expand``), each image's outputs moved back to the original cells and
    averaged (``sym_mean``). The average is over LOGITS (policy and mine logits; the value as a
    scalar), not over probabilities. For inference (``evaluate_vec``, ``python -m ms_amd.eval
    --symmetry``): the outputs carry no gradient. ``model`` is a submodule, so ``parameters()``,
    ``eval()`` and ``train()`` reach it; the forward runs under the caller's autocast."""

    def __init__(self, model: torch.nn.Module) -> None:
        super().__init__()
        self.model = model

    @torch.no_grad()
    def forward(self, obs: torch.Tensor, return_mine: bool = False):
        """obs: the env's f32 obs [n, 10, H, W] or its u8 cell codes [n, H, W]. Returns f32
        ``logits`` [n, A], ``value`` [n] and, with ``return_mine``, ``mine`` [n, 1, H, W]."""
        if obs.dtype == torch.uint8:
            codes = obs.contiguous()
        else:
            from .fused import obs_encode
            codes = torch.empty((obs.shape[0],) + tuple(obs.shape[2:]), dtype=torch.uint8, device=obs.device)
            obs_encode(obs.contiguous(), codes)
        n, H, W = codes.shape
        images = sym_expand(codes)
        G = images.shape[0]
        res = self.model(images.view(G * n, H, W), return_mine=return_mine)
        logits = sym_mean(res[0].float().reshape(G, n, H * W), H, W)
        value = sym_mean(res[1].float().reshape(G, n, 1), 1, 1).reshape(n)
        if return_mine:
            return logits, value, sym_mean(res[2].float().reshape(G, n, H * W), H, W).view(n, 1, H, W)
        return logits, value


__all__ = ["group_size", "inverse", "cell_map", "sym_gather", "sym_expand", "sym_mean", "SymmetricModel", "PLANES"]
