"""Exact mine-probability posterior (include/msposterior.h): for every hidden cell, the share of
the mine layouts consistent with the revealed numbers and the mine count that put a mine on it.

One HIP kernel launch over all boards (``posterior_states`` / ``VecMinesweeper.mine_posterior``)
and a plain C++ twin on the host (``posterior_host``): the exact fallback for the boards the
bounded device search reports undecided, and the only path that needs no device.

Every function returns the four per-env outputs of msposterior.h as a dict: ``status`` (0 not
analysed, 1 decided, 2 undecided), ``prob`` f64 [n, H*W] (0 at revealed cells and on boards
that are not decided), ``configs`` f64 [n] (the number of consistent layouts) and ``max_nodes``.

``PosteriorModel`` wraps the analysis as a policy: ``evaluate_vec(PosteriorModel(K), cfg)`` is
the greedy least-dangerous-cell player.

``method`` chooses the per-component counting: "enumerate" (the default: one node per cell value,
include/msposterior.h) or "grouped" (one node per value of a group of equivalent cells,
include/msposterior_grouped.h). Wherever both decide a board their ``prob`` and ``configs`` are
bitwise equal; "grouped" decides boards whose solutions are too many to list.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from .avoid import _dev_u8, _np_u8

# Nodes per query of the host fallback (16x the device default); boards past it stay status 2.
# Enumeration cannot finish a weakly constrained component (few numbers, many solutions) at any
# budget worth waiting for; the host gives a board up at its first stopped query (about 20 ms)
# and spends at most (free cells + 1) such queries on one it decides.
HOST_BUDGET = 1 << 20

# Nodes per query of the belief-target launch inside a rollout (VecMinesweeper.posterior_labels,
# collect_rollout(belief_targets="posterior")); a board past the budget keeps its 0 / 1 labels.
# A rule player's boards at 16x16x40 are decided within 2^11 nodes 99.76 % of the time, but the
# boards of an untrained policy's rollout (4,096 envs x 64 steps) only 96.7 % of the time, against
# 98.3 % within 2^12 and 94.5 % within 2^10: more than a point apart, so the budget is 2^12. At
# about 1.3 us per node that bounds a query at about 5 ms (DESIGN.md sections 12 and 13).
TRAIN_BUDGET = 1 << 12


def posterior_host(revealed, number, mine_count: int, live=None, host_budget: int = 0,
                   method: str = "enumerate") -> Dict[str, np.ndarray]:
    """ms_posterior_host (or, method "grouped", ms_posterior_host_grouped) on numpy arrays:
    revealed [n, H, W] (bool or u8), number u8 [n, H, W] (read at revealed cells only).
    host_budget: nodes per query, 0 = unbounded. Raises MsEnvError for a board no layout of
    ``mine_count`` mines can reproduce."""
    entry = L.posterior_entry("ms_posterior_host", method)
    revealed = np.asarray(revealed)
    if revealed.ndim != 3:
        raise ValueError(f"revealed: expected [n, H, W], got shape {revealed.shape}")
    n, H, W = revealed.shape
    rev = _np_u8(revealed, (n, H, W), "revealed")
    number = np.asarray(number)
    if number.shape != (n, H, W):
        raise ValueError(f"number: expected shape {(n, H, W)}, got {number.shape}")
    num = np.ascontiguousarray(number, dtype=np.uint8)
    lv = None if live is None else _np_u8(live, (n,), "live")
    out = {k: np.zeros((n, H * W) if cells else (n,), dtype=dt) for k, dt, cells in L.POSTERIOR_OUTPUTS}
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    L.check(entry(p(rev), p(num), int(mine_count), p(lv), n, H, W, int(host_budget),
                  *(p(out[k]) for k, _, _ in L.POSTERIOR_OUTPUTS)))
    return out


def _alloc(n: int, A: int, device) -> Dict[str, torch.Tensor]:
    return {k: torch.empty((n, A) if cells else (n,), dtype=getattr(torch, dt), device=device)
            for k, dt, cells in L.POSTERIOR_OUTPUTS}


def posterior_states(revealed: torch.Tensor, number: torch.Tensor, mine_count: int,
                     live: Optional[torch.Tensor] = None,
                     budget: int = L.MS_POSTERIOR_DEFAULT_BUDGET, method: str = "enumerate") -> Dict[str, torch.Tensor]:
    """ms_posterior_states (or, method "grouped", ms_posterior_states_grouped) on device tensors:
    revealed [n, H, W] (bool or u8), number [n, H, W] (any integer dtype; read at revealed cells
    only). No host fallback: a board may come back with status 2."""
    entry = L.posterior_entry("ms_posterior_states", method)
    if revealed.dim() != 3 or revealed.device.type != "cuda":
        raise ValueError("revealed: expected a [n, H, W] tensor on a HIP device")
    dev = revealed.device
    n, H, W = revealed.shape
    rev = _dev_u8(revealed, (n, H, W), "revealed", dev)
    num = torch.as_tensor(number, device=dev)
    if tuple(num.shape) != (n, H, W):
        raise ValueError(f"number: expected shape {(n, H, W)}, got {tuple(num.shape)}")
    num = num.to(torch.uint8).contiguous()
    lv = _dev_u8(live, (n,), "live", dev)
    out = _alloc(n, H * W, dev)
    with torch.cuda.device(dev):
        L.check(entry(L.ptr(rev), L.ptr(num), int(mine_count), L.ptr(lv), n, H, W, int(budget),
                      *(L.ptr(out[k]) for k, _, _ in L.POSTERIOR_OUTPUTS), L.stream_ptr(dev)))
    return out


def resolve_undecided(out: Dict[str, torch.Tensor], revealed: torch.Tensor, number: torch.Tensor, mine_count: int,
                      host_budget: Optional[int] = None, method: str = "enumerate") -> int:
    """Overwrites the status-2 rows of a device result with the host solver's answer for the
    boards ``revealed`` / ``number`` [n, H, W]; returns how many there were (one host sync; rows
    are copied only when there are such boards). Boards the host budget (default HOST_BUDGET)
    cannot finish either, and inconsistent boards, stay status 2. ``method``: the host solver's
    counting."""
    if method not in L.POSTERIOR_METHODS:
        raise ValueError(f"method: expected one of {L.POSTERIOR_METHODS}, got {method!r}")
    host_budget = HOST_BUDGET if host_budget is None else int(host_budget)
    und = torch.nonzero(out["status"] == L.MS_AVOID_UNDECIDED).reshape(-1)
    if und.numel() == 0:
        return 0
    rev = revealed[und].cpu().numpy()
    num = number[und].to(torch.uint8).cpu().numpy()
    for i in range(rev.shape[0]):  # board by board: one inconsistent board must not hide the others
        try:
            fixed = posterior_host(rev[i:i + 1], num[i:i + 1], mine_count, host_budget=host_budget, method=method)
        except L.MsEnvError:
            continue
        for k, v in fixed.items():
            out[k][und[i]] = torch.from_numpy(v).to(out[k].device)[0]
    return int(und.numel())


class PosteriorModel(torch.nn.Module):
    """The exact posterior as a policy: logits = -p shifted per board (so the greedy pick is a
    least-dangerous hidden cell, exactly, in float32 too), value 0, mine logits = logit(p)
    clamped to +-30. Revealed cells come from ``obs[:, 0]``, their numbers from the one-hot
    channels 1-9. Boards with nothing revealed get p = M / A on every cell; boards neither the
    device nor the host budget can finish keep p = 0 (no information) on every cell. ``method``:
    the counting of both the device search and the host fallback.

    ``lookahead=K`` (1 .. 16; 0 = off, the forward above) adds the two-guess lookahead of
    ms_amd/lookahead.py: on a guess board the chosen cell's logit becomes +1.0 (every other logit
    is at most 0), so the greedy arg-max is the lookahead's choice, exactly in float32. ``margin``
    and ``lookahead_cap`` (guess boards analysed per forward, default all) are its parameters. The
    module then keeps device-side running sums, read by ``lookahead_counters()``."""

    COUNTERS = ("guess_boards", "changed", "unscored_candidates", "overflow")

    def __init__(self, mine_count: int, budget: int = L.MS_POSTERIOR_DEFAULT_BUDGET,
                 host_budget: Optional[int] = None, method: str = "enumerate", *, lookahead: int = 0,
                 margin: float = 0.1, lookahead_cap: Optional[int] = None):
        super().__init__()
        if method not in L.POSTERIOR_METHODS:
            raise ValueError(f"method: expected one of {L.POSTERIOR_METHODS}, got {method!r}")
        if lookahead != 0 or isinstance(lookahead, bool):
            from .lookahead import check_params
            check_params(lookahead, margin, lookahead_cap)
        self.method = method
        self.mine_count, self.budget, self.host_budget = int(mine_count), int(budget), host_budget
        self.lookahead, self.margin, self.lookahead_cap = int(lookahead), float(margin), lookahead_cap
        self.dummy = torch.nn.Parameter(torch.zeros(1))  # gives the module a device
        if self.lookahead:
            self.register_buffer("_la_sums", torch.zeros(len(self.COUNTERS), dtype=torch.int64), persistent=False)

    def lookahead_counters(self) -> Dict[str, int]:
        """The running sums over every forward so far (one host sync): guess boards met, boards
        where the choice was not the greedy cell, candidates left unscored (a search ran out of
        budget), guess boards past ``lookahead_cap`` (played greedily)."""
        if not self.lookahead:
            return {k: 0 for k in self.COUNTERS}
        return dict(zip(self.COUNTERS, self._la_sums.tolist()))

    @torch.no_grad()
    def forward(self, obs: torch.Tensor, return_mine: bool = False):
        n, _, H, W = obs.shape
        rev = obs[:, 0] > 0.5
        number = obs[:, 1:10].argmax(dim=1).to(torch.uint8)
        out = posterior_states(rev, number, self.mine_count, budget=self.budget, method=self.method)
        resolve_undecided(out, rev, number, self.mine_count, self.host_budget, method=self.method)
        p = out["prob"]
        blank = ~rev.reshape(n, -1).any(dim=1)
        p = torch.where(blank[:, None], torch.full_like(p, self.mine_count / float(H * W)), p)
        # -p up to a per-board constant, so that float32 keeps the order exactly: a least-dangerous
        # hidden cell gets 0, every other hidden cell a negative number, revealed cells -2
        hidden = ~rev.reshape(n, -1)
        pmin = torch.where(hidden, p, torch.full_like(p, 2.0)).min(dim=1, keepdim=True).values
        logits = torch.where(hidden, pmin - p, torch.full_like(p, -2.0)).to(torch.float32)
        if self.lookahead:
            from .lookahead import counters, lookahead_states
            cap = n if self.lookahead_cap is None else int(self.lookahead_cap)
            res = lookahead_states(rev, number, self.mine_count, out, K=self.lookahead, margin=self.margin,
                                   budget=self.budget, method=self.method, cap=cap)
            picked = res["action"] >= 0
            cell = res["action"].clamp_min(0)[:, None]
            logits.scatter_(1, cell, torch.where(picked[:, None], torch.ones_like(logits[:, :1]), logits.gather(1, cell)))
            inc = counters(res, cap)
            self._la_sums += torch.stack([inc[k] for k in self.COUNTERS]).to(self._la_sums.device)
        value = torch.zeros(n, dtype=torch.float32, device=obs.device)
        if not return_mine:
            return logits, value
        mine = torch.logit(p).clamp(-30.0, 30.0).to(torch.float32).reshape(n, 1, H, W)
        return logits, value, mine


__all__ = ["posterior_host", "posterior_states", "resolve_undecided", "PosteriorModel", "HOST_BUDGET",
           "TRAIN_BUDGET"]
