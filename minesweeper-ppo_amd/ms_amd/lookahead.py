"""Two-guess lookahead of the exact-posterior player (include/mslookahead.h).

On a board where every move risks a mine (a *guess board*), the ``K`` least dangerous hidden cells
within ``margin`` of the smallest mine probability are scored by the probability of surviving the
click and, where no safe move follows it, the next guess too; the best-scoring cell is chosen in
place of the greedy least-dangerous one.

``lookahead_states`` (device tensors, no host sync) expands every guess board into its K * 9
hypothetical boards "candidate c shows v" (ms_lookahead_expand), analyses them with the unchanged
``ms_posterior_states*`` entry point and applies the rule (ms_lookahead_score).
``lookahead_host`` is the same on numpy through the plain C++ twin (ms_lookahead_host); with the
same ``budget`` its results are bitwise the device's. Both return a dict:

  ``slot`` i32 [n]        the guess boards' slots 0, 1, ... in board order; -1 on other boards and
                          on guess boards past the first ``cap``;
  ``count`` i32 [1]       the number of guess boards (those past ``cap`` included);
  ``cand`` i32 [cap, K]   the candidates of each slot in (prob, index) order, -1 padding;
  ``action`` i64 [n]      the chosen cell, -1 on boards without a slot;
  ``score`` f64 [cap, K]  NaN where the candidate is unscored (a search ran out of budget) or padding;
  ``n_scored`` i32 [n]    scored candidates;
  ``changed`` u8 [n]      1 iff the choice is not the greedy cell (candidate 0).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from .avoid import _dev_u8, _np_u8

OUTPUTS = (("slot", "int32", "n"), ("count", "int32", "1"), ("cand", "int32", "cap"), ("action", "int64", "n"),
           ("score", "float64", "cap"), ("n_scored", "int32", "n"), ("changed", "uint8", "n"))


def check_params(K: int, margin: float, cap: Optional[int] = None) -> None:
    if not isinstance(K, (int, np.integer)) or isinstance(K, bool) or not 1 <= K <= L.MS_LOOKAHEAD_MAX_K:
        raise ValueError(f"lookahead: expected 1 <= K <= {L.MS_LOOKAHEAD_MAX_K}, got {K!r}")
    if not (isinstance(margin, (int, float)) and 0.0 <= float(margin) <= 1.0):  # NaN fails both comparisons
        raise ValueError(f"lookahead margin: expected a number in [0, 1], got {margin!r}")
    if cap is not None and int(cap) < 1:
        raise ValueError(f"lookahead cap: expected >= 1, got {cap!r}")


def _shape(kind: str, n: int, cap: int, K: int):
    return {"n": (n,), "1": (1,), "cap": (cap, K)}[kind]


def workspace_bytes(cap: int, K: int, H: int, W: int) -> int:
    """Bytes of the expanded boards and their posterior result for ``cap`` slots."""
    rows = cap * K * L.MS_LOOKAHEAD_OUTCOMES
    return rows * (H * W * (1 + 1 + 8) + 1 + 1 + 8 + 4)


def lookahead_host(revealed, number, mine_count: int, base: Dict[str, np.ndarray], K: int = 8, margin: float = 0.1,
                   budget: int = 0, method: str = "enumerate", cap: Optional[int] = None) -> Dict[str, np.ndarray]:
    """ms_lookahead_host on numpy arrays: revealed / number [n, H, W] as ``posterior_host`` takes
    them, ``base`` its result for them (``status``, ``prob``, ``configs``). ``budget``: nodes per
    query of the outcome boards' searches, 0 = unbounded."""
    if method not in L.POSTERIOR_METHODS:
        raise ValueError(f"method: expected one of {L.POSTERIOR_METHODS}, got {method!r}")
    revealed = np.asarray(revealed)
    if revealed.ndim != 3:
        raise ValueError(f"revealed: expected [n, H, W], got shape {revealed.shape}")
    n, H, W = revealed.shape
    cap = n if cap is None else int(cap)
    check_params(K, margin, cap)
    rev = _np_u8(revealed, (n, H, W), "revealed")
    number = np.asarray(number)
    if number.shape != (n, H, W):
        raise ValueError(f"number: expected shape {(n, H, W)}, got {number.shape}")
    num = np.ascontiguousarray(number, dtype=np.uint8)
    status = np.ascontiguousarray(base["status"], dtype=np.uint8).reshape(n)
    prob = np.ascontiguousarray(base["prob"], dtype=np.float64).reshape(n, H * W)
    configs = np.ascontiguousarray(base["configs"], dtype=np.float64).reshape(n)
    out = {k: np.zeros(_shape(kind, n, cap, K), dtype=dt) for k, dt, kind in OUTPUTS}
    p = lambda a: a.ctypes.data  # noqa: E731
    L.check(L.load().ms_lookahead_host(p(status), p(prob), p(configs), p(rev), p(num), int(mine_count), n, H, W, int(K),
                                       float(margin), cap, int(budget), int(method == "grouped"),
                                       *(p(out[k]) for k, _, _ in OUTPUTS)))
    return out


def lookahead_states(revealed: torch.Tensor, number: torch.Tensor, mine_count: int, base: Dict[str, torch.Tensor],
                     K: int = 8, margin: float = 0.1, budget: int = L.MS_POSTERIOR_DEFAULT_BUDGET,
                     method: str = "enumerate", cap: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The lookahead of the boards revealed / number [n, H, W] (as ``posterior_states`` takes them)
    whose posterior result is ``base`` (``status`` u8 [n], ``prob`` f64 [n, H*W], ``configs`` f64
    [n]; any ms_posterior* call). ``budget`` and ``method``: the device search of the outcome
    boards. ``cap`` (default n): slots, that is guess boards analysed; the workspace is
    ``workspace_bytes(cap, K, H, W)``. Six launches on the current stream, no host sync, no host
    fallback: a candidate with an outcome the search does not finish stays unscored."""
    entry = L.posterior_entry("ms_posterior_states", method)
    if revealed.dim() != 3 or revealed.device.type != "cuda":
        raise ValueError("revealed: expected a [n, H, W] tensor on a HIP device")
    dev = revealed.device
    n, H, W = revealed.shape
    A = H * W
    cap = n if cap is None else int(cap)
    check_params(K, margin, cap)
    K = int(K)
    rev = _dev_u8(revealed, (n, H, W), "revealed", dev)
    num = torch.as_tensor(number, device=dev)
    if tuple(num.shape) != (n, H, W):
        raise ValueError(f"number: expected shape {(n, H, W)}, got {tuple(num.shape)}")
    num = num.to(torch.uint8).contiguous()
    status, prob, configs = base["status"], base["prob"], base["configs"]
    if status.dtype != torch.uint8 or prob.dtype != torch.float64 or configs.dtype != torch.float64:
        raise ValueError("lookahead_states: base must be a posterior result (status uint8, prob and configs float64)")
    status, prob, configs = status.reshape(n).contiguous(), prob.reshape(n, A).contiguous(), configs.reshape(n).contiguous()
    out = {k: torch.empty(_shape(kind, n, cap, K), dtype=getattr(torch, dt), device=dev) for k, dt, kind in OUTPUTS}
    rows = cap * K * L.MS_LOOKAHEAD_OUTCOMES
    rev2 = torch.empty((rows, H, W), dtype=torch.uint8, device=dev)
    num2 = torch.empty((rows, H, W), dtype=torch.uint8, device=dev)
    live2 = torch.empty((rows,), dtype=torch.uint8, device=dev)
    post2 = {k: torch.empty((rows, A) if cells else (rows,), dtype=getattr(torch, dt), device=dev)
             for k, dt, cells in L.POSTERIOR_OUTPUTS}
    lib = L.load()
    with torch.cuda.device(dev):
        s = L.stream_ptr(dev)
        L.check(lib.ms_lookahead_expand(L.ptr(status), L.ptr(prob), L.ptr(rev), L.ptr(num), n, H, W, K, float(margin),
                                        cap, L.ptr(out["slot"]), L.ptr(out["count"]), L.ptr(out["cand"]), L.ptr(rev2),
                                        L.ptr(num2), L.ptr(live2), s))
        L.check(entry(L.ptr(rev2), L.ptr(num2), int(mine_count), L.ptr(live2), rows, H, W, int(budget),
                      *(L.ptr(post2[k]) for k, _, _ in L.POSTERIOR_OUTPUTS), s))
        L.check(lib.ms_lookahead_score(L.ptr(out["slot"]), L.ptr(out["cand"]), L.ptr(prob), L.ptr(configs),
                                       L.ptr(post2["status"]), L.ptr(post2["prob"]), L.ptr(post2["configs"]),
                                       L.ptr(rev2), int(mine_count), n, H, W, K, cap, L.ptr(out["action"]),
                                       L.ptr(out["score"]), L.ptr(out["n_scored"]), L.ptr(out["changed"]), s))
    return out


def counters(res: Dict[str, torch.Tensor], cap: int) -> Dict[str, torch.Tensor]:
    """The four running-sum increments of one ``lookahead_states`` result, as 0-dim i64 device
    tensors (no host sync): guess boards, boards whose choice is not the greedy cell, candidates left
    unscored, guess boards past ``cap``."""
    count = res["count"][0].to(torch.int64)
    n_cand = (res["cand"] >= 0).sum()
    return {"guess_boards": count, "changed": res["changed"].sum(dtype=torch.int64),
            "unscored_candidates": n_cand - res["n_scored"].sum(dtype=torch.int64),
            "overflow": (count - cap).clamp_min(0)}


__all__ = ["lookahead_states", "lookahead_host", "counters", "check_params", "workspace_bytes", "OUTPUTS"]
