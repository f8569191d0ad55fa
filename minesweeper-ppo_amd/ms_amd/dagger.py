"""On-policy imitation (DAgger): the learner chooses the moves, the exact-posterior
player labels the states it reaches.

``dagger_act`` is the step that decides who plays (include/msdagger.h, one HIP launch, one
wavefront per board): per board two keyed coins pick a uniform legal click (probability
``explore``), else the learner's own move (probability 1 - ``beta``; the arg-max of
``evaluate_vec`` or a sample of its logits), else the teacher's move where the board has a target
and a uniform click where it has none. ``beta = 1`` is ``collect_expert``'s rule and reads no
logits; ``beta = 0`` plays the learner everywhere.

``collect_dagger`` has ``collect_expert``'s contract (ms_amd/imitate.py) and its carry, so the two
may alternate on one ``vec`` and buffer. Per step, all on the device and on one stream:
  vec.expert_targets   -> best / kind / labels of the boards as they stand, whoever plays
  model forward        -> the learner's logits (no grad, eval mode; skipped when beta >= 1)
  ms_dagger_act        -> the action, who chose it, the learner's move and whether the teacher agrees
  ms_step_codes        -> the next step's cell codes and action mask, straight into the buffer
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib as L
from .env import OBS_CHANNELS, VecMinesweeper
from .imitate import ExpertBuffer
from .ppo import _autocast

MODES = {"greedy": L.MS_DAGGER_GREEDY, "sample": L.MS_DAGGER_SAMPLE}
SOURCE_UNIFORM, SOURCE_EXPERT, SOURCE_LEARNER = (L.MS_DAGGER_SRC_UNIFORM, L.MS_DAGGER_SRC_EXPERT,
                                                 L.MS_DAGGER_SRC_LEARNER)
_U64 = 2**64 - 1


def _check_mix(beta: float, explore: float, mode: str) -> None:
    if not 0.0 <= float(beta) <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"beta: expected a probability, got {beta}")
    if not 0.0 <= float(explore) <= 1.0:
        raise ValueError(f"explore: expected a probability, got {explore}")
    if mode not in MODES:
        raise ValueError(f"mode: expected one of {sorted(MODES)}, got {mode!r}")


def dagger_act(logits: Optional[torch.Tensor], mask: torch.Tensor, targets: Dict[str, torch.Tensor], *, seed: int,
               counter: int, beta: float, explore: float = 0.0, mode: str = "greedy", row_begin: int = 0,
               out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """ms_dagger_act on device tensors: ``logits`` [n, A] (None only with ``beta >= 1``), ``mask``
    bool / u8 [n, A], ``targets`` the ``best`` / ``action`` / ``kind`` of ``expert_targets``. Row i
    draws from the hash streams of global row ``row_begin + i``. Returns ``action`` i64,
    ``source`` u8 (0 uniform, 1 teacher, 2 learner), ``learner_action`` i64 (-1 without logits) and
    ``agree`` u8 (the learner's move is one of the teacher's best), each [n]; ``out`` may hold
    tensors to write them into. One launch on the current stream, no host sync."""
    _check_mix(beta, explore, mode)
    if logits is None and float(beta) < 1.0:
        raise ValueError("dagger_act: logits may be None only with beta >= 1")
    n, A = mask.shape
    dev = mask.device
    if dev.type != "cuda":
        raise ValueError("dagger_act: expected tensors on a HIP device")
    if not 1 <= A <= L.MS_DAGGER_MAX_CELLS:
        raise ValueError(f"dagger_act needs 1 <= cells <= {L.MS_DAGGER_MAX_CELLS}, got {A}")
    lg = None
    if logits is not None:
        lg = logits.detach().float().contiguous()
        if tuple(lg.shape) != (n, A):
            raise ValueError(f"logits: expected shape {(n, A)}, got {tuple(lg.shape)}")
    m = mask.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m.ne(0).view(torch.uint8)
    best, act, kind = targets["best"].contiguous(), targets["action"].contiguous(), targets["kind"].contiguous()
    if best.dtype != torch.uint8 or kind.dtype != torch.uint8 or act.dtype != torch.int64:
        raise ValueError("targets: best and kind must be uint8 and action int64 (an expert_targets result)")
    if tuple(best.shape) != (n, A) or kind.numel() != n or act.numel() != n:
        raise ValueError(f"targets: expected {n} rows of {A} cells")
    res = {}
    for k, dt in L.DAGGER_OUTPUTS:
        t = out.get(k) if out is not None else None
        if t is None:
            t = torch.empty(n, dtype=getattr(torch, dt), device=dev)
        elif t.dtype != getattr(torch, dt) or t.numel() != n or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"out[{k!r}]: expected a contiguous {dt} tensor of {n} elements on {dev}")
        res[k] = t
    with torch.cuda.device(dev):
        L.check(L.load().ms_dagger_act(L.ptr(lg), L.ptr(m), L.ptr(best), L.ptr(act), L.ptr(kind), n, A,
                                       int(row_begin), int(seed) & _U64, int(counter) & _U64, float(beta),
                                       float(explore), MODES[mode], *(L.ptr(res[k]) for k, _ in L.DAGGER_OUTPUTS),
                                       L.stream_ptr(dev)))
    return res


@torch.no_grad()
def collect_dagger(vec: VecMinesweeper, model: torch.nn.Module, steps: int, *, beta: float, budget: int,
                   method: str = "grouped", explore: float = 0.0, mode: str = "greedy",
                   amp: Optional[torch.dtype] = None, seed: int, buffer: Optional[ExpertBuffer] = None,
                   reset: bool = True, lookahead: int = 0, margin: float = 0.1) -> ExpertBuffer:
    """``collect_expert`` with the move of every step chosen by ``dagger_act``: ``steps`` steps on
    every env of ``vec``, from a reset or (``reset=False``) from where the previous collection on
    this ``vec`` and ``buffer`` stopped, by either collector. Every row is labelled with the
    teacher's targets whoever played. ``model`` runs without grad in ``eval()`` mode under ``amp``
    autocast (its mode is put back afterwards) and is not called at all when ``beta >= 1``; with
    ``beta = 1, explore = 0`` the buffer and the carry are bitwise ``collect_expert(explore=0)``'s
    of the same seeds. The buffer additionally carries ``source`` u8 [B] (who played the row) and
    ``learner_agree`` u8 [B] (the learner's move was one of the teacher's best; 0 where the row has
    no target or no forward ran), and ``learner_action`` i64 [B] (-1 where no forward ran): plain
    attributes, not in ``FIELDS``. No host sync inside the loop. ``lookahead`` / ``margin``: the
    teacher's two-guess lookahead, as in ``collect_expert``."""
    if method not in L.POSTERIOR_METHODS:
        raise ValueError(f"method: expected one of {L.POSTERIOR_METHODS}, got {method!r}")
    _check_mix(beta, explore, mode)
    if lookahead != 0 or isinstance(lookahead, bool):
        from .lookahead import check_params
        check_params(lookahead, margin)
    from .fused import obs_encode
    N, H, W, A, dev = vec.num_envs, vec.H, vec.W, vec.H * vec.W, vec.device
    if buffer is None or buffer.num_envs != N or buffer.steps != steps or tuple(buffer.codes.shape[1:]) != (H, W):
        buffer = ExpertBuffer(N, steps, H, W, dev)
    for name, dt in (("source", torch.uint8), ("learner_agree", torch.uint8), ("learner_action", torch.int64)):
        if getattr(buffer, name, None) is None:
            setattr(buffer, name, torch.zeros(len(buffer), dtype=dt, device=dev))
    obs0 = torch.empty((N, OBS_CHANNELS, H, W), dtype=torch.float32, device=dev) if reset else None
    rewards = torch.empty(N, dtype=torch.float32, device=dev)
    dones = torch.empty(N, dtype=torch.bool, device=dev)
    actions = torch.empty(N, dtype=torch.int64, device=dev)
    last_codes = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    last_mask = torch.empty((N, A), dtype=torch.bool, device=dev)
    s = buffer.slot(0)
    if reset:
        vec.reset(out={"obs": obs0, "action_mask": s["mask"]})
        obs_encode(obs0, s["codes"])
    else:
        if buffer.carry is None or buffer.carry[0] is not vec:
            raise ValueError("collect_dagger(reset=False) continues the previous call on the same vec and buffer")
        s["codes"].copy_(buffer.carry[1])
        s["mask"].copy_(buffer.carry[2])
    forward = float(beta) < 1.0
    was_training = model.training if forward else None
    if forward:
        model.eval()
    try:
        for t in range(steps):
            tg = vec.expert_targets(budget=budget, method=method, hidden=s["mask"], lookahead=lookahead,
                                    margin=margin)
            s["best"].copy_(tg["best"])
            s["kind"].copy_(tg["kind"])
            s["labels"].copy_(tg["labels"])
            logits = None
            if forward:
                with _autocast(s["codes"], amp):
                    logits = model(s["codes"])[0]
            rows = slice(t * N, (t + 1) * N)
            dagger_act(logits, s["mask"], tg, seed=seed, counter=t, beta=beta, explore=explore, mode=mode,
                       row_begin=vec.env_begin,
                       out={"action": actions, "source": buffer.source[rows], "agree": buffer.learner_agree[rows],
                            "learner_action": buffer.learner_action[rows]})
            nxt = buffer.slot(t + 1) if t + 1 < steps else {"codes": last_codes, "mask": last_mask}
            vec.step(actions, out={"codes": nxt["codes"], "action_mask": nxt["mask"], "rewards": rewards,
                                   "dones": dones})
            s = nxt
    finally:
        if forward:
            model.train(was_training)
    buffer.carry = (vec, last_codes, last_mask)  # collect_expert's carry: either collector continues it
    return buffer


def dagger_shares(buffer: ExpertBuffer) -> Dict[str, float]:
    """Who played the rows of a ``collect_dagger`` buffer, and how often the learner's own move was
    one of the teacher's best on the rows that have a target (NaN when none has). One host sync."""
    if getattr(buffer, "source", None) is None or getattr(buffer, "learner_agree", None) is None:
        raise ValueError("dagger_shares: the buffer was not filled by collect_dagger")
    has = buffer.kind != L.MS_EXPERT_NONE
    c = torch.cat([torch.bincount(buffer.source.to(torch.int64), minlength=3)[:3],
                   torch.stack([(buffer.learner_agree.bool() & has).sum(), has.sum()])]).tolist()
    n = max(1, len(buffer))
    return {"share_uniform": c[SOURCE_UNIFORM] / n, "share_expert": c[SOURCE_EXPERT] / n,
            "share_learner": c[SOURCE_LEARNER] / n, "on_policy_agree": c[3] / c[4] if c[4] else float("nan")}


def beta_at(it: int, start: float, end: float, decay_iters: int) -> float:
    """The teacher's share of round ``it`` (0-based): linear from ``start`` at round 0 to ``end`` at
    round ``decay_iters``, ``end`` from there on; ``decay_iters <= 0`` is ``end`` from round 0."""
    if decay_iters <= 0 or it >= decay_iters:
        return float(end)
    return float(start) + (float(end) - float(start)) * (max(0, int(it)) / float(decay_iters))


__all__ = ["dagger_act", "collect_dagger", "dagger_shares", "beta_at", "MODES", "SOURCE_UNIFORM", "SOURCE_EXPERT",
           "SOURCE_LEARNER"]
