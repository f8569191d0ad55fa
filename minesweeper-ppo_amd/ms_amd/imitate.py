"""Imitation warm start: states visited and labelled by the exact-posterior player, and a
behaviour-cloning update on them. An opt-in path beside PPO; it makes the
checkpoint that ``train_rl.py --init_ckpt`` takes.

``collect_expert`` plays ``steps`` steps on every env of a ``VecMinesweeper``. Per step, all on
the device and on one stream:
  vec.expert_targets   -> best / kind / labels of the boards as they stand (ms_posterior*, k_expert)
  ms_sample_masked     -> a uniform legal action per env (the keyed sampler on zero logits)
  ms_step_codes        -> the next step's u8 cell codes and action mask, straight into the buffer
Boards with a target (``kind`` != 0) take the expert's action; boards without one (before the first
click, or not decided within the budget) and, with probability ``explore``, any board take the
uniform one. There is no host round trip inside the loop. pretrain_il.py resets the envs once and
then continues the same games from one collection to the next. ``collect_dagger``
(ms_amd/dagger.py) is the on-policy variant with the same contract and carry: the
learner chooses a share 1 - beta of the moves; pretrain_il.py uses it in rounds whose beta is below 1.

``bc_update`` runs shuffled minibatches of one buffer through the model and the HIP loss of
ms_amd/bc_loss.py, under the autocast / GradScaler / fused-AdamW arrangement of ms_amd/ppo.py.
Single GPU only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib as L
from .bc_loss import OUT_KEYS, bc_loss_terms
from .dropout import MINIBATCH, keyed_dropout, mix_seed
from .env import OBS_CHANNELS, VecMinesweeper
from .expert import KIND_GUESS, KIND_NONE, KIND_SAFE
from .ppo import _autocast
from .rollout import sample_masked


@dataclass
class BCConfig:
    mini_batches: int = 8
    epochs: int = 1
    guess_weight: float = 1.0  # row weight of forced-guess states; 0 = learn from provably safe moves only
    ent_coef: float = 0.0
    aux_mine_weight: float = 0.0
    aux_mine_calib_weight: float = 0.0
    max_grad_norm: float = 0.5
    seed: int = 0
    augment: bool = False  # a fresh random board symmetry per row and epoch (ms_amd/symmetry.py)


class ExpertBuffer:
    """[steps * num_envs] rows, row t * num_envs + e as in RolloutBuffer: ``codes`` u8 [B, H, W] (the
    policy's cell-code input), ``mask`` bool [B, A], ``best`` u8 [B, A], ``kind`` u8 [B],
    ``labels`` f32 [B, A] (the exact mine probability at hidden cells)."""

    FIELDS = ("codes", "mask", "best", "kind", "labels")

    def __init__(self, num_envs: int, steps: int, H: int, W: int, device):
        B, A = num_envs * steps, H * W
        self.num_envs, self.steps, self.device = num_envs, steps, torch.device(device)
        self.codes = torch.zeros((B, H, W), dtype=torch.uint8, device=device)
        self.mask = torch.zeros((B, A), dtype=torch.bool, device=device)
        self.best = torch.zeros((B, A), dtype=torch.uint8, device=device)
        self.kind = torch.zeros((B,), dtype=torch.uint8, device=device)
        self.labels = torch.zeros((B, A), dtype=torch.float32, device=device)
        self.carry = None  # (vec, codes, mask) after the last collected step (collect_expert(reset=False))

    def __len__(self) -> int:
        return self.kind.shape[0]

    def slot(self, t: int) -> Dict[str, torch.Tensor]:
        s, e = t * self.num_envs, (t + 1) * self.num_envs
        return {k: getattr(self, k)[s:e] for k in self.FIELDS}

    def gather(self, rows: torch.Tensor, g: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The rows ``rows`` of every field; with ``g`` (u8 per row, ms_amd/symmetry.py) each row's
        board, mask, best set and labels under the symmetry ``g[i]``, in one launch (ms_sym_gather)."""
        if g is None:
            d = {k: getattr(self, k)[rows] for k in self.FIELDS}
        else:
            from .symmetry import sym_gather
            H, W = self.codes.shape[1:]
            d = sym_gather(rows, g, H, W, **{k: getattr(self, k) for k in self.FIELDS})
        d["rows"] = rows
        return d

    def kind_shares(self) -> Dict[str, float]:
        """Shares of the rows without a target, with a provably safe move, with a forced guess
        (one host sync)."""
        c = torch.bincount(self.kind.to(torch.int64), minlength=3)[:3].tolist()
        n = max(1, len(self))
        return {"kind_none": c[KIND_NONE] / n, "kind_safe": c[KIND_SAFE] / n, "kind_guess": c[KIND_GUESS] / n}


@torch.no_grad()
def collect_expert(vec: VecMinesweeper, steps: int, *, budget: int, method: str = "grouped", explore: float = 0.0,
                   seed: int, buffer: Optional[ExpertBuffer] = None, reset: bool = True, lookahead: int = 0,
                   margin: float = 0.1) -> ExpertBuffer:
    """``steps`` steps of the exact-posterior player on every env of ``vec``, as an ``ExpertBuffer``:
    from a reset, or with ``reset=False`` from where the previous call on this ``vec`` and
    ``buffer`` stopped (the posterior player needs more than 100 clicks for a 16x16x40 game, so
    only a continued collection reaches the late game). ``budget``: nodes per query of the device
    search; ``method``: its counting. ``explore``: the probability of a uniform legal action in
    place of the expert's (the state is still labelled with the expert's targets). ``seed`` keys
    the uniform actions and the coins: the same vec seed and ``seed`` give a bitwise equal buffer.
    ``buffer`` may be passed back in. ``lookahead`` / ``margin``: the teacher's two-guess lookahead on
    forced guesses (``VecMinesweeper.expert_targets``; 0 = the greedy teacher)."""
    if method not in L.POSTERIOR_METHODS:
        raise ValueError(f"method: expected one of {L.POSTERIOR_METHODS}, got {method!r}")
    if not 0.0 <= float(explore) <= 1.0:
        raise ValueError(f"explore: expected a probability, got {explore}")
    if lookahead != 0 or isinstance(lookahead, bool):
        from .lookahead import check_params
        check_params(lookahead, margin)
    from .fused import obs_encode
    N, H, W, A, dev = vec.num_envs, vec.H, vec.W, vec.H * vec.W, vec.device
    if buffer is None or buffer.num_envs != N or buffer.steps != steps or tuple(buffer.codes.shape[1:]) != (H, W):
        buffer = ExpertBuffer(N, steps, H, W, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    zeros = torch.zeros((N, A), dtype=torch.float32, device=dev)
    obs0 = torch.empty((N, OBS_CHANNELS, H, W), dtype=torch.float32, device=dev) if reset else None
    rewards = torch.empty(N, dtype=torch.float32, device=dev)
    dones = torch.empty(N, dtype=torch.bool, device=dev)
    last_codes = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    last_mask = torch.empty((N, A), dtype=torch.bool, device=dev)
    s = buffer.slot(0)
    if reset:
        vec.reset(out={"obs": obs0, "action_mask": s["mask"]})
        obs_encode(obs0, s["codes"])
    else:
        if buffer.carry is None or buffer.carry[0] is not vec:
            raise ValueError("collect_expert(reset=False) continues the previous call on the same vec and buffer")
        s["codes"].copy_(buffer.carry[1])
        s["mask"].copy_(buffer.carry[2])
    for t in range(steps):
        tg = vec.expert_targets(budget=budget, method=method, hidden=s["mask"], lookahead=lookahead, margin=margin)
        s["best"].copy_(tg["best"])
        s["kind"].copy_(tg["kind"])
        s["labels"].copy_(tg["labels"])
        uniform, _ = sample_masked(zeros, s["mask"], seed, t, row_begin=vec.env_begin)
        coin = torch.rand(N, device=dev, generator=gen) < float(explore)
        actions = torch.where((tg["kind"] != KIND_NONE) & ~coin, tg["action"], uniform)
        nxt = buffer.slot(t + 1) if t + 1 < steps else {"codes": last_codes, "mask": last_mask}
        vec.step(actions, out={"codes": nxt["codes"], "action_mask": nxt["mask"], "rewards": rewards, "dones": dones})
        s = nxt
    buffer.carry = (vec, last_codes, last_mask)  # the state after the last step, for reset=False
    return buffer


def _row_weight(kind: torch.Tensor, guess_weight: float) -> torch.Tensor:
    w = torch.zeros(kind.shape, dtype=torch.float32, device=kind.device)
    w = torch.where(kind == KIND_SAFE, torch.ones_like(w), w)
    return torch.where(kind == KIND_GUESS, torch.full_like(w, float(guess_weight)), w)


def bc_losses(model, batch: Dict[str, torch.Tensor], cfg: BCConfig,
              amp: Optional[torch.dtype]) -> Dict[str, torch.Tensor]:
    """Forward + the loss terms of include/msbc.h on one minibatch (``ExpertBuffer.gather``), as
    0-dim tensors (no host sync). weight = 1 for kind 1, ``cfg.guess_weight`` for kind 2, 0 for
    kind 0; the belief terms count the hidden cells of the rows that have a target."""
    need_mine = cfg.aux_mine_weight > 0 or cfg.aux_mine_calib_weight > 0
    kind, mask = batch["kind"], batch["mask"]
    with _autocast(batch["codes"], amp):
        if need_mine:
            logits, _, mine = model(batch["codes"], return_mine=True)
        else:
            logits, _ = model(batch["codes"], return_mine=False)
            mine = None
        valid = mask & (kind != KIND_NONE)[:, None]
        t = bc_loss_terms(logits, mine, mask, batch["best"], _row_weight(kind, cfg.guess_weight),
                          labels=batch["labels"] if need_mine else None, valid=valid if need_mine else None,
                          ent_coef=cfg.ent_coef, aux_mine_weight=cfg.aux_mine_weight,
                          aux_mine_calib_weight=cfg.aux_mine_calib_weight, world=1)
    return {k: t[i] for i, k in enumerate(OUT_KEYS)}


def _drop_packed_weights() -> None:
    """ms_amd/fused.py keeps 16-bit re-layouts of the trunk's and the heads' weights, keyed by the
    parameters' version counters. torch's fused AdamW (the Trainer's optimizer) writes the
    parameters without advancing those counters, so after a step the re-layouts would stay those
    of the old weights: the forward would never see the trunk and head weights it is training, and
    a checkpoint would hold weights that no forward ever used. Dropping the cached copies after
    every step makes the next forward re-lay them out (two launches)."""
    from . import fused
    fused._wcache.clear()
    fused._hcache.clear()


def bc_step(model, batch: Dict[str, torch.Tensor], optimizer, cfg: BCConfig, amp: Optional[torch.dtype] = None,
            scaler=None) -> Dict[str, torch.Tensor]:
    """One optimizer step on one minibatch: backward, unscale, clip_grad_norm_(max_grad_norm),
    step, as ppo_update does. Returns the loss terms of the step's forward, on the device."""
    out = bc_losses(model, batch, cfg, amp)
    optimizer.zero_grad(set_to_none=True)
    if scaler is not None:
        scaler.scale(out["loss"]).backward()
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.max_grad_norm)
        scaler.step(optimizer)
        scaler.update()
    else:
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.max_grad_norm)
        optimizer.step()
    _drop_packed_weights()
    return {k: v.detach() for k, v in out.items()}


def bc_update(model, buffer: ExpertBuffer, optimizer, cfg: BCConfig, amp: Optional[torch.dtype] = None,
              scaler=None, *, counter: int = 0) -> Dict[str, float]:
    """``cfg.epochs`` passes over ``buffer`` in ``cfg.mini_batches`` shuffled minibatches each
    (one device randperm per epoch, seeded by ``cfg.seed``, ``counter`` and the epoch). With
    ``cfg.augment`` every row is shown under a board symmetry drawn per epoch from the same
    generator after the permutation, so the minibatches' rows are those of ``augment=False``. Returns
    the means of the loss terms over the steps, ``bad_rows`` summed (one host sync at the end).
    ``amp``: the autocast type (torch.float16 with a GradScaler, torch.bfloat16) or None for fp32."""
    model.train()
    B = len(buffer)
    size = max(1, B // max(1, cfg.mini_batches))
    dseed = mix_seed(cfg.seed, MINIBATCH)
    acc: Dict[str, torch.Tensor] = {}
    n = 0
    for epoch in range(cfg.epochs):
        gen = torch.Generator(device=buffer.device)
        gen.manual_seed((int(cfg.seed) * 1000003 + int(counter)) * 64 + epoch)
        perm = torch.randperm(B, device=buffer.device, generator=gen)
        g = None
        if cfg.augment:
            from .symmetry import group_size
            g = torch.randint(0, group_size(*buffer.codes.shape[1:]), (B,), dtype=torch.uint8, device=buffer.device,
                              generator=gen)
        for k, s in enumerate(range(0, B - size + 1, size)):
            rows = perm[s:s + size]
            batch = buffer.gather(rows) if g is None else buffer.gather(rows, g[rows])
            with keyed_dropout(model, batch["rows"], dseed, (((int(counter) << 8) + epoch) << 16) + k):
                st = bc_step(model, batch, optimizer, cfg, amp, scaler)
            for name, v in st.items():
                acc[name] = acc[name] + v.float() if name in acc else v.float()
            n += 1
    keys = sorted(acc)
    vals = torch.stack([acc[k] if k == "bad_rows" else acc[k] / max(1, n) for k in keys]).tolist()
    return dict(zip(keys, vals))


def imitation_params(extras: Dict) -> Dict:
    """The YAML ``imitation:`` section with its defaults (configs/imitation/)."""
    d = dict(extras.get("imitation") or {}) if isinstance(extras, dict) else {}
    out = {"num_envs": 1024, "steps_per_env": 64, "mini_batches": 16, "epochs": 1, "iters": 100,
           "budget": 1 << 12, "method": "grouped", "explore": 0.05, "guess_weight": 1.0, "ent_coef": 0.0,
           "augment": False, "beta_start": 1.0, "beta_end": 1.0, "beta_decay_iters": 0, "learner": "greedy",
           "lookahead": 0, "lookahead_margin": 0.1}
    unknown = sorted(set(d) - set(out))
    if unknown:
        raise ValueError(f"imitation: unknown keys {unknown}")
    out.update(d)
    return out


def main(argv=None) -> None:
    """pretrain_il.py: alternate collect_expert and bc_update, write train_metrics.csv and
    checkpoints in the Trainer's format (``train_rl.py --init_ckpt``, ``python -m ms_amd.eval --ckpt``).
    With a beta schedule (``beta_start`` / ``beta_end`` / ``beta_decay_iters``, ms_amd/dagger.py) a
    round whose beta is below 1 is collected on policy by ``collect_dagger`` on the same games."""
    import argparse
    import csv
    import logging
    import os
    import time

    from .dagger import MODES, beta_at, collect_dagger, dagger_shares
    from .train import Trainer, load_config
    ap = argparse.ArgumentParser(description="Behaviour-cloning warm start from the exact-posterior player")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--out", type=str, default="runs/il")
    ap.add_argument("--iters", type=int, default=None, help="collect + update rounds (imitation.iters)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--amp", choices=["bf16", "fp16", "fp32"], default="fp16")
    ap.add_argument("--budget", type=int, default=None, help="nodes per posterior query (imitation.budget)")
    ap.add_argument("--method", choices=list(L.POSTERIOR_METHODS), default=None)
    ap.add_argument("--explore", type=float, default=None, help="probability of a uniform legal action per step")
    ap.add_argument("--guess_weight", type=float, default=None,
                    help="row weight of forced-guess states (0: learn from provably safe moves only)")
    ap.add_argument("--augment", action="store_true", default=None,
                    help="a fresh random board symmetry per row and epoch (imitation.augment)")
    ap.add_argument("--epochs", type=int, default=None, help="passes over each collected buffer (imitation.epochs)")
    ap.add_argument("--beta_start", type=float, default=None,
                    help="the teacher's share of the moves in round 1 (imitation.beta_start; 1 = collect_expert)")
    ap.add_argument("--beta_end", type=float, default=None, help="its share from round beta_decay_iters + 1 on")
    ap.add_argument("--beta_decay_iters", type=int, default=None, help="rounds of the linear beta schedule")
    ap.add_argument("--learner", choices=["greedy", "sample"], default=None,
                    help="the learner's own move in on-policy rounds: arg-max or a sample of its logits")
    ap.add_argument("--lookahead", type=int, default=None,
                    help="candidates of the teacher's two-guess lookahead on forced guesses (imitation.lookahead; 0 off)")
    ap.add_argument("--lookahead_margin", type=float, default=None,
                    help="candidates lie within this of the least mine probability (imitation.lookahead_margin)")
    ap.add_argument("--max_seconds", type=float, default=None,
                    help="stop after the round that passes this wall time (default: run all rounds)")
    ap.add_argument("--save_every", type=int, default=20)
    args = ap.parse_args(argv)
    cfg, env_d, model_d, extras = load_config(args.config)
    il = imitation_params(extras)
    for k in ("iters", "budget", "method", "explore", "guess_weight", "augment", "epochs", "beta_start", "beta_end",
              "beta_decay_iters", "learner", "lookahead", "lookahead_margin"):
        if getattr(args, k) is not None:
            il[k] = getattr(args, k)
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(message)s", datefmt="%H:%M:%S")
    log = logging.getLogger("ms_amd.imitate")
    device = torch.device("cuda", torch.cuda.current_device())
    cfg.num_envs, cfg.steps_per_env, cfg.total_updates = int(il["num_envs"]), int(il["steps_per_env"]), int(il["iters"])
    tr = Trainer(cfg, env_d, model_d, extras, seed=args.seed, amp=args.amp, device=device)
    bc = BCConfig(mini_batches=int(il["mini_batches"]), epochs=int(il["epochs"]),
                  guess_weight=float(il["guess_weight"]),
                  ent_coef=float(il["ent_coef"]), aux_mine_weight=cfg.aux_mine_weight,
                  aux_mine_calib_weight=cfg.aux_mine_calib_weight, max_grad_norm=cfg.max_grad_norm, seed=args.seed,
                  augment=bool(il["augment"]))
    if il["learner"] not in MODES:
        raise ValueError(f"imitation.learner: expected one of {sorted(MODES)}, got {il['learner']!r}")
    for k in ("beta_start", "beta_end"):
        if not 0.0 <= float(il[k]) <= 1.0:
            raise ValueError(f"imitation.{k}: expected a probability, got {il[k]}")
    if int(il["lookahead"]):
        from .lookahead import check_params
        check_params(int(il["lookahead"]), float(il["lookahead_margin"]))
    la = {"lookahead": int(il["lookahead"]), "margin": float(il["lookahead_margin"])}
    os.makedirs(args.out, exist_ok=True)
    rows, buf = [], None
    t_start = time.perf_counter()
    for it in range(int(il["iters"])):
        if args.max_seconds is not None and time.perf_counter() - t_start > args.max_seconds:
            break
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        beta = beta_at(it, float(il["beta_start"]), float(il["beta_end"]), int(il["beta_decay_iters"]))
        if beta >= 1.0:
            buf = collect_expert(tr.vec, cfg.steps_per_env, budget=int(il["budget"]), method=il["method"],
                                 explore=float(il["explore"]), seed=args.seed * 7919 + it, buffer=buf, reset=it == 0,
                                 **la)
            # no forward ran: the learner played nothing, and who else played was not recorded
            nan = float("nan")
            mix = {"share_learner": 0.0, "share_expert": nan, "share_uniform": nan, "on_policy_agree": nan}
        else:
            buf = collect_dagger(tr.vec, tr.model, cfg.steps_per_env, beta=beta, budget=int(il["budget"]),
                                 method=il["method"], explore=float(il["explore"]), mode=il["learner"],
                                 amp=tr.amp_dtype, seed=args.seed * 7919 + it, buffer=buf, reset=it == 0, **la)
            mix = dagger_shares(buf)
        shares = buf.kind_shares()  # syncs: the collect time is the device's
        t1 = time.perf_counter()
        st = bc_update(tr.model, buf, tr.opt, bc, tr.amp_dtype, tr.scaler, counter=it)
        tr.sched.step()
        t2 = time.perf_counter()
        rows.append({"iter": it + 1, "collect_s": t1 - t0, "update_s": t2 - t1, "beta": beta, **mix, **shares, **st})
        log.info(f"iter {it + 1}/{il['iters']} | collect {t1 - t0:.2f}s update {t2 - t1:.2f}s | "
                 f"ce={st['policy_ce']:.4f} "
                 f"agree={st['agree']:.4f} loss={st['loss']:.4f} bad={st['bad_rows']:.0f} | none/safe/guess "
                 f"{shares['kind_none']:.3f}/{shares['kind_safe']:.3f}/{shares['kind_guess']:.3f}" +
                 (f" | beta {beta:.3f} learner {mix['share_learner']:.3f} on-policy agree "
                  f"{mix['on_policy_agree']:.4f}" if beta < 1.0 else ""))
        if (it + 1) % max(1, args.save_every) == 0:
            tr.checkpoint(os.path.join(args.out, "ckpt_latest.pt"))
    with open(os.path.join(args.out, "train_metrics.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=sorted(set().union(*rows)) if rows else [])
        w.writeheader()
        w.writerows(rows)
    tr.checkpoint(os.path.join(args.out, "ckpt_latest.pt"))
    tr.checkpoint(os.path.join(args.out, "ckpt_final.pt"))


__all__ = ["BCConfig", "ExpertBuffer", "collect_expert", "bc_losses", "bc_step", "bc_update", "imitation_params",
           "main"]
