"""Greedy evaluation on device: win rate + Wilson CI, steps, progress, invalid-action
rate, belief AUROC / ECE over unknown cells.

Reference: eval.py:265-511 (``evaluate_vec``), AUROC eval.py:54-66, ECE eval.py:69-90,
Wilson interval eval.py:447-458, CLI eval.py:526-640. The episode bookkeeping follows
the reference loop exactly (a batch of ``num_envs`` envs; each env's current episode
is counted once; the env stream is NOT reset between batches; envs past
``batch_size`` in a final partial batch still count, as in the reference), but every
per-env quantity is a device tensor: one host sync per step (the loop condition).

The avoidability diagnostics (``forced_guess_*``, ``safe_option_*``, component sizes;
eval.py:381-398, 421-422, 469-488 via avoidability.py) are opt-in: with
``diagnostics=True`` every live board is analysed on device before each step (one launch,
``VecMinesweeper.avoidability``; include/mssolve.h) and the counters behind the nine keys are
device accumulators. The count of boards the bounded device search left undecided rides on
the step's one host sync; such boards (none in any run measured) are re-solved
exactly on the host from a device copy of the pre-step planes. With the default
``diagnostics=False`` the nine keys are NaN, so callers that print the reference's summary
work. Not computed: rules.analyze_forced_modules (eval.py:363-379), which feeds only
counters that never reach the reference's result dict.

``posterior=True`` (not in the reference) scores the run against the exact posterior mine
probability (include/msposterior.h; one launch per step over the live boards past their first
click, before the step): the belief head per hidden cell (``belief_posterior_mae``,
``belief_posterior_kl``) and every move against the least-dangerous cell (``chosen_mine_prob``,
``guess_regret``, ``optimal_pick_rate``). Boards the bounded device search leaves undecided go
through the host solver like the avoidability ones; ``posterior_undecided`` counts those the
host budget could not finish either, which are left out.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import Callable, Dict, Optional

import numpy as np
import torch

from .env import EnvConfig, VecMinesweeper

NAN = float("nan")
_AVOIDABILITY_KEYS = ("forced_guess_rate", "forced_guess_success_rate", "forced_guess_episode_rate",
                   "safe_option_rate", "safe_option_miss_rate", "safe_option_pick_rate",
                   "avg_safe_options_per_turn", "avg_frontier_component_size", "avg_selected_component_size")


def wilson_interval(successes: int, total: int, z: float = 1.96) -> tuple:
    """95 % Wilson score interval (eval.py:447-458)."""
    if total <= 0:
        return NAN, NAN
    phat = successes / float(total)
    denom = 1.0 + (z * z) / total
    center = phat + (z * z) / (2.0 * total)
    rad = z * math.sqrt((phat * (1.0 - phat) / total) + (z * z) / (4.0 * total * total))
    return float((center - rad) / denom), float((center + rad) / denom)


def compute_auroc(labels: torch.Tensor, scores: torch.Tensor) -> float:
    """Rank-sum AUROC (eval.py:54-66): ranks 1..n by ascending score, no tie averaging."""
    labels = labels.reshape(-1)
    scores = scores.reshape(-1).to(torch.float64)
    pos = float((labels == 1).sum())
    neg = float((labels == 0).sum())
    if pos == 0 or neg == 0:
        return NAN
    order = torch.argsort(scores, stable=True)
    ranks = torch.empty_like(scores)
    ranks[order] = torch.arange(1, scores.numel() + 1, dtype=torch.float64, device=scores.device)
    pos_rank_sum = float(ranks[labels == 1].sum())
    return float((pos_rank_sum - pos * (pos + 1.0) / 2.0) / (pos * neg))


def compute_ece(probs: torch.Tensor, labels: torch.Tensor, bins: int = 15) -> float:
    """Expected calibration error with equal-width bins (eval.py:69-90): bin i holds
    [i/bins, (i+1)/bins), the last bin is closed."""
    probs = probs.reshape(-1).to(torch.float64)
    labels = labels.reshape(-1).to(torch.float64)
    total = probs.numel()
    if total == 0:
        return NAN
    edges = torch.linspace(0.0, 1.0, bins + 1, dtype=torch.float64, device=probs.device)
    idx = torch.bucketize(probs, edges[1:-1], right=True)  # probs in [e_i, e_{i+1}) -> i
    idx = torch.where(probs >= edges[-1], torch.full_like(idx, bins - 1), idx)
    inside = (probs >= 0.0) & (probs <= 1.0)
    idx, p, lab = idx[inside], probs[inside], labels[inside]
    # one masked reduction per bin: index_add_ on device adds with atomics, in an order that varies
    # from run to run, so the last bits of the result did too
    member = [idx == b for b in range(bins)]
    count = torch.stack([m.sum() for m in member]).to(torch.float64)
    acc = torch.stack([(lab * m).sum() for m in member])
    conf = torch.stack([(p * m).sum() for m in member])
    nz = count > 0
    ece = ((count[nz] / total) * (acc[nz] / count[nz] - conf[nz] / count[nz]).abs()).sum()
    return float(ece)


@torch.no_grad()
def evaluate_vec(model: torch.nn.Module, env_cfg: EnvConfig, episodes: int = 1000, seed: int = 0,
                 num_envs: int = 256, progress_every: int = 0,
                 print_fn: Optional[Callable[[str], None]] = None, reveal_only: bool = False,
                 max_steps_per_episode: int = 512, reveal_fallback_every: int = 0,
                 device: Optional[torch.device] = None, amp_dtype: Optional[torch.dtype] = None,
                 vec: Optional[VecMinesweeper] = None, diagnostics: bool = False,
                 posterior: bool = False, posterior_method: str = "enumerate") -> Dict[str, float]:
    """Greedy (argmax over valid cells) evaluation, reference semantics (eval.py:265-511).

    ``amp_dtype`` None runs the model in fp32 like the reference; torch.bfloat16 uses
    the fused MFMA trunk. ``vec`` may be passed to evaluate on an existing env stream.
    ``diagnostics`` fills the nine avoidability keys (module docstring) instead of NaN;
    ``posterior`` adds the seven exact-posterior keys (module docstring), computed with
    ``posterior_method`` ("enumerate" or "grouped", ms_amd/posterior.py)."""
    if posterior_method not in ("enumerate", "grouped"):
        raise ValueError(f"posterior_method: expected 'enumerate' or 'grouped', got {posterior_method!r}")
    device = device or next(model.parameters()).device
    train_mode = model.training
    model.eval()
    if print_fn is None:
        def print_fn(msg: str):
            print(msg, flush=True)
    if vec is None:
        vec = VecMinesweeper(num_envs, env_cfg, seed=seed, device=device)
    num_envs = vec.num_envs
    batch = vec.reset()
    H, W = env_cfg.H, env_cfg.W
    reveal_count = H * W
    ar = torch.arange(num_envs, device=device)

    remaining = episodes
    processed = 0
    wins = torch.zeros((), dtype=torch.int64, device=device)
    total_steps = torch.zeros((), dtype=torch.int64, device=device)
    total_progress = torch.zeros((), dtype=torch.float64, device=device)
    invalids = torch.zeros((), dtype=torch.int64, device=device)
    belief_p, belief_l = [], []
    diag = _AvoidCounters(num_envs, device) if diagnostics else None
    post = _PosteriorCounters(num_envs, device, posterior_method) if posterior else None
    while remaining > 0:
        batch_size = min(num_envs, remaining)
        counted = torch.zeros(num_envs, dtype=torch.bool, device=device)
        step_counters = torch.zeros(num_envs, dtype=torch.int32, device=device)
        if diag:
            diag.new_batch()
        finished = 0
        tick = 0
        last_reported = 0
        while finished < batch_size:
            obs = batch["obs"]
            mask = batch["action_mask"].clone()
            if reveal_only or (reveal_fallback_every and tick % reveal_fallback_every == 0):
                mask[:, reveal_count:] = False  # the action space is reveal-only: a no-op here
            empty = ~mask.any(dim=1)
            mask[empty] = True
            with torch.autocast("cuda", dtype=amp_dtype or torch.bfloat16, enabled=amp_dtype is not None):
                logits, _, mine_logits = model(obs, return_mine=True)
            logits = logits.float().reshape(num_envs, -1)
            actions = logits.masked_fill(~mask, -1e9).argmax(dim=-1)
            invalids += (~mask[ar, actions]).sum()
            # belief over unknown (= not revealed; flags are never set) cells of the
            # envs whose episode is still being counted, captured before the step
            labels, _ = vec.mine_labels()  # mine_mask (all 0 before the first click)
            unknown = obs[:, 0] == 0
            live = (~counted) & (ar < batch_size)
            sel = unknown & live[:, None, None]
            belief_p.append(torch.sigmoid(mine_logits.float()).reshape(num_envs, H, W)[sel])
            belief_l.append(labels[sel])
            if diag:  # the reference analyses before the step (eval.py:381-398)
                diag.analyse(vec, actions, live, labels.reshape(num_envs, -1)[ar, actions] > 0)
            if post:
                post.analyse(vec, actions, live, unknown.reshape(num_envs, -1),
                             torch.sigmoid(mine_logits.float()).reshape(num_envs, -1))

            batch, _, dones, infos = vec.step(actions)
            t = infos.tensors
            step_counters += 1
            open_ = ~counted
            total_progress += (t["last_new_reveals"].to(torch.float64) * open_).sum() / float(H * W)
            fin = open_ & dones
            wins += (fin & (t["outcome"] == 1)).sum()
            total_steps += (step_counters.to(torch.int64) * fin).sum()
            step_counters = torch.where(fin, torch.zeros_like(step_counters), step_counters)
            counted = counted | fin
            if max_steps_per_episode > 0:
                cut = (~counted) & (step_counters >= max_steps_per_episode)
                total_steps += (step_counters.to(torch.int64) * cut).sum()
                step_counters = torch.where(cut, torch.zeros_like(step_counters), step_counters)
                counted = counted | cut
            if diag or post:
                # one sync for all numbers (the reference counts envs past batch_size too)
                zero = torch.zeros((), dtype=torch.int64, device=device)
                finished, undecided, p_undecided = torch.stack(
                    (counted.sum(), diag.undecided if diag else zero, post.undecided if post else zero)).tolist()
                if diag:
                    diag.finish_step(undecided, fin)
                if post:
                    post.finish_step(p_undecided)
            else:
                finished = int(counted.sum())  # the reference counts envs past batch_size too
            tick += 1
            if progress_every:
                if finished - last_reported >= min(progress_every, batch_size):
                    print_fn(f"eval progress: {processed + finished}/{episodes} episodes")
                    last_reported = finished
                elif tick % 50 == 0:
                    print_fn(f"eval progress: {processed + finished}/{episodes} episodes (running)")
        remaining -= batch_size
        processed += batch_size
        if progress_every and processed % progress_every == 0:
            print_fn(f"eval progress: {processed}/{episodes} episodes")
    if train_mode:
        model.train()

    wins_i = int(wins)
    lo, hi = wilson_interval(wins_i, max(1, episodes))
    if belief_p:
        probs = torch.cat(belief_p)
        labs = torch.cat(belief_l)
        auroc = compute_auroc(labs, probs) if probs.numel() else NAN
        ece = compute_ece(probs, labs) if probs.numel() else NAN
    else:
        auroc = ece = NAN
    ts = int(total_steps)
    out = {
        "win_rate": wins_i / max(1, episodes),
        "win_ci_low": lo,
        "win_ci_high": hi,
        "avg_steps": ts / max(1, episodes),
        "avg_progress": float(total_progress) / max(1, episodes),
        "invalid_rate": int(invalids) / max(1, ts),
        "belief_auroc": auroc,
        "belief_ece": ece,
        "wins": float(wins_i),
        "episodes": float(episodes),
    }
    out.update(diag.metrics(episodes) if diag else {k: NAN for k in _AVOIDABILITY_KEYS})
    if post:
        out.update(post.metrics())
    return out


class _AvoidCounters:
    """Device-side counters behind the nine avoidability keys (eval.py:381-398, 421-422, 469-488)."""
    _NAMES = ("reveal", "comp_n", "comp_cells", "chosen_n", "chosen_sum", "safe_opt", "safe_cells", "hits",
              "forced", "forced_ok", "forced_episodes", "undecided")

    def __init__(self, num_envs: int, device):
        self.c = {k: torch.zeros((), dtype=torch.int64, device=device) for k in self._NAMES}
        self.num_envs, self.device = num_envs, device
        self.max_nodes = torch.zeros((), dtype=torch.int32, device=device)
        self.new_batch()

    def new_batch(self):
        self.ep_unavoidable = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)

    def analyse(self, vec: VecMinesweeper, actions, live, chosen_is_mine):
        self.actions, self.chosen_is_mine = actions, chosen_is_mine
        self.planes = vec.board_planes()  # pre-step copy, read only if some board is undecided
        self.res = vec.avoidability(actions, live=live, resolve=False)
        status = self.res["status"]
        self.undecided = (status == 2).sum()
        self.max_nodes = torch.maximum(self.max_nodes, self.res["max_nodes"].max())
        self._add(status == 1)

    def _add(self, rows):
        r, c = self.res, self.c
        av = r["avoidable"] != 0
        c["reveal"] += rows.sum()
        c["comp_n"] += (r["n_comp"] * rows).sum()
        c["comp_cells"] += (r["n_frontier"] * rows).sum()
        c["chosen_n"] += (rows & (r["chosen_comp"] > 0)).sum()
        c["chosen_sum"] += (r["chosen_comp"] * rows).sum()
        c["safe_opt"] += (rows & av).sum()
        c["safe_cells"] += (r["n_safe"] * (rows & av)).sum()
        c["hits"] += (rows & av & (r["chosen_safe"] != 0)).sum()
        forced = rows & ~av
        c["forced"] += forced.sum()
        c["forced_ok"] += (forced & ~self.chosen_is_mine).sum()
        self.ep_unavoidable |= forced

    def finish_step(self, undecided: int, fin):
        if undecided:
            from .avoid import avoid_host
            rows = torch.nonzero(self.res["status"] == 2).reshape(-1)
            rev, mine = self.planes
            fixed = avoid_host(rev[rows].cpu().numpy(), mine[rows].cpu().numpy(), self.actions[rows].cpu().numpy())
            for k, v in fixed.items():
                self.res[k][rows] = torch.from_numpy(v).to(self.device)
            late = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            late[rows] = True
            self._add(late)
            self.c["undecided"] += undecided
        self.c["forced_episodes"] += (fin & self.ep_unavoidable).sum()

    def metrics(self, episodes: int) -> Dict[str, float]:
        c = {k: int(v) for k, v in self.c.items()}
        ratio = lambda a, b: a / float(b) if b > 0 else NAN  # noqa: E731
        return {
            # not in the reference: boards re-solved on the host, and the device search's largest query
            "avoid_undecided": float(c["undecided"]),
            "avoid_max_nodes": float(int(self.max_nodes)),
            "forced_guess_rate": c["forced"] / float(max(1, c["reveal"])),
            "forced_guess_success_rate": ratio(c["forced_ok"], c["forced"]),
            "forced_guess_episode_rate": c["forced_episodes"] / float(max(1, episodes)),
            "safe_option_rate": c["safe_opt"] / float(max(1, c["reveal"])),
            "safe_option_miss_rate": ratio(c["safe_opt"] - c["hits"], c["safe_opt"]),
            "safe_option_pick_rate": ratio(c["hits"], c["safe_opt"]),
            "avg_safe_options_per_turn": ratio(c["safe_cells"], c["safe_opt"]),
            "avg_frontier_component_size": ratio(c["comp_cells"], c["comp_n"]),
            "avg_selected_component_size": ratio(c["chosen_sum"], c["chosen_n"]),
        }


class _PosteriorCounters:
    """Device-side sums behind the exact-posterior keys of ``evaluate_vec(posterior=True)``."""
    _NAMES = ("cells", "abs_err", "kl", "picks", "chosen_p", "regret", "optimal")

    def __init__(self, num_envs: int, device, method: str = "enumerate"):
        self.c = {k: torch.zeros((), dtype=torch.float64, device=device) for k in self._NAMES}
        self.num_envs, self.device, self.method = num_envs, device, method
        self.max_nodes = torch.zeros((), dtype=torch.int32, device=device)
        self.left_out = 0

    def analyse(self, vec: VecMinesweeper, actions, live, hidden, belief):
        self.actions, self.hidden, self.belief = actions, hidden, belief.to(torch.float64)
        snap = vec.snapshot_tensors()  # pre-step copy, read only if some board is undecided
        self.rev, self.num = snap["revealed"], snap["counts"]
        self.mine_count = vec.cfg.mine_count
        self.res = vec.mine_posterior(live=live, resolve=False, method=self.method)
        status = self.res["status"]
        self.undecided = (status == 2).sum()
        self.max_nodes = torch.maximum(self.max_nodes, self.res["max_nodes"].max())
        self._add(status == 1)

    def _add(self, rows):
        c, p, q, hid = self.c, self.res["prob"], self.belief, self.hidden & rows[:, None]
        c["cells"] += hid.sum()
        c["abs_err"] += ((q - p).abs() * hid).sum()
        qc = q.clamp(1e-6, 1.0 - 1e-6)
        kl = torch.xlogy(p, p / qc) + torch.xlogy(1.0 - p, (1.0 - p) / (1.0 - qc))
        c["kl"] += (kl * hid).sum()
        ar = torch.arange(self.num_envs, device=self.device)
        picked = rows & self.hidden[ar, self.actions]  # a revealed pick (invalid action) has no probability
        pc = p[ar, self.actions]
        pmin = torch.where(self.hidden, p, torch.full_like(p, 2.0)).min(dim=1).values
        c["picks"] += picked.sum()
        c["chosen_p"] += (pc * picked).sum()
        c["regret"] += ((pc - pmin) * picked).sum()
        c["optimal"] += (picked & (pc - pmin <= 1e-9)).sum()

    def finish_step(self, undecided: int):
        if undecided:
            from .posterior import resolve_undecided
            was = self.res["status"] == 2
            resolve_undecided(self.res, self.rev, self.num, self.mine_count, method=self.method)
            self._add(was & (self.res["status"] == 1))
            self.left_out += int((self.res["status"] == 2).sum())
            self.max_nodes = torch.maximum(self.max_nodes, self.res["max_nodes"].max())

    def metrics(self) -> Dict[str, float]:
        c = {k: float(v) for k, v in self.c.items()}
        ratio = lambda a, b: a / b if b > 0 else NAN  # noqa: E731
        return {
            "belief_posterior_mae": ratio(c["abs_err"], c["cells"]),
            "belief_posterior_kl": ratio(c["kl"], c["cells"]),
            "chosen_mine_prob": ratio(c["chosen_p"], c["picks"]),
            "guess_regret": ratio(c["regret"], c["picks"]),
            "optimal_pick_rate": ratio(c["optimal"], c["picks"]),
            "posterior_undecided": float(self.left_out),
            "posterior_max_nodes": float(int(self.max_nodes)),
        }


def main(argv=None) -> None:
    """CLI with the reference's flags (eval.py:526-536)."""
    import yaml

    from .models import build_model, strip_compile_prefix
    ap = argparse.ArgumentParser(description="Evaluate a Minesweeper RL checkpoint on device")
    ap.add_argument("--run_dir", type=str, default=None)
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--model", type=str, default=None)
    ap.add_argument("--num_envs", type=int, default=128)
    ap.add_argument("--progress", action="store_true")
    ap.add_argument("--reveal_only", action="store_true")
    ap.add_argument("--debug_eval", action="store_true", help="accepted; not implemented on device")
    ap.add_argument("--amp", choices=["fp32", "bf16", "fp16"], default="fp32")
    ap.add_argument("--diagnostics", action="store_true",
                    help="fill the avoidability metrics (forced_guess_*, safe_option_*, component sizes) on device")
    ap.add_argument("--posterior", action="store_true",
                    help="score beliefs and moves against the exact posterior mine probability on device")
    ap.add_argument("--posterior_method", choices=["enumerate", "grouped"], default="enumerate",
                    help="counting of the exact posterior: one node per cell value, or per group of equivalent cells")
    ap.add_argument("--symmetry", action="store_true",
                    help="average the model's logits over the board's mirror images and rotations "
                         "(ms_amd.symmetry.SymmetricModel)")
    ap.add_argument("--player", choices=["checkpoint", "posterior", "lookahead"], default="checkpoint",
                    help="who plays: a checkpoint's model, the greedy exact-posterior player, or that player "
                         "with the two-guess lookahead (the last two need no --ckpt; --posterior_method is their counting)")
    ap.add_argument("--lookahead", type=int, default=8, help="candidates per forced guess of --player lookahead")
    ap.add_argument("--lookahead_margin", type=float, default=0.1,
                    help="candidates lie within this of the least mine probability")
    args = ap.parse_args(argv)
    from . import exact_fp32_convs
    exact_fp32_convs()
    device = torch.device("cuda")
    if args.player != "checkpoint":
        ckpt = None
    elif args.ckpt:
        ckpt = args.ckpt
    else:
        if not args.run_dir:
            raise SystemExit("Provide either --ckpt or --run_dir")
        import glob
        import re
        paths = glob.glob(os.path.join(args.run_dir, "ckpt_*.pt"))
        if not paths:
            raise FileNotFoundError(f"No checkpoints found in {args.run_dir}")
        num = lambda p: int(m.group(1)) if (m := re.search(r"ckpt_(\d+)\.pt$", os.path.basename(p))) else -1  # noqa: E731
        ckpt = max(paths, key=num)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    env_d = dict(cfg["env"] if "env" in cfg else cfg)
    env_d.pop("include_frontier_channel", None)
    env_cfg = EnvConfig(**env_d)
    if ckpt is None:
        from .posterior import PosteriorModel
        name = args.player
        model = PosteriorModel(env_cfg.mine_count, method=args.posterior_method,
                               lookahead=args.lookahead if args.player == "lookahead" else 0,
                               margin=args.lookahead_margin).to(device)
    else:
        state = torch.load(ckpt, map_location=device, weights_only=True)
        meta = state.get("model_meta", {}) if isinstance(state, dict) else {}
        mcfg = dict((meta or {}).get("config", {}))
        mcfg.pop("name", None)
        name = args.model or (meta or {}).get("name", "cnn")
        model = build_model(name, obs_shape=(10, env_cfg.H, env_cfg.W), model_cfg=mcfg).to(device)
        sd = strip_compile_prefix(dict(state["model"]) if isinstance(state, dict) and "model" in state else state)
        ms = model.state_dict()
        model.load_state_dict({k: v for k, v in sd.items() if k in ms and ms[k].shape == v.shape}, strict=False)
    if args.symmetry:
        from .symmetry import SymmetricModel
        model = SymmetricModel(model)
    metrics = evaluate_vec(model, env_cfg, episodes=args.episodes, seed=0,
                           num_envs=min(args.num_envs, args.episodes),
                           progress_every=(max(1, args.episodes // 4) if args.progress else 0),
                           reveal_only=args.reveal_only, diagnostics=args.diagnostics, posterior=args.posterior,
                           posterior_method=args.posterior_method,
                           amp_dtype={"bf16": torch.bfloat16, "fp16": torch.float16}.get(args.amp))
    summary = {"checkpoint": os.path.basename(ckpt) if ckpt else None, "model": name, **metrics}
    if args.player == "lookahead":
        summary.update({f"lookahead_{k}": v for k, v in model.lookahead_counters().items()})
    for k, v in summary.items():
        print(f"{k}: {v:.3f}" if isinstance(v, float) and np.isfinite(v) else f"{k}: {v}")


if __name__ == "__main__":
    main()
