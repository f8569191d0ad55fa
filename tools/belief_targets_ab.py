"""Hard 0 / 1 belief targets against the exact posterior, two measurements:

  python tools/belief_targets_ab.py rollout [--envs 4096 --steps 64 --out DIR]
      collect_rollout at 16x16x40 with the shipped model: hard, then posterior at budgets 2^10,
      2^11 and 2^12, the four alternated twice in one process after a warm-up of each. Prints
      seconds per rollout (host clock around a device synchronise) and the exact fraction.

  python tools/belief_targets_ab.py train [--updates 500 --episodes 2048 --out DIR]
      the shipped medium config, seed 0, once per mode; each final checkpoint scored with
      evaluate_vec(posterior=True). Prints win rate, belief_ece, belief_auroc,
      belief_posterior_mae, seconds per update (median) and the mean exact fraction.

Each line printed is one JSON object; --out also keeps them in DIR/belief_targets_<what>.jsonl."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minesweeper-ppo_amd"))

import torch  # noqa: E402

MEDIUM = os.path.join(ROOT, "configs", "training", "16x16x40_medium.yaml")


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def rollout(args, fh):
    from ms_amd.rollout import collect_rollout
    from ms_amd.train import Trainer, load_config
    dev = torch.device("cuda", 0)
    cfg, env_d, model_d, extras = load_config(MEDIUM)
    cfg.num_envs, cfg.steps_per_env = args.envs, args.steps
    extras = dict(extras, training=dict(extras.get("training", {}), rollout={}))
    tr = Trainer(cfg, env_d, model_d, extras, seed=0, amp="fp16", device=dev)
    tr.model.train()
    variants = [("hard", None)] + [("posterior", 1 << b) for b in (10, 11, 12)]
    bufs = {}

    def run(mode, budget, counter):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        buf, _ = collect_rollout(tr.vec, tr.model, cfg.steps_per_env, dev, cfg.aux_mine_weight,
                                 cfg.aux_mine_calib_weight, amp_dtype=torch.float16, buffer=bufs.get(mode),
                                 sample_seed=17, sample_counter=counter << 20, obs_codes=True, timing=False,
                                 belief_targets=mode, posterior_budget=budget)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        bufs[mode] = buf
        rec = {"what": "rollout", "targets": mode, "budget": budget, "envs": args.envs, "steps": args.steps,
               "seconds": round(dt, 4)}
        if buf.mine_source is not None:
            src = buf.mine_source
            rec["belief_exact_frac"] = float((src == 1).sum()) / max(1, int((src != 0).sum()))
            rec["boards"] = int((src != 0).sum())
        return rec

    k = 0
    for mode, budget in variants:  # warm-up: every shape and kernel once
        run(mode, budget, k)
        k += 1
    for rep in (1, 2):
        for mode, budget in variants:
            _emit(dict(run(mode, budget, k), rep=rep), fh)
            k += 1


def train(args, fh):
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.models import build_model
    from ms_amd.train import load_config, main
    dev = torch.device("cuda", 0)
    cfg, env_d, _, _ = load_config(MEDIUM)
    for mode in ("hard", "posterior"):
        out = os.path.join(args.work, f"belief_{mode}")
        main(["--config", MEDIUM, "--seed", "0", "--updates", str(args.updates), "--out", out,
              "--belief_targets", mode, "--eval_quick_episodes", "0", "--skip_final_eval", "--save_every", "100000"])
        with open(os.path.join(out, "train_metrics.csv")) as f:
            rows = list(csv.DictReader(f))
        state = torch.load(os.path.join(out, "ckpt_final.pt"), map_location=dev, weights_only=True)
        mcfg = dict(state["model_meta"]["config"])
        model = build_model(state["model_meta"]["name"], obs_shape=(10, cfg.H, cfg.W), model_cfg=mcfg).to(dev)
        model.load_state_dict(state["model"])
        model.eval()
        ed = dict(env_d)
        ed.pop("include_frontier_channel", None)
        m = evaluate_vec(model, EnvConfig(**ed), episodes=args.episodes, seed=0, num_envs=min(1024, args.episodes),
                         posterior=True)
        rec = {"what": "train", "targets": mode, "updates": len(rows), "seed": 0, "eval_episodes": args.episodes,
               "seconds_per_update_median": round(statistics.median(float(r["seconds"]) for r in rows), 4)}
        if "belief_exact_frac" in rows[0]:
            rec["belief_exact_frac_mean"] = statistics.fmean(float(r["belief_exact_frac"]) for r in rows)
        for key in ("win_rate", "win_ci_low", "win_ci_high", "belief_ece", "belief_auroc", "belief_posterior_mae",
                    "belief_posterior_kl", "posterior_undecided"):
            rec[key] = m[key]
        for key in ("aux_bce", "aux_calib"):
            rec["last_" + key] = float(rows[-1][key])
        _emit(rec, fh)


def main_cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["rollout", "train"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--updates", type=int, default=500)
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None, help="directory for the .jsonl record")
    ap.add_argument("--work", type=str, default="runs", help="directory for the training runs")
    args = ap.parse_args(argv)
    fh = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fh = open(os.path.join(args.out, f"belief_targets_{args.what}.jsonl"), "w")
    from ms_amd import exact_fp32_convs
    exact_fp32_convs()
    (rollout if args.what == "rollout" else train)(args, fh)


if __name__ == "__main__":
    main_cli()
