"""The two counting methods of the exact posterior, "enumerate" and "grouped" (DESIGN.md section
14), timed against each other in one process on the same boards: each measurement alternates the
two methods twice after a warm-up of each.

  python tools/posterior_grouped_ab.py kernel [--envs 4096 --out DIR]
      ms_posterior / ms_posterior_grouped per launch on boards after 15 safe-biased tape steps at
      9x9x10, 16x16x40 and 30x16x99, budgets 2^10, 2^12 and 2^16 (HIP events around one launch).
  python tools/posterior_grouped_ab.py rollout [--envs 4096 --steps 64 --out DIR]
      collect_rollout(belief_targets="posterior") at 16x16x40 with the shipped model.
  python tools/posterior_grouped_ab.py eval [--episodes 4096 --envs 1024 --out DIR]
      evaluate_vec(RuleModel, 16x16x40, posterior=True).

Every line printed is one JSON object with the undecided count (or belief_exact_frac) and the
largest query beside the time; --out appends them to DIR/posterior_grouped_ab.txt."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minesweeper-ppo_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # eval_model.RuleModel

import torch  # noqa: E402

METHODS = ("enumerate", "grouped")
MEDIUM = os.path.join(ROOT, "configs", "training", "16x16x40_medium.yaml")


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def _alternate(run, fh):
    """run(method) -> record; a warm-up of each method, then both alternated twice."""
    for m in METHODS:
        run(m)
    for rep in (1, 2):
        for m in METHODS:
            _emit(dict(run(m), method=m, rep=rep), fh)


def kernel(args, fh):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd import _lib as L
    dev = torch.device("cuda", 0)
    for H, W, K in ((9, 9, 10), (16, 16, 40), (30, 16, 99)):
        vec = VecMinesweeper(args.envs, EnvConfig(H=H, W=W, mine_count=K), seed=0, device=dev)
        vec.reset()
        for t in range(15):
            vec.step(vec.tape_actions(t, L.MS_TAPE_SAFE_BIASED))
        for budget in (1 << 10, 1 << 12, 1 << 16):
            vec.set_posterior_budget(budget)

            def run(method):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                out = vec.mine_posterior(resolve=False, method=method)
                e1.record()
                torch.cuda.synchronize(dev)
                st = out["status"]
                return {"what": "kernel", "board": f"{H}x{W}x{K}", "envs": args.envs, "budget": budget,
                        "ms": round(e0.elapsed_time(e1), 3), "analysed": int((st != 0).sum()),
                        "undecided": int((st == 2).sum()), "max_nodes": int(out["max_nodes"].max())}

            _alternate(run, fh)


def rollout(args, fh):
    from ms_amd.rollout import collect_rollout
    from ms_amd.train import Trainer, load_config
    dev = torch.device("cuda", 0)
    cfg, env_d, model_d, extras = load_config(MEDIUM)
    cfg.num_envs, cfg.steps_per_env = args.envs, args.steps
    extras = dict(extras, training=dict(extras.get("training", {}), rollout={}))
    tr = Trainer(cfg, env_d, model_d, extras, seed=0, amp="fp16", device=dev)
    tr.model.train()
    state = {"buf": None, "k": 0}

    def run(method):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        buf, _ = collect_rollout(tr.vec, tr.model, cfg.steps_per_env, dev, cfg.aux_mine_weight,
                                 cfg.aux_mine_calib_weight, amp_dtype=torch.float16, buffer=state["buf"],
                                 sample_seed=17, sample_counter=state["k"] << 20, obs_codes=True, timing=False,
                                 belief_targets="posterior", posterior_method=method)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        state["buf"], state["k"] = buf, state["k"] + 1
        src = buf.mine_source
        return {"what": "rollout", "envs": args.envs, "steps": args.steps, "seconds": round(dt, 4),
                "boards": int((src != 0).sum()),
                "belief_exact_frac": float((src == 1).sum()) / max(1, int((src != 0).sum()))}

    _alternate(run, fh)


def evaluate(args, fh):
    from eval_model import RuleModel
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    dev = torch.device("cuda", 0)
    model = RuleModel().to(dev)

    def run(method):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        m = evaluate_vec(model, EnvConfig(H=16, W=16, mine_count=40), episodes=args.episodes, seed=0,
                         num_envs=min(args.envs, args.episodes), posterior=True, posterior_method=method)
        torch.cuda.synchronize(dev)
        return {"what": "eval", "episodes": args.episodes, "envs": min(args.envs, args.episodes),
                "seconds": round(time.perf_counter() - t0, 3), "win_rate": m["win_rate"],
                "posterior_undecided": m["posterior_undecided"], "posterior_max_nodes": m["posterior_max_nodes"],
                "guess_regret": m["guess_regret"]}

    _alternate(run, fh)


def main_cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "rollout", "eval"])
    ap.add_argument("--envs", type=int, default=None, help="default 4096 (kernel, rollout), 1024 (eval)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None, help="directory for posterior_grouped_ab.txt")
    args = ap.parse_args(argv)
    if args.envs is None:
        args.envs = 1024 if args.what == "eval" else 4096
    fh = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fh = open(os.path.join(args.out, "posterior_grouped_ab.txt"), "a")
    from ms_amd import exact_fp32_convs
    exact_fp32_convs()
    {"kernel": kernel, "rollout": rollout, "eval": evaluate}[args.what](args, fh)


if __name__ == "__main__":
    main_cli()
