"""Measurements of on-policy imitation:

  python tools/dagger_ab.py kernels [--out DIR]
      ms_dagger_act at 1,024 and 4,096 rows x 256 cells, greedy and sample, against the same step
      as PyTorch ops (sample_masked on zeros, sample_masked or a masked argmax on the logits, two
      rand coins, the where chain and a gather of best): each variant warmed up, then the variants
      alternated twice, HIP events around 50 calls each. Then collect_dagger (the shipped model in
      fp16) against collect_expert per step at 1,024 envs of 16x16x40: what the forward
      costs next to the posterior.

  python tools/dagger_ab.py pretrain --variant NAME [--seconds S | --iters N] [--work DIR --out DIR]
      pretrain_il.py on configs/imitation/16x16x40_medium_sym.yaml, seed 0, fp16, as one of
        sym          as shipped (beta 1 every round: collect_expert)
        dagger       beta 1.0 -> 0.25 over 40 rounds, greedy learner
        dagger_b0    beta 1.0 -> 0.0 over 40 rounds, greedy learner
        dagger_smp   beta 1.0 -> 0.25 over 40 rounds, sampled learner
      held to a wall-time budget (--seconds) or to a number of rounds (--iters), then
      evaluate_vec of ckpt_final.pt (--episodes, fp32; win_ci_* is its Wilson interval).

Each line printed is one JSON object; --out also appends them to DIR/dagger_<what>.jsonl."""
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
SYM = os.path.join(ROOT, "configs", "imitation", "16x16x40_medium_sym.yaml")


def _schedule(end, learner="greedy"):
    return ["--beta_start", "1.0", "--beta_end", str(end), "--beta_decay_iters", "40", "--learner", learner]


VARIANTS = {"sym": [], "dagger": _schedule(0.25), "dagger_b0": _schedule(0.0),
            "dagger_smp": _schedule(0.25, "sample")}


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def _timed(fn, dev, n=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1000.0 / n


def _alternate(variants, dev, fh, n=50, **tags):
    for _, fn in variants:
        _timed(fn, dev, max(2, n // 5))
    for rep in (1, 2):
        for name, fn in variants:
            _emit({"what": "kernels", "variant": name, **tags, "us_per_call": round(_timed(fn, dev, n), 2),
                   "calls": n, "rep": rep}, fh)


def kernels(args, fh):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd import _lib as L
    from ms_amd.dagger import collect_dagger, dagger_act
    from ms_amd.imitate import collect_expert
    from ms_amd.models import build_model
    from ms_amd.rollout import sample_masked
    from ms_amd.train import load_config
    dev = torch.device("cuda", 0)
    lib = L.load()
    A = 256
    gen = torch.Generator(device=dev).manual_seed(0)
    for B in (1024, 4096):
        logits = torch.randn((B, A), device=dev, generator=gen) * 3
        mask = torch.rand((B, A), device=dev, generator=gen) < 0.5
        m8 = mask.view(torch.uint8)
        kind = torch.randint(0, 3, (B,), dtype=torch.uint8, device=dev, generator=gen)
        best = (torch.rand((B, A), device=dev, generator=gen) < 0.1).to(torch.uint8)
        expert = torch.where(kind != 0, torch.randint(0, A, (B,), device=dev, generator=gen), -1)
        tg = {"best": best, "action": expert, "kind": kind}
        zeros = torch.zeros((B, A), device=dev)
        outs = [torch.empty(B, dtype=dt, device=dev) for dt in (torch.int64, torch.uint8, torch.int64, torch.uint8)]
        beta, explore = 0.5, 0.05

        def hip_entry(mode):  # the C entry point on preallocated outputs
            L.check(lib.ms_dagger_act(L.ptr(logits), L.ptr(m8), L.ptr(best), L.ptr(expert), L.ptr(kind), B, A, 0, 1, 2,
                                      beta, explore, mode, *(L.ptr(o) for o in outs), L.stream_ptr(dev)))

        def hip_python(mode):  # through ms_amd.dagger (allocates its outputs)
            return dagger_act(logits, mask, tg, seed=1, counter=2, beta=beta, explore=explore, mode=mode)

        def torch_ops(sample):
            u, _ = sample_masked(zeros, mask, 1, 2)
            if sample:
                l, _ = sample_masked(logits, mask, 3, 2)
            else:
                l = logits.masked_fill(~mask, -1e9).argmax(dim=-1)
            ce = torch.rand(B, device=dev, generator=gen) < explore
            cb = torch.rand(B, device=dev, generator=gen) >= beta
            has = kind != 0
            action = torch.where(ce, u, torch.where(cb, l, torch.where(has, expert, u)))
            source = torch.where(ce, 0, torch.where(cb, 2, has.to(torch.int64))).to(torch.uint8)
            agree = (best.gather(1, l[:, None])[:, 0] != 0) & has
            return action, source, l, agree.to(torch.uint8)

        # the same learner move and agreement as the op form (the coins are torch's there, so the
        # mixed action is not comparable); the full rule is checked by tests/test_dagger_act_gpu.py
        g = hip_python("greedy")
        ref = torch_ops(False)
        _emit({"what": "kernels", "check": "greedy learner_action, agree == torch ops", "rows": B,
               "equal": bool(torch.equal(g["learner_action"], ref[2]) and torch.equal(g["agree"], ref[3]))}, fh)
        _alternate([("ms_dagger_act greedy (C entry, preallocated)", lambda: hip_entry(0)),
                    ("ms_dagger_act sample (C entry, preallocated)", lambda: hip_entry(1)),
                    ("ms_dagger_act greedy (ms_amd.dagger.dagger_act)", lambda: hip_python("greedy")),
                    ("ms_dagger_act sample (ms_amd.dagger.dagger_act)", lambda: hip_python("sample")),
                    ("torch ops greedy: sample_masked + argmax + 2 rand + where chain + gather", lambda: torch_ops(False)),
                    ("torch ops sample: 2 sample_masked + 2 rand + where chain + gather", lambda: torch_ops(True))],
                   dev, fh, rows=B, cells=A)
    # the collectors, per step, at the shipped size
    cfg, env_d, _, _ = load_config(MEDIUM)
    _, _, model_d, _ = load_config(SYM)
    ed = dict(env_d)
    ed.pop("include_frontier_channel", None)
    N, T = 1024, 16
    torch.manual_seed(0)
    model = build_model(model_d["name"], obs_shape=(10, cfg.H, cfg.W), model_cfg=dict(model_d)).to(dev)
    state = {}

    def run(beta):  # every call continues the same games
        if "vec" not in state:
            state["vec"] = VecMinesweeper(N, EnvConfig(**ed), seed=0, device=dev)
            state["buf"] = collect_expert(state["vec"], T, budget=4096, seed=0)
        if beta is None:
            state["buf"] = collect_expert(state["vec"], T, budget=4096, explore=0.05, seed=1, buffer=state["buf"],
                                          reset=False)
        else:
            state["buf"] = collect_dagger(state["vec"], model, T, beta=beta, budget=4096, explore=0.05,
                                          amp=torch.float16, seed=1, buffer=state["buf"], reset=False)

    # beta 0.999: the forward runs every step but the teacher still plays nearly every move, so the
    # boards (and with them the posterior's cost) are those of the other two variants
    variants = [("collect_expert", lambda: run(None)), ("collect_dagger beta 1 (no forward)", lambda: run(1.0)),
                ("collect_dagger beta 0.999 (fp16 forward every step)", lambda: run(0.999))]
    for _, fn in variants:
        _timed(fn, dev, 2)
    for rep in (1, 2):
        for name, fn in variants:
            us = _timed(fn, dev, 4)
            _emit({"what": "collect", "variant": name, "envs": N, "steps_per_call": T, "calls": 4,
                   "us_per_step": round(us / T, 1), "rep": rep}, fh)


def _evaluate(ckpt, episodes):
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.models import build_model
    from ms_amd.train import load_config
    dev = torch.device("cuda", 0)
    cfg, env_d, _, _ = load_config(MEDIUM)
    state = torch.load(ckpt, map_location=dev, weights_only=True)
    model = build_model(state["model_meta"]["name"], obs_shape=(10, cfg.H, cfg.W),
                        model_cfg=dict(state["model_meta"]["config"])).to(dev)
    model.load_state_dict(state["model"])
    model.eval()
    ed = dict(env_d)
    ed.pop("include_frontier_channel", None)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    m = evaluate_vec(model, EnvConfig(**ed), episodes=episodes, seed=0, num_envs=min(1024, episodes))
    out = {k: m[k] for k in ("win_rate", "win_ci_low", "win_ci_high", "avg_steps", "belief_auroc", "belief_ece")}
    out["eval_seconds"] = round(time.perf_counter() - t0, 2)
    return out


def pretrain(args, fh):
    from ms_amd.imitate import main
    held = "seconds" if args.seconds is not None else "rounds"
    out = os.path.join(args.work, f"il_{args.variant}_{held}")
    argv = ["--config", SYM, "--seed", "0", "--amp", "fp16", "--out", out, "--save_every", "100000"]
    argv += VARIANTS[args.variant]
    if args.iters is not None:
        argv += ["--iters", str(args.iters)]
    if args.seconds is not None:
        argv += ["--max_seconds", str(args.seconds)]
    t0 = time.perf_counter()
    main(argv)
    wall = time.perf_counter() - t0
    with open(os.path.join(out, "train_metrics.csv")) as f:
        rows = list(csv.DictReader(f))
    on_policy = [(int(r["iter"]), float(r["on_policy_agree"])) for r in rows if r["on_policy_agree"] not in ("", "nan")]
    rec = {"what": "pretrain", "variant": args.variant, "held_to": held, "rounds": len(rows), "seed": 0,
           "train_seconds": round(wall, 1),
           "collect_s_median": round(statistics.median(float(r["collect_s"]) for r in rows), 4),
           "update_s_median": round(statistics.median(float(r["update_s"]) for r in rows), 4),
           "last_agree": float(rows[-1]["agree"]), "last_policy_ce": float(rows[-1]["policy_ce"]),
           "last_beta": float(rows[-1]["beta"]), "last_share_learner": float(rows[-1]["share_learner"]),
           "on_policy_agree_first": on_policy[0] if on_policy else None,
           "on_policy_agree_last": on_policy[-1] if on_policy else None,
           "bad_rows": sum(float(r["bad_rows"]) for r in rows)}
    _emit(rec, fh)
    _emit({"what": "eval", "variant": args.variant, "held_to": held, "rounds": len(rows), "episodes": args.episodes,
           **_evaluate(os.path.join(out, "ckpt_final.pt"), args.episodes)}, fh)


def main_cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "pretrain"])
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="sym")
    ap.add_argument("--seconds", type=float, default=None, help="wall-time budget of the training loop")
    ap.add_argument("--iters", type=int, default=None, help="collect + update rounds")
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None, help="directory for the .jsonl record")
    ap.add_argument("--work", type=str, default="runs", help="directory for the training runs")
    args = ap.parse_args(argv)
    fh = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fh = open(os.path.join(args.out, f"dagger_{args.what}.jsonl"), "a")
    from ms_amd import exact_fp32_convs
    exact_fp32_convs()
    {"kernels": kernels, "pretrain": pretrain}[args.what](args, fh)


if __name__ == "__main__":
    main_cli()
