"""Measurements of the imitation warm start:

  python tools/imitation_ab.py kernels [--rows 32768 --cells 256 --out DIR]
      k_expert and the two passes of the behaviour-cloning loss (csrc/msexpert.hip, csrc/msbc.hip)
      against the PyTorch-op restatement of the same loss in f32 on the same device: each variant
      warmed up, then the variants alternated twice, HIP events around 50 calls each.

  python tools/imitation_ab.py collect [--envs 4096 --steps 64 --out DIR]
      collect_expert at 16x16x40, grouped counting, budgets 2^10 and 2^12, alternated twice after a
      warm-up of each: seconds per collect (host clock around a device synchronise), kind shares.

  python tools/imitation_ab.py pretrain [--iters N --work DIR --out DIR]
      pretrain_il.py on configs/imitation/16x16x40_medium.yaml, seed 0, then evaluate_vec of
      ckpt_final.pt (2,048 episodes, fp32).

  python tools/imitation_ab.py train [--updates 500 --work DIR --out DIR]
      train_rl.py on configs/training/16x16x40_medium.yaml, seed 0, no quick evals: once from
      WORK/il/ckpt_final.pt (--init_ckpt) and once cold; each final checkpoint evaluated as above.

Each line printed is one JSON object; --out also keeps them in DIR/imitation_<what>.jsonl."""
from __future__ import annotations

import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minesweeper-ppo_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MEDIUM = os.path.join(ROOT, "configs", "training", "16x16x40_medium.yaml")
IMITATION = os.path.join(ROOT, "configs", "imitation", "16x16x40_medium.yaml")


def _emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def _torch_loss(lg, mi, mask, best, w, labels, valid, counts, ent_coef, aw, cw):
    """include/msbc.h as PyTorch ops in f32 (what the HIP passes replace)."""
    x = lg.masked_fill(~mask, -1e9)
    lp = F.log_softmax(x, -1)
    bf = best.to(lp.dtype)
    ce_row = -(lp * bf).sum(1) / bf.sum(1)
    ent_row = -(lp.exp() * lp).sum(1)
    agree_row = best.gather(1, x.argmax(1, keepdim=True)).squeeze(1).to(lp.dtype)
    norm = 1.0 / counts[0]
    ce, agree, ent = (w * ce_row).sum() * norm, (w * agree_row).sum() * norm, (w * ent_row).sum() * norm
    vm = valid.to(lp.dtype)
    pos, cnt = counts[1], counts[2]
    pw = (cnt - pos + 1e-6) / (pos + 1e-6)
    scale = 1.0 / cnt.clamp_min(1.0)
    bce = (F.binary_cross_entropy_with_logits(mi, labels, pos_weight=pw, reduction="none") * vm).sum() * scale
    cal = ((torch.sigmoid(mi) - labels).pow(2) * vm).sum() * scale
    return torch.stack([ce, agree.detach(), ent, bce, cal, ce - ent_coef * ent + aw * bce + cw * cal])


def kernels(args, fh):
    from ms_amd import _lib as L
    from ms_amd.bc_loss import bc_loss_terms
    dev = torch.device("cuda", 0)
    lib = L.load()
    M, A = args.rows, args.cells
    g = torch.Generator(device="cpu").manual_seed(0)
    lg = (torch.randn(M, A, generator=g) * 3).to(dev)
    mi = (torch.randn(M, A, generator=g) * 2).to(dev)
    mask = (torch.rand(M, A, generator=g) < 0.7).to(dev)
    mask[:, 0] = True
    prob = torch.rand(M, A, generator=g, dtype=torch.float64)
    prob[torch.rand(M, A, generator=g) < 0.1] = 0.0
    prob = prob.to(dev)
    status = torch.ones(M, dtype=torch.uint8, device=dev)
    ex = {k: torch.empty((M, A) if cells else (M,), dtype=getattr(torch, dt), device=dev)
          for k, dt, cells in L.EXPERT_OUTPUTS}

    def expert():
        L.check(lib.ms_expert_targets(L.ptr(status), L.ptr(prob), L.ptr(mask), M, A,
                                      *(L.ptr(ex[k]) for k, _, _ in L.EXPERT_OUTPUTS), L.stream_ptr(dev)))
    expert()
    best, labels = ex["best"].bool(), ex["labels"]
    w = torch.where(ex["kind"] == 1, 1.0, 0.5).to(dev)
    valid = mask.clone()
    counts = torch.stack([w.sum(), (labels * valid).sum(), valid.float().sum()])
    kw = dict(ent_coef=0.01, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
    # the HIP passes through their C entry points, on preallocated buffers
    a = L.McBcLossArgs()
    keep = [mask.contiguous(), ex["best"], w, labels, valid, counts]
    a.action_mask, a.best, a.weight, a.labels, a.valid, a.counts = [L.ptr(t) for t in keep]
    a.logits, a.mine = L.ptr(lg), L.ptr(mi)
    a.mask_fill, a.ent_coef, a.aux_mine_weight, a.aux_mine_calib_weight = -1e9, 0.01, 0.05, 0.01
    a.world, a.M, a.A = 1.0, M, A
    out, gout = torch.empty(8, device=dev), torch.ones(8, device=dev)
    nws = int(lib.mc_bc_loss_workspace(M))
    work = torch.empty(nws, device=dev)
    dl, dm = torch.empty_like(lg), torch.empty_like(mi)

    def hip_fwd():
        L.check_mc(lib.mc_bc_loss_fwd(ctypes.byref(a), L.ptr(out), L.ptr(work), nws, L.stream_ptr(dev)))

    def hip_bwd():
        L.check_mc(lib.mc_bc_loss_bwd(ctypes.byref(a), L.ptr(gout), L.ptr(work), nws, L.ptr(dl), L.ptr(dm),
                                      L.stream_ptr(dev)))
    lgr, mir = lg.clone().requires_grad_(True), mi.clone().requires_grad_(True)

    def hip_autograd():
        lgr.grad = mir.grad = None
        bc_loss_terms(lgr, mir, mask, ex["best"], w, labels=labels, valid=valid, counts=counts, **kw)[5].backward()

    def torch_fwd():
        with torch.no_grad():
            _torch_loss(lg, mi, mask, best, w, labels, valid, counts, 0.01, 0.05, 0.01)

    def torch_fwd_bwd():
        lgr.grad = mir.grad = None
        _torch_loss(lgr, mir, mask, best, w, labels, valid, counts, 0.01, 0.05, 0.01)[5].backward()
    hip_fwd()
    ref = _torch_loss(lg, mi, mask, best, w, labels, valid, counts, 0.01, 0.05, 0.01)
    _emit({"what": "kernels", "check": "terms", "hip": out[:6].tolist(), "torch_ops": ref.tolist()}, fh)
    variants = [("k_expert", expert), ("bc_loss_fwd (k_bc_loss_fwd + k_bc_loss_fin)", hip_fwd),
                ("bc_loss_bwd (k_bc_loss_bwd)", hip_bwd), ("hip fwd + bwd through autograd", hip_autograd),
                ("torch ops fwd", torch_fwd), ("torch ops fwd + bwd", torch_fwd_bwd)]

    def timed(fn, n=50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1000.0 / n
    for _, fn in variants:
        timed(fn, 10)
    for rep in (1, 2):
        for name, fn in variants:
            _emit({"what": "kernels", "variant": name, "rows": M, "cells": A, "us_per_call": round(timed(fn), 2),
                   "rep": rep}, fh)


def collect(args, fh):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.imitate import collect_expert
    dev = torch.device("cuda", 0)
    vec = VecMinesweeper(args.envs, EnvConfig(H=16, W=16, mine_count=40), seed=0, device=dev)
    bufs = {}

    def run(budget, seed):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        buf = collect_expert(vec, args.steps, budget=budget, method="grouped", explore=0.0, seed=seed,
                             buffer=bufs.get(budget))
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        bufs[budget] = buf
        return {"what": "collect", "budget": budget, "envs": args.envs, "steps": args.steps, "seconds": round(dt, 4),
                "ms_per_step": round(1000 * dt / args.steps, 3), **buf.kind_shares()}
    budgets = (1 << 10, 1 << 12)
    for b in budgets:
        run(b, 0)
    for rep in (1, 2):
        for b in budgets:
            _emit(dict(run(b, rep), rep=rep), fh)


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
    m = evaluate_vec(model, EnvConfig(**ed), episodes=episodes, seed=0, num_envs=min(1024, episodes))
    return {k: m[k] for k in ("win_rate", "win_ci_low", "win_ci_high", "avg_steps", "belief_auroc", "belief_ece")}


def pretrain(args, fh):
    from ms_amd.imitate import main
    out = os.path.join(args.work, "il")
    argv = ["--config", IMITATION, "--seed", "0", "--out", out, "--save_every", "100000"]
    if args.iters is not None:
        argv += ["--iters", str(args.iters)]
    main(argv)
    with open(os.path.join(out, "train_metrics.csv")) as f:
        rows = list(csv.DictReader(f))
    rec = {"what": "pretrain", "iters": len(rows), "seed": 0, "eval_episodes": args.episodes,
           "collect_s_median": round(statistics.median(float(r["collect_s"]) for r in rows), 4),
           "update_s_median": round(statistics.median(float(r["update_s"]) for r in rows), 4)}
    for key in ("agree", "policy_ce", "aux_bce", "aux_calib", "bad_rows", "kind_none", "kind_safe", "kind_guess"):
        rec["first_" + key], rec["last_" + key] = float(rows[0][key]), float(rows[-1][key])
    rec.update(_evaluate(os.path.join(out, "ckpt_final.pt"), args.episodes))
    _emit(rec, fh)


def train(args, fh):
    from ms_amd.train import main
    il = os.path.join(args.work, "il", "ckpt_final.pt")
    for start, extra in (("warm", ["--init_ckpt", il]), ("cold", [])):
        out = os.path.join(args.work, f"rl_{start}")
        main(["--config", MEDIUM, "--seed", "0", "--updates", str(args.updates), "--out", out,
              "--eval_quick_episodes", "0", "--skip_final_eval", "--save_every", "100000"] + extra)
        with open(os.path.join(out, "train_metrics.csv")) as f:
            rows = list(csv.DictReader(f))
        rec = {"what": "train", "start": start, "updates": len(rows), "seed": 0, "eval_episodes": args.episodes,
               "seconds_per_update_median": round(statistics.median(float(r["seconds"]) for r in rows), 4)}
        for key in ("entropy", "policy_loss", "value_loss", "aux_bce"):
            rec["first_" + key], rec["last_" + key] = float(rows[0][key]), float(rows[-1][key])
        rec.update(_evaluate(os.path.join(out, "ckpt_final.pt"), args.episodes))
        _emit(rec, fh)


def main_cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "collect", "pretrain", "train"])
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--updates", type=int, default=500)
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None, help="directory for the .jsonl record")
    ap.add_argument("--work", type=str, default="runs", help="directory for the training runs")
    args = ap.parse_args(argv)
    fh = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fh = open(os.path.join(args.out, f"imitation_{args.what}.jsonl"), "w")
    from ms_amd import exact_fp32_convs
    exact_fp32_convs()
    {"kernels": kernels, "collect": collect, "pretrain": pretrain, "train": train}[args.what](args, fh)


if __name__ == "__main__":
    main_cli()
