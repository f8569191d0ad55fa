"""Measurements of the board symmetries:

  python tools/symmetry_ab.py kernels [--out DIR]
      ms_sym_gather at 4,096 and 32,768 rows x 256 cells against the same work as PyTorch ops (an
      index per plane, then a gather through a precomputed [B, A] cell map), and ms_sym_expand +
      ms_sym_mean at 1,024 x 256 against flip / transpose ops: each variant warmed up, then the
      variants alternated twice, HIP events around 50 calls each; bytes moved per second.

  python tools/symmetry_ab.py pretrain --variant NAME [--seconds S | --iters N] [--work DIR --out DIR]
      pretrain_il.py on configs/imitation/16x16x40_medium.yaml, seed 0, fp16, as one of
        shipped      epochs 1, no augmentation
        aug_e1       augment, epochs 1
        aug_e4       augment, epochs 4
        plain_e4     epochs 4, no augmentation (the control for extra passes alone)
      held to a wall-time budget (--seconds) or to a number of rounds (--iters), then
      evaluate_vec of ckpt_final.pt (--episodes, fp32) without and with SymmetricModel.

Each line printed is one JSON object; --out also appends them to DIR/symmetry_<what>.jsonl."""
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
IMITATION = os.path.join(ROOT, "configs", "imitation", "16x16x40_medium.yaml")
VARIANTS = {"shipped": [], "aug_e1": ["--augment", "--epochs", "1"], "aug_e4": ["--augment", "--epochs", "4"],
            "plain_e4": ["--epochs", "4"]}


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


def _alternate(variants, dev, fh, **tags):
    for _, fn, _ in variants:
        _timed(fn, dev, 10)
    for rep in (1, 2):
        for name, fn, nbytes in variants:
            us = _timed(fn, dev)
            _emit({"what": "kernels", "variant": name, **tags, "us_per_call": round(us, 2),
                   "GB_per_s": round(nbytes / us / 1e3, 1), "rep": rep}, fh)


def kernels(args, fh):
    from ms_amd import _lib as L
    from ms_amd.symmetry import PLANES, cell_map, sym_expand, sym_gather, sym_mean
    dev = torch.device("cuda", 0)
    lib = L.load()
    H = W = 16
    A, G = H * W, 8
    gen = torch.Generator(device=dev).manual_seed(0)
    maps = torch.stack([torch.from_numpy(cell_map(H, W, g)).to(dev).long() for g in range(G)])  # [G, A]
    for B in (4096, 32768):
        src = dict(codes=torch.randint(0, 10, (B, H, W), dtype=torch.uint8, device=dev, generator=gen),
                   mask=torch.rand((B, A), device=dev, generator=gen) < 0.5,
                   best=torch.randint(0, 2, (B, A), dtype=torch.uint8, device=dev, generator=gen),
                   labels=torch.rand((B, A), device=dev, generator=gen),
                   kind=torch.randint(0, 3, (B,), dtype=torch.uint8, device=dev, generator=gen))
        rows = torch.randperm(B, device=dev, generator=gen)
        g = torch.randint(0, G, (B,), dtype=torch.uint8, device=dev, generator=gen)
        out = {k: torch.empty_like(v) for k, v in src.items()}
        ins = [src[k] for k in PLANES]
        outs = [out[k] for k in PLANES]

        def hip_entry():  # the C entry point on preallocated outputs
            L.check(lib.ms_sym_gather(L.ptr(rows), L.ptr(g), B, H, W, B, *(L.ptr(t) for t in ins),
                                      *(L.ptr(t) for t in outs), None, L.stream_ptr(dev)))

        def hip_python():  # through ms_amd.symmetry (allocates its outputs, as ExpertBuffer.gather does)
            sym_gather(rows, g, H, W, **src)

        def torch_ops():  # an index per plane, then a gather through the [B, A] map of each row's g
            idx = maps[g.long()]
            d = {k: src[k][rows] for k in PLANES}
            return {k: (d[k] if k == "kind" else torch.gather(d[k].reshape(B, A), 1, idx)) for k in PLANES}

        def torch_index_only():  # ExpertBuffer.gather without a symmetry: the five index ops alone
            return {k: src[k][rows] for k in PLANES}
        ref = torch_ops()
        hip_entry()
        same = all(torch.equal(out[k].reshape(B, -1), ref[k].reshape(B, -1)) for k in PLANES)
        _emit({"what": "kernels", "check": "gather == torch ops", "rows": B, "equal": same}, fh)
        moved = 2 * B * (3 * A + 4 * A + 1) + B * 9  # every plane read and written once; rows and g
        _alternate([("ms_sym_gather (C entry, preallocated)", hip_entry, moved),
                    ("ms_sym_gather (ms_amd.symmetry.sym_gather)", hip_python, moved),
                    ("torch ops: 5 index + map lookup + 4 gather", torch_ops, moved),
                    ("torch ops: 5 index, no symmetry", torch_index_only, moved)], dev, fh, rows=B, cells=A)
    n = 1024
    codes = torch.randint(0, 10, (n, H, W), dtype=torch.uint8, device=dev, generator=gen)
    x = torch.randn((G, n, A), device=dev, generator=gen)

    def t(v, gg):
        if gg & 4:
            v = v.transpose(-1, -2)
        if gg & 1:
            v = v.flip(-2)
        if gg & 2:
            v = v.flip(-1)
        return v
    inv = [gg if gg < 4 else 4 | ((gg & 1) << 1) | ((gg >> 1) & 1) for gg in range(G)]

    def torch_expand():
        return torch.stack([t(codes, gg) for gg in range(G)])

    def torch_mean():
        y = [t(x[gg].view(n, H, W), inv[gg]) for gg in range(G)]
        return ((((y[0] + y[1]) + (y[2] + y[3])) + ((y[4] + y[5]) + (y[6] + y[7]))) * 0.125).reshape(n, A)
    same = torch.equal(sym_expand(codes), torch_expand()) and torch.equal(sym_mean(x, H, W), torch_mean())
    _emit({"what": "kernels", "check": "expand, mean == torch ops", "rows": n, "equal": same}, fh)
    _alternate([("ms_sym_expand", lambda: sym_expand(codes), n * A * (1 + G)),
                ("ms_sym_mean", lambda: sym_mean(x, H, W), n * A * 4 * (G + 1)),
                ("torch ops expand (flip / transpose / stack)", torch_expand, n * A * (1 + G)),
                ("torch ops mean (flip / transpose / 7 adds / mul)", torch_mean, n * A * 4 * (G + 1))],
               dev, fh, rows=n, cells=A, G=G)


def _evaluate(ckpt, episodes, symmetry):
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.models import build_model
    from ms_amd.symmetry import SymmetricModel
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
    m = evaluate_vec(SymmetricModel(model) if symmetry else model, EnvConfig(**ed), episodes=episodes, seed=0,
                     num_envs=min(1024, episodes))
    out = {k: m[k] for k in ("win_rate", "win_ci_low", "win_ci_high", "avg_steps", "belief_auroc", "belief_ece")}
    out["eval_seconds"] = round(time.perf_counter() - t0, 2)
    return out


def pretrain(args, fh):
    from ms_amd.imitate import main
    out = os.path.join(args.work, "il_" + args.variant)
    argv = ["--config", IMITATION, "--seed", "0", "--amp", "fp16", "--out", out, "--save_every", "100000"]
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
    rec = {"what": "pretrain", "variant": args.variant, "held_to": "seconds" if args.seconds is not None else "rounds",
           "rounds": len(rows), "seed": 0, "train_seconds": round(wall, 1),
           "collect_s_median": round(statistics.median(float(r["collect_s"]) for r in rows), 4),
           "update_s_median": round(statistics.median(float(r["update_s"]) for r in rows), 4),
           "last_agree": float(rows[-1]["agree"]), "last_policy_ce": float(rows[-1]["policy_ce"]),
           "bad_rows": sum(float(r["bad_rows"]) for r in rows)}
    _emit(rec, fh)
    ckpt = os.path.join(out, "ckpt_final.pt")
    for symmetry in (False, True):
        _emit({"what": "eval", "variant": args.variant, "held_to": rec["held_to"], "rounds": len(rows),
               "symmetry": symmetry, "episodes": args.episodes, **_evaluate(ckpt, args.episodes, symmetry)}, fh)


def main_cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "pretrain"])
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="shipped")
    ap.add_argument("--seconds", type=float, default=None, help="wall-time budget of the training loop")
    ap.add_argument("--iters", type=int, default=None, help="collect + update rounds")
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None, help="directory for the .jsonl record")
    ap.add_argument("--work", type=str, default="runs", help="directory for the training runs")
    args = ap.parse_args(argv)
    fh = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        fh = open(os.path.join(args.out, f"symmetry_{args.what}.jsonl"), "a")
    from ms_amd import exact_fp32_convs
    exact_fp32_convs()
    {"kernels": kernels, "pretrain": pretrain}[args.what](args, fh)


if __name__ == "__main__":
    main_cli()
