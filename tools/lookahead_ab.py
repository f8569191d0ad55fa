"""Measurements of the two-guess lookahead, one JSON line each:

  python tools/lookahead_ab.py kernels [--envs 1024 4096]
      ms_lookahead_expand and ms_lookahead_score on live 16x16x40 boards (K = 8, margin 0.1,
      cap = n) against the same selection and scoring written as PyTorch ops: HIP events around 50
      calls after a warm-up, two alternated repeats.
  python tools/lookahead_ab.py step [--envs 1024]
      what the lookahead adds to a PosteriorModel forward and to a collect_expert step, and the
      workspace at cap = n.
  python tools/lookahead_ab.py winrate --board 16x16x40 --episodes 32768 [--envs 4096]
      evaluate_vec, method "grouped", seed 0: the greedy player against the lookahead player, with
      Wilson intervals and the lookahead's counters.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "minesweeper-ppo_amd"), ROOT]

from ms_amd import EnvConfig, VecMinesweeper  # noqa: E402
from ms_amd import _lib as L  # noqa: E402
from ms_amd.lookahead import lookahead_states, workspace_bytes  # noqa: E402
from ms_amd.posterior import PosteriorModel, posterior_states  # noqa: E402

INF = float("inf")


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def live_boards(n, cfg, dev, steps=30, budget=1 << 12):
    """n boards after ``steps`` moves of the greedy posterior player, with the last obs."""
    vec = VecMinesweeper(n, cfg, seed=0, device=dev)
    batch = vec.reset()
    for t in range(steps):
        tg = vec.expert_targets(budget=budget, hidden=batch["action_mask"])
        batch = vec.step(torch.where(tg["kind"] != 0, tg["action"], vec.tape_actions(t)))[0]
    snap = vec.snapshot_tensors()
    return vec, batch, snap["revealed"].to(torch.uint8), snap["counts"]


def timed(fn, calls=50, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # us per call


def torch_expand(status, prob, rev, num, K, margin):
    """The selection and the board expansion as PyTorch ops (dense: slot = board)."""
    n, A = prob.shape
    hid = (rev.reshape(n, A) == 0) & (status == 1)[:, None]
    pm = torch.where(hid, prob, torch.full_like(prob, INF)).min(dim=1).values
    guess = (pm > 0) & (pm < INF)
    key = torch.where(hid & (prob <= (pm + margin)[:, None]) & guess[:, None], prob, torch.full_like(prob, INF))
    val, idx = torch.sort(key, dim=1, stable=True)
    cand = torch.where(val[:, :K] < INF, idx[:, :K], torch.full_like(idx[:, :K], -1))
    at = cand.clamp_min(0)[:, :, None, None].expand(n, K, 9, 1)
    rev2 = rev.reshape(n, 1, 1, A).expand(n, K, 9, A).clone().scatter_(3, at, 1)
    v = torch.arange(9, dtype=torch.uint8, device=prob.device).reshape(1, 1, 9, 1).expand(n, K, 9, 1)
    num2 = num.reshape(n, 1, 1, A).expand(n, K, 9, A).clone().scatter_(3, at, v)
    live2 = (cand >= 0)[:, :, None].expand(n, K, 9).contiguous().to(torch.uint8)
    return guess, cand, rev2, num2, live2


def torch_score(cand, prob, configs, status2, prob2, configs2, rev2, M):
    """The scoring rule as PyTorch ops on dense [n, K, 9] outcome rows."""
    n, K = cand.shape
    A = prob.shape[1]
    hid2 = rev2.reshape(n, K, 9, A) == 0
    p2 = torch.where(hid2, prob2.reshape(n, K, 9, A), torch.full_like(prob2.reshape(n, K, 9, A), INF))
    pm = p2.min(dim=3).values
    t = torch.where((hid2.sum(dim=3) == M) | (pm == 0), torch.ones_like(pm), 1.0 - pm)
    ok = status2.reshape(n, K, 9) == 1
    z = torch.where(ok, configs2.reshape(n, K, 9), torch.zeros_like(pm))
    sum_zt = (z * torch.where(ok, t, torch.zeros_like(t))).sum(dim=2)
    want = configs[:, None] * (1.0 - prob.gather(1, cand.clamp_min(0)))
    scored = ((z.sum(dim=2) - want).abs() <= 1e-9 * want) & (cand >= 0)
    score = torch.where(scored, sum_zt / configs[:, None], torch.full_like(sum_zt, -INF))
    best = score.argmax(dim=1)
    return torch.where(scored.any(dim=1), cand.gather(1, best[:, None])[:, 0], cand[:, 0]), score


def cmd_kernels(args, dev):
    lib = L.load()
    cfg = EnvConfig(H=16, W=16, mine_count=40)
    K, margin, M, H, W, A = 8, 0.1, 40, 16, 16, 256
    for n in args.envs:
        _, _, rev, num = live_boards(n, cfg, dev)
        base = posterior_states(rev, num, M, budget=1 << 12, method="grouped")
        res = lookahead_states(rev, num, M, base, K=K, margin=margin, budget=1 << 12, method="grouped")
        rows = n * K * 9
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
        slot, count, cand = i32(n), i32(1), i32(n, K)
        rev2 = torch.empty((rows, H, W), dtype=torch.uint8, device=dev)
        num2, live2 = torch.empty_like(rev2), torch.empty(rows, dtype=torch.uint8, device=dev)
        s = L.stream_ptr(dev)

        def hip_expand():
            L.check(lib.ms_lookahead_expand(L.ptr(base["status"]), L.ptr(base["prob"]), L.ptr(rev), L.ptr(num), n, H, W,
                                            K, margin, n, L.ptr(slot), L.ptr(count), L.ptr(cand), L.ptr(rev2),
                                            L.ptr(num2), L.ptr(live2), s))
        hip_expand()
        post2 = posterior_states(rev2, num2, M, live=live2, budget=1 << 12, method="grouped")
        action = torch.empty(n, dtype=torch.int64, device=dev)
        score = torch.empty((n, K), dtype=torch.float64, device=dev)
        n_scored, changed = i32(n), torch.empty(n, dtype=torch.uint8, device=dev)

        def hip_score():
            L.check(lib.ms_lookahead_score(L.ptr(slot), L.ptr(cand), L.ptr(base["prob"]), L.ptr(base["configs"]),
                                           L.ptr(post2["status"]), L.ptr(post2["prob"]), L.ptr(post2["configs"]),
                                           L.ptr(rev2), M, n, H, W, K, n, L.ptr(action), L.ptr(score), L.ptr(n_scored),
                                           L.ptr(changed), s))
        hip_score()
        assert torch.equal(action, res["action"])
        # the dense PyTorch restatement, checked against the kernels on the guess boards
        guess, tcand, trev2, tnum2, tlive2 = torch_expand(base["status"], base["prob"], rev, num, K, margin)
        tpost2 = posterior_states(trev2.reshape(rows, H, W), tnum2.reshape(rows, H, W), M, live=tlive2.reshape(rows),
                                  budget=1 << 12, method="grouped")
        tact, _ = torch_score(tcand, base["prob"], base["configs"], tpost2["status"], tpost2["prob"], tpost2["configs"],
                              trev2, M)
        agree = float((tact[guess] == action[guess]).double().mean())
        rec = {"what": "kernels", "envs": n, "guess_boards": int(count), "torch_agrees_on_guess_boards": agree}
        for rep in range(2):
            rec[f"hip_expand_us_{rep}"] = timed(hip_expand)
            rec[f"torch_expand_us_{rep}"] = timed(lambda: torch_expand(base["status"], base["prob"], rev, num, K, margin))
            rec[f"hip_score_us_{rep}"] = timed(hip_score)
            rec[f"torch_score_us_{rep}"] = timed(lambda: torch_score(tcand, base["prob"], base["configs"],
                                                                     tpost2["status"], tpost2["prob"],
                                                                     tpost2["configs"], trev2, M))
        emit(rec, args.out)


def cmd_step(args, dev):
    from ms_amd.imitate import collect_expert
    cfg = EnvConfig(H=16, W=16, mine_count=40)
    for n in args.envs:
        _, batch, _, _ = live_boards(n, cfg, dev)
        obs = batch["obs"]
        rec = {"what": "step", "envs": n, "workspace_bytes_cap_n": workspace_bytes(n, 8, 16, 16)}
        models = {k: PosteriorModel(40, budget=1 << 12, method="grouped", lookahead=k).to(dev) for k in (0, 8)}
        for rep in range(2):
            for k, m in models.items():
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                rec[f"forward_us_lookahead{k}_{rep}"] = timed(lambda: m(obs), calls=20, warm=2)
                rec[f"forward_peak_bytes_lookahead{k}"] = torch.cuda.max_memory_allocated(dev) - before
        for rep in range(2):
            for k in (0, 8):
                vec = VecMinesweeper(n, cfg, seed=0, device=dev)
                buf = collect_expert(vec, 32, budget=1 << 12, seed=1, lookahead=k)  # opening moves: warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                collect_expert(vec, 32, budget=1 << 12, seed=2, buffer=buf, reset=False, lookahead=k)
                torch.cuda.synchronize()
                rec[f"collect_ms_per_step_lookahead{k}_{rep}"] = (time.perf_counter() - t0) * 1e3 / 32
        emit(rec, args.out)


def cmd_winrate(args, dev):
    from ms_amd.eval import evaluate_vec
    H, W, M = (int(x) for x in args.board.split("x"))
    cfg = EnvConfig(H=H, W=W, mine_count=M)
    for name, k in (("greedy", 0), ("lookahead", args.lookahead)):
        m = PosteriorModel(M, method="grouped", lookahead=k, margin=args.margin).to(dev)
        t0 = time.perf_counter()
        r = evaluate_vec(m, cfg, episodes=args.episodes, seed=0, num_envs=args.envs[0])
        rec = {"what": "winrate", "board": args.board, "player": name, "K": k, "margin": args.margin,
               "episodes": args.episodes, "envs": args.envs[0], "seconds": time.perf_counter() - t0,
               **{x: r[x] for x in ("win_rate", "win_ci_low", "win_ci_high", "wins", "avg_steps", "invalid_rate")},
               **m.lookahead_counters()}
        emit(rec, args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "step", "winrate"])
    ap.add_argument("--envs", type=int, nargs="+", default=None)
    ap.add_argument("--board", type=str, default="16x16x40")
    ap.add_argument("--episodes", type=int, default=32768)
    ap.add_argument("--lookahead", type=int, default=8)
    ap.add_argument("--margin", type=float, default=0.1)
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    args.envs = args.envs or {"kernels": [1024, 4096], "step": [1024], "winrate": [4096]}[args.what]
    dev = torch.device("cuda", torch.cuda.current_device())
    {"kernels": cmd_kernels, "step": cmd_step, "winrate": cmd_winrate}[args.what](args, dev)


if __name__ == "__main__":
    main()
