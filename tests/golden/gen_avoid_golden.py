"""Avoidability fixtures from the REFERENCE (minesweeper/avoidability.py: analyze_avoidability).

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_avoid_golden.py

Writes tests/golden/avoid_states.npz: board states met by a rule-first player on the reference
env, each with a chosen cell and the reference's analysis of it. Data only; the tests never
import the reference.

Player: the lowest forced-safe cell when the reference finds one, else a random hidden safe
cell with p = 0.85, else any hidden cell (a purely random player almost never reaches states in
which only the exact search proves a cell safe).

Classes (``cls``): 0 ``prop`` the propagation rules proved a safe cell (the search never ran),
1 ``exact_safe`` only the search proved one, 2 ``forced`` nothing is provably safe. The class is
read off the reference by counting its solver's queries, not re-derived.

Per board ``HxWxK`` the file holds ``<board>_rev`` and ``_mine`` (np.packbits of [S, H*W]),
``_chosen`` i64[S], ``_avoidable`` u8[S], ``_safe`` (packed forced-safe mask), ``_comp_sizes``
(all states' sorted component sizes, concatenated) with ``_comp_off`` i32[S+1],
``_chosen_comp`` i32[S] (0 = None), ``_chosen_safe`` u8[S], ``_cls`` u8[S] and ``_ref_nodes``
i32[S] (the reference's largest per-query count of attempted assignments; 0 = no search)."""
import os

import numpy as np

from minesweeper import avoidability as AV  # noqa: E402  (the reference, via PYTHONPATH)
from minesweeper.env import EnvConfig, MinesweeperEnv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BOARDS = ((9, 9, 10), (16, 16, 40), (30, 16, 99), (16, 30, 99))
CAPS = {0: 44, 1: 36, 2: 40}  # at most 120 states per board
NEED = {0: 16, 1: 8, 2: 8}
WANT = {0: 24, 1: 12, 2: 16}  # stop early once every class has this many

# count the reference solver's work without touching its text
_stats = {"queries": 0, "cur": 0, "max": 0}
_orig_feasible = AV._ConstraintSolver.is_feasible
_orig_assign = AV._ConstraintSolver._assign


def _feasible(self, forced=None):
    _stats["queries"] += 1
    _stats["cur"] = 0
    out = _orig_feasible(self, forced)
    _stats["max"] = max(_stats["max"], _stats["cur"])
    return out


def _assign(self, *a, **k):
    _stats["cur"] += 1
    return _orig_assign(self, *a, **k)


AV._ConstraintSolver.is_feasible = _feasible
AV._ConstraintSolver._assign = _assign


def analyse(env, chosen):
    _stats.update(queries=0, cur=0, max=0)
    res = AV.analyze_avoidability(env, chosen)
    if not res.avoidable:
        cls = 2
    else:
        cls = 1 if _stats["queries"] else 0
    return res, cls, _stats["max"]


def main():
    rng = np.random.default_rng(20240607)
    out = {}
    for (H, W, K) in BOARDS:
        A = H * W
        rows = []
        have = {0: 0, 1: 0, 2: 0}
        episode = 0
        while True:
            if all(have[c] >= WANT[c] for c in have) or (episode >= 4000 and all(have[c] >= NEED[c] for c in have)):
                break
            env = MinesweeperEnv(EnvConfig(H=H, W=W, mine_count=K), seed=int(rng.integers(0, 2**31 - 1)))
            env.reset()
            episode += 1
            _, _, done, _ = env.step(int(rng.integers(0, A)))
            while not done:
                res, cls, _ = analyse(env, None)
                hidden = np.flatnonzero(~env.revealed.reshape(-1))
                if res.forced_safe_cells:
                    pick = min(res.forced_safe_cells)
                else:
                    safe = hidden[~env.mine_mask.reshape(-1)[hidden]]
                    pick = int(rng.choice(safe)) if (safe.size and rng.random() < 0.85) else int(rng.choice(hidden))
                take = have[cls] < CAPS[cls] and (cls != 0 or rng.random() < 0.08)
                if take:
                    u = rng.random()
                    if u < 0.5:
                        chosen = int(pick)
                    elif u < 0.92:
                        chosen = int(rng.choice(hidden))
                    else:
                        chosen = int(rng.choice(np.flatnonzero(env.revealed.reshape(-1))))
                    r, c2, nodes = analyse(env, chosen)
                    assert c2 == cls and r.forced_safe_cells == res.forced_safe_cells
                    safe_mask = np.zeros(A, dtype=np.uint8)
                    safe_mask[list(r.forced_safe_cells)] = 1
                    rows.append(dict(rev=env.revealed.reshape(-1).astype(np.uint8).copy(),
                                     mine=env.mine_mask.reshape(-1).astype(np.uint8).copy(), chosen=chosen,
                                     avoidable=int(r.avoidable), safe=safe_mask,
                                     comps=sorted(int(s) for s in r.component_sizes),
                                     chosen_comp=int(r.chosen_component_size or 0),
                                     chosen_safe=int(r.chosen_is_forced_safe), cls=cls, nodes=nodes))
                    have[cls] += 1
                _, _, done, _ = env.step(pick)
        assert all(have[c] >= NEED[c] for c in have), have
        assert any(r["rev"][r["chosen"]] for r in rows), "no revealed chosen cell"
        b = f"{H}x{W}x{K}"
        out[f"{b}_rev"] = np.packbits(np.stack([r["rev"] for r in rows]), axis=1)
        out[f"{b}_mine"] = np.packbits(np.stack([r["mine"] for r in rows]), axis=1)
        out[f"{b}_safe"] = np.packbits(np.stack([r["safe"] for r in rows]), axis=1)
        out[f"{b}_chosen"] = np.array([r["chosen"] for r in rows], dtype=np.int64)
        out[f"{b}_avoidable"] = np.array([r["avoidable"] for r in rows], dtype=np.uint8)
        out[f"{b}_comp_sizes"] = np.array([s for r in rows for s in r["comps"]], dtype=np.int32)
        out[f"{b}_comp_off"] = np.cumsum([0] + [len(r["comps"]) for r in rows]).astype(np.int32)
        out[f"{b}_chosen_comp"] = np.array([r["chosen_comp"] for r in rows], dtype=np.int32)
        out[f"{b}_chosen_safe"] = np.array([r["chosen_safe"] for r in rows], dtype=np.uint8)
        out[f"{b}_cls"] = np.array([r["cls"] for r in rows], dtype=np.uint8)
        out[f"{b}_ref_nodes"] = np.array([r["nodes"] for r in rows], dtype=np.int32)
        print(b, "episodes", episode, "states", len(rows), have, "max ref nodes", int(out[f"{b}_ref_nodes"].max()))
    out["boards"] = np.array([f"{H}x{W}x{K}" for (H, W, K) in BOARDS])
    path = os.path.join(HERE, "avoid_states.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
