"""tests/golden/avoid_states.npz (gen_avoid_golden.py: the reference's analyze_avoidability on
states a rule-first player met) and the comparison both avoidability suites share."""
from __future__ import annotations

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLS_PROP, CLS_EXACT_SAFE, CLS_FORCED = 0, 1, 2


@functools.lru_cache(maxsize=None)
def boards():
    z = np.load(os.path.join(GOLDEN, "avoid_states.npz"), allow_pickle=False)
    return tuple(str(b) for b in z["boards"])


@functools.lru_cache(maxsize=None)
def load(board: str):
    """The states of one board, unpacked once: rev / mine / safe u8 [S, H, W] or [S, A]."""
    z = np.load(os.path.join(GOLDEN, "avoid_states.npz"), allow_pickle=False)
    H, W, K = (int(v) for v in board.split("x"))
    A = H * W
    d = {k: z[f"{board}_{k}"] for k in ("chosen", "avoidable", "comp_sizes", "comp_off", "chosen_comp",
                                        "chosen_safe", "cls", "ref_nodes")}
    for k in ("rev", "mine", "safe"):
        d[k] = np.unpackbits(z[f"{board}_{k}"], axis=1)[:, :A]
    S = d["rev"].shape[0]
    d["rev"] = d["rev"].reshape(S, H, W)
    d["mine"] = d["mine"].reshape(S, H, W)
    d.update(H=H, W=W, K=K, S=S)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def component_multiset(comp_size_row: np.ndarray):
    """Sorted component sizes rebuilt from the per-cell output: s cells carry size s per component."""
    sizes, counts = np.unique(comp_size_row[comp_size_row > 0], return_counts=True)
    out = []
    for s, c in zip(sizes, counts):
        assert c % s == 0, f"{c} cells claim a component of size {s}"
        out += [int(s)] * (int(c) // int(s))
    return out


def assert_matches_reference(got: dict, ref: dict, rows=None, where: str = ""):
    """Every output of the rows (default all) equals the reference's: integers exactly, the safe
    mask bit for bit, component sizes as a sorted multiset."""
    rows = range(ref["S"]) if rows is None else rows
    for i in rows:
        tag = f"{where} state {i} (class {int(ref['cls'][i])})"
        assert int(got["status"][i]) == 1, tag
        assert int(got["avoidable"][i]) == int(ref["avoidable"][i]), tag
        assert np.array_equal(got["safe_mask"][i], ref["safe"][i]), tag
        assert int(got["n_safe"][i]) == int(ref["safe"][i].sum()), tag
        assert int(got["chosen_safe"][i]) == int(ref["chosen_safe"][i]), tag
        assert int(got["chosen_comp"][i]) == int(ref["chosen_comp"][i]), tag
        comps = list(ref["comp_sizes"][ref["comp_off"][i]:ref["comp_off"][i + 1]])
        assert component_multiset(got["comp_size"][i]) == comps, tag
        assert int(got["n_comp"][i]) == len(comps) and int(got["n_frontier"][i]) == sum(comps), tag
        if int(ref["cls"][i]) == CLS_PROP:  # the closure answered: no search
            assert int(got["max_nodes"][i]) == 0, tag
        elif int(ref["cls"][i]) == CLS_EXACT_SAFE:
            assert int(got["max_nodes"][i]) > 0, tag
