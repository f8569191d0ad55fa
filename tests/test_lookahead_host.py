"""The two-guess lookahead on the host (include/mslookahead.h: ms_lookahead_host) against the exact
rational reference of tests/lookahead_ref.py, the header against its ctypes table, the argument
checks, the edge rows and the configuration. No device needed.

Bounds. ``score`` against the exact fraction: rel 1e-12, set by the issue; the twin's score is at
most nine products and sums of f64 terms that are themselves within a few ulp (the posterior's
combine), so the observed error is below 1e-15. The identity sum_v Z_v = Z (1 - p_c) is exact in
the reference (integers) and is what ``n_scored`` reports for the twin.

The issue asks for at least 30 guess boards on every shape of posterior_ref.SHAPES. The 5x1 board
with one mine cannot give them: its 80 states (every mine position with every set of safe cells
revealed) hold exactly 5 guess boards, the finished games whose one hidden cell is the mine
(test_thin_shape_has_five_guess_boards lists them). All 5 are used; every other shape gives 30."""
from __future__ import annotations

import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import lookahead_ref as R
import posterior_ref as P
from conftest import ROOT
from test_abi_signatures import parse_headers, table_errors

HEADER = os.path.join(ROOT, "include", "mslookahead.h")
NAMES = ["ms_lookahead_expand", "ms_lookahead_host", "ms_lookahead_score"]
METHODS = ("enumerate", "grouped")
K, MARGIN = 8, 0.1


def _stack(states):
    return np.stack([s["rev"] for s in states]), np.stack([s["number"] for s in states])


def _host(states, M, method="grouped", **kw):
    from ms_amd.lookahead import lookahead_host
    from ms_amd.posterior import posterior_host
    rev, num = _stack(states)
    base = posterior_host(rev, num, M, method=method)
    return base, lookahead_host(rev, num, M, base, method=method, **kw)


def test_table_matches_the_header():
    from ms_amd import _lib as L
    from conftest import PKG_DIR
    protos, structs, defines, diag_only = parse_headers([HEADER])
    assert sorted(protos) == NAMES and not structs and not diag_only
    assert table_errors(L.SIGNATURES_LOOKAHEAD, L._RESTYPES, protos) == []
    assert defines == {"MS_LOOKAHEAD_MAX_K": L.MS_LOOKAHEAD_MAX_K, "MS_LOOKAHEAD_OUTCOMES": L.MS_LOOKAHEAD_OUTCOMES,
                       "MS_LOOKAHEAD_SCORED_RTOL": L.MS_LOOKAHEAD_SCORED_RTOL}
    assert (L.MS_LOOKAHEAD_MAX_K, L.MS_LOOKAHEAD_OUTCOMES, L.MS_LOOKAHEAD_SCORED_RTOL) == (16, 9, 1e-9)
    others = [L.SIGNATURES, L.SIGNATURES_GROUPED, L.SIGNATURES_EXPERT, L.SIGNATURES_BC, L.SIGNATURES_SYM,
              L.SIGNATURES_DAGGER]
    assert not any(set(L.SIGNATURES_LOOKAHEAD) & set(t) for t in others)
    lib = L.load()
    with open(os.path.join(PKG_DIR, "libmsenv_diag.so"), "rb") as f:
        diag_image = f.read()
    for name, argtypes in L.SIGNATURES_LOOKAHEAD.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int, name
        assert b"\0" + name.encode() + b"\0" in diag_image, f"libmsenv_diag.so lacks {name}"
    wrong = dict(L.SIGNATURES_LOOKAHEAD, ms_lookahead_score=L.SIGNATURES_LOOKAHEAD["ms_lookahead_expand"])
    assert table_errors(wrong, L._RESTYPES, protos)  # a wrong table is reported
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3


def test_bad_arguments_are_refused_and_write_nothing():
    from ms_amd import _lib as L
    lib = L.load()
    n, H, W, M, Kk = 2, 4, 4, 3, 4
    st = R.guess_states()[(4, 4, 3)][:n]
    rev, num = _stack(st)
    rev, num = np.ascontiguousarray(rev), np.ascontiguousarray(num)
    from ms_amd.posterior import posterior_host
    base = posterior_host(rev, num, M)
    outs = {"slot": np.full(n, 7, np.int32), "count": np.full(1, 7, np.int32), "cand": np.full((n, Kk), 7, np.int32),
            "action": np.full(n, 7, np.int64), "score": np.full((n, Kk), 7.0), "n_scored": np.full(n, 7, np.int32),
            "changed": np.full(n, 7, np.uint8)}
    p = lambda a: a.ctypes.data  # noqa: E731
    good = dict(status=p(base["status"]), prob=p(base["prob"]), configs=p(base["configs"]), revealed=p(rev),
                number=p(num), mine_count=M, n=n, H=H, W=W, K=Kk, margin=0.1, cap=n, budget=0, grouped=0,
                **{k: p(v) for k, v in outs.items()})

    def host(**kw):
        a = dict(good, **kw)
        return lib.ms_lookahead_host(*a.values())

    bad = [dict(K=0), dict(K=17), dict(K=-1), dict(margin=-0.01), dict(margin=1.5), dict(margin=math.nan),
           dict(margin=math.inf), dict(cap=0), dict(cap=-3), dict(cap=1 << 40), dict(H=32, W=17), dict(H=0), dict(W=0),
           dict(n=0), dict(mine_count=-1), dict(mine_count=17), dict(budget=-1)]
    bad += [{k: None} for k in ("status", "prob", "configs", "revealed", "number", *outs)]
    for kw in bad:
        assert host(**kw) == 1, kw
        assert b"ms_lookahead_host" in lib.ms_last_error(), kw
        for k, v in outs.items():
            assert (v == 7).all(), (kw, k)
    assert host(H=32, W=17) == 1 and b"512" in lib.ms_last_error()
    assert host() == 0 and outs["count"][0] == 2 and (outs["slot"] == [0, 1]).all()
    # the device entry points check before any device work: the pointers are never dereferenced
    fake = ctypes.c_void_p(4096)
    exp = dict(status=fake, prob=fake, revealed=fake, number=fake, n=4, H=4, W=4, K=8, margin=0.1, cap=4, slot=fake,
               count=fake, cand=fake, revealed2=fake, number2=fake, live2=fake, stream=None)
    sco = dict(slot=fake, cand=fake, prob=fake, configs=fake, status2=fake, prob2=fake, configs2=fake, revealed2=fake,
               mine_count=3, n=4, H=4, W=4, K=8, cap=4, action=fake, score=fake, n_scored=fake, changed=fake, stream=None)
    for fn, args, who in ((lib.ms_lookahead_expand, exp, b"ms_lookahead_expand:"),
                          (lib.ms_lookahead_score, sco, b"ms_lookahead_score:")):
        cases = [dict(K=0), dict(K=17), dict(cap=0), dict(H=32, W=17), dict(n=0), dict(n=1 << 31), dict(cap=1 << 31)]
        cases += [dict(margin=m) for m in (-0.5, 1.01, math.nan)] if "margin" in args else [dict(mine_count=17)]
        cases += [{k: None} for k, v in args.items() if v is fake]
        for kw in cases:
            assert fn(*dict(args, **kw).values()) == 1, (who, kw)
            assert who in lib.ms_last_error(), (who, kw)


@pytest.mark.parametrize("shape", P.SHAPES)
def test_host_twin_equals_the_exact_reference(shape):
    H, W, M = shape
    states = R.guess_states()[shape]
    assert len(states) >= (5 if shape == (5, 1, 1) else R.GUESS_PER_SHAPE)
    worst = 0.0
    for method in METHODS:
        base, got = _host(states, M, method, K=K, margin=MARGIN)
        assert got["count"][0] == len(states) and np.array_equal(got["slot"], np.arange(len(states)))
        for i, s in enumerate(states):
            assert float(s["Z"]) == base["configs"][i]
            ex = R.exact(s["rev"], s["number"], M, base["prob"][i], K, MARGIN, masks=s["masks"])
            assert ex["identity"] == 0
            cand = got["cand"][i]
            nc = len(ex["cand"])
            assert cand[:nc].tolist() == ex["cand"] and (cand[nc:] == -1).all(), (shape, method, i)
            assert np.isnan(got["score"][i, nc:]).all()
            assert got["n_scored"][i] == nc, (shape, method, i)  # unbounded searches: every candidate is scored
            for k, f in enumerate(ex["score"]):
                err = abs(Fraction(float(got["score"][i, k])) - f)
                worst = max(worst, float(err / f) if f else float(err))
                assert err <= Fraction(1, 10 ** 12) * f, (shape, method, i, k, got["score"][i, k], float(f))
            assert got["action"][i] == ex["action"] and got["changed"][i] == ex["changed"], (shape, method, i)
    print(f"{shape}: {len(states)} guess boards, worst relative score error {worst:.3g}, "
          f"{int(got['changed'].sum())} with another choice than the greedy")


def test_enough_boards_where_the_choice_changes():
    total = 0
    for (H, W, M), states in R.guess_states().items():
        total += int(_host(states, M, K=K, margin=MARGIN)[1]["changed"].sum())
    assert total >= 10, total


def test_thin_shape_has_five_guess_boards():
    found = []
    for rev, number in R.all_states(5, 1, 1):
        masks = R.consistent_masks(rev, number, 1)
        Z, counts = R.posterior(masks, rev)
        if R.is_guess(rev, Z, counts):
            found.append(int((rev == 0).sum()))
    assert found == [1] * 5  # the finished games: the one hidden cell is the mine
    assert len(R.guess_states()[(5, 1, 1)]) == 5


def test_k1_is_the_greedy_player():
    from ms_amd.expert import expert_targets_host
    for (H, W, M), states in R.guess_states().items():
        base, got = _host(states, M, K=1, margin=1.0)
        tg = expert_targets_host(base, np.stack([s["rev"] for s in states]) == 0)
        assert (tg["kind"] == 2).all()
        assert np.array_equal(got["action"], tg["action"]) and not got["changed"].any()
        assert np.array_equal(got["cand"][:, 0], tg["action"].astype(np.int32))


def test_margin_zero_keeps_the_cells_at_pmin():
    tied = 0
    for (H, W, M), states in R.guess_states().items():
        base, got = _host(states, M, K=16, margin=0.0)
        for i, s in enumerate(states):
            hid = np.flatnonzero(s["rev"].reshape(-1) == 0)
            pm = base["prob"][i][hid].min()
            want = [int(c) for c in hid if base["prob"][i][c] == pm][:16]
            tied += len(want) > 1
            assert [int(c) for c in got["cand"][i] if c >= 0] == want
            assert got["action"][i] in want
    assert tied >= 10


def test_a_click_that_wins_counts_as_one():
    """2x2, one mine, the top row revealed as 1 1: the two hidden cells are 50 : 50, and whichever
    is clicked the game is over (one hidden cell left = M). Rule 1 gives t = 1 and score 1/2;
    rule 3 alone would give 1 - pmin' = 0."""
    from ms_amd.lookahead import lookahead_host
    from ms_amd.posterior import posterior_host
    rev = np.array([[[1, 1], [0, 0]]], dtype=np.uint8)
    num = np.array([[[1, 1], [9, 9]]], dtype=np.uint8)
    for method in METHODS:
        base = posterior_host(rev, num, 1, method=method)
        assert base["prob"][0].tolist() == [0, 0, 0.5, 0.5]
        got = lookahead_host(rev, num, 1, base, K=4, margin=0.0, method=method)
        assert got["cand"][0].tolist() == [2, 3, -1, -1] and got["score"][0, :2].tolist() == [0.5, 0.5]
        assert got["action"][0] == 2 and got["n_scored"][0] == 2 and got["changed"][0] == 0


@pytest.mark.parametrize("shape", [(1, 7, 2), (5, 1, 2)])
def test_thin_boards(shape):
    H, W, M = shape
    states = []
    for rev, number in R.all_states(H, W, M):
        masks = R.consistent_masks(rev, number, M)
        Z, counts = R.posterior(masks, rev)
        if R.is_guess(rev, Z, counts):
            states.append({"rev": rev, "number": number, "masks": masks})
    assert len(states) >= 10
    for method in METHODS:
        base, got = _host(states, M, method, K=3, margin=1.0)
        for i, s in enumerate(states):
            ex = R.exact(s["rev"], s["number"], M, base["prob"][i], 3, 1.0, masks=s["masks"])
            assert [int(c) for c in got["cand"][i] if c >= 0] == ex["cand"]
            assert got["action"][i] == ex["action"] and got["changed"][i] == ex["changed"]
            for k, f in enumerate(ex["score"]):
                assert abs(Fraction(float(got["score"][i, k])) - f) <= Fraction(1, 10 ** 12) * f


def test_budget_one_leaves_candidates_unscored_and_falls_back():
    from ms_amd.expert import expert_targets_host
    none_scored = 0
    for shape in ((5, 5, 5), (4, 6, 5)):
        states = R.guess_states()[shape]
        base, got = _host(states, shape[2], K=K, margin=MARGIN, budget=1)
        full = _host(states, shape[2], K=K, margin=MARGIN)[1]
        tg = expert_targets_host(base, np.stack([s["rev"] for s in states]) == 0)
        assert np.array_equal(got["cand"], full["cand"])
        assert (got["n_scored"] <= full["n_scored"]).all()
        scored = ~np.isnan(got["score"])
        assert np.array_equal(scored.sum(axis=1), got["n_scored"])
        assert np.array_equal(got["score"][scored].view(np.uint64), full["score"][scored].view(np.uint64))
        zero = got["n_scored"] == 0
        none_scored += int(zero.sum())
        assert np.array_equal(got["action"][zero], tg["action"][zero]) and not got["changed"][zero].any()
    assert none_scored >= 1


def test_cap_and_boards_without_a_slot():
    from ms_amd.lookahead import lookahead_host
    from ms_amd.posterior import posterior_host
    states = R.guess_states()[(4, 4, 3)][:6]
    rev, num = _stack(states)
    rev, num = rev.copy(), num.copy()
    rev[2] = 0  # nothing revealed: status 0, no slot
    base = posterior_host(rev, num, 3)
    full = lookahead_host(rev, num, 3, base, K=4, margin=0.1)
    assert full["slot"].tolist() == [0, 1, -1, 2, 3, 4] and full["count"][0] == 5
    assert full["action"][2] == -1 and full["n_scored"][2] == 0 and (full["cand"][5] == -1).all()
    assert np.isnan(full["score"][5]).all()
    two = lookahead_host(rev, num, 3, base, K=4, margin=0.1, cap=2)
    assert two["slot"].tolist() == [0, 1, -1, -1, -1, -1] and two["count"][0] == 5
    assert two["action"][2:].tolist() == [-1] * 4 and np.array_equal(two["action"][:2], full["action"][:2])
    assert np.array_equal(two["cand"], full["cand"][:2])


def test_config_keys_yaml_and_invalid_values():
    from ms_amd.imitate import collect_expert, imitation_params
    from ms_amd.posterior import PosteriorModel
    from ms_amd.train import load_config
    d = imitation_params({})
    assert d["lookahead"] == 0 and d["lookahead_margin"] == 0.1
    got = imitation_params({"imitation": {"lookahead": 4, "lookahead_margin": 0.2}})
    assert got["lookahead"] == 4 and got["lookahead_margin"] == 0.2
    with pytest.raises(ValueError, match="unknown"):
        imitation_params({"imitation": {"look_ahead": 4}})
    sym = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium_sym.yaml"))
    la = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium_lookahead.yaml"))
    assert la[1] == sym[1] and la[2] == sym[2] and vars(la[0]) == vars(sym[0])
    il0, il1 = imitation_params(sym[3]), imitation_params(la[3])
    two = ("lookahead", "lookahead_margin")
    assert {k: v for k, v in il1.items() if k not in two} == {k: v for k, v in il0.items() if k not in two}
    assert il1["lookahead"] == 8 and il1["lookahead_margin"] == 0.1 and il0["lookahead"] == 0
    m = PosteriorModel(10)
    assert m.lookahead == 0 and m.lookahead_counters() == dict.fromkeys(PosteriorModel.COUNTERS, 0)
    assert list(m.state_dict()) == list(PosteriorModel(10, lookahead=8).state_dict())
    for kw in (dict(lookahead=-1), dict(lookahead=17), dict(lookahead=True), dict(lookahead=8, margin=-0.1),
               dict(lookahead=8, margin=1.5), dict(lookahead=8, margin=math.nan), dict(lookahead=8, lookahead_cap=0)):
        with pytest.raises(ValueError, match="lookahead"):
            PosteriorModel(10, **kw)
    with pytest.raises(ValueError, match="lookahead"):
        collect_expert(None, 4, budget=16, seed=0, lookahead=17)
    with pytest.raises(ValueError, match="lookahead"):
        collect_expert(None, 4, budget=16, seed=0, lookahead=8, margin=2.0)
