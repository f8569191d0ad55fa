"""On-policy imitation without a device (include/msdagger.h, ms_amd/dagger.py): the ctypes table
and the constants against the header, the argument checks (made before any device work), the beta
schedule, the imitation config keys and the new YAML, and the numpy restatement
tests/dagger_ref.py itself (coin thresholds, rule order, greedy). No device needed."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import dagger_ref as R
from conftest import PKG_DIR, ROOT
from test_abi_signatures import parse_headers, table_errors

DAGGER_H = os.path.join(ROOT, "include", "msdagger.h")


def test_table_matches_the_header():
    from ms_amd import _lib as L
    lib = L.load()
    protos, structs, defines, diag_only = parse_headers([DAGGER_H])
    table = L.SIGNATURES_DAGGER
    assert sorted(protos) == ["ms_dagger_act"] and not structs and not diag_only
    assert table_errors(table, L._RESTYPES, protos) == []
    others = (L.SIGNATURES, L.SIGNATURES_GROUPED, L.SIGNATURES_EXPERT, L.SIGNATURES_BC, L.SIGNATURES_SYM)
    assert not any(set(table) & set(t) for t in others)
    with open(os.path.join(PKG_DIR, "libmsenv_diag.so"), "rb") as f:
        diag_image = f.read()
    fn = lib.ms_dagger_act  # the product library exports and binds it
    assert list(fn.argtypes) == table["ms_dagger_act"] and fn.restype is ctypes.c_int
    assert b"\0ms_dagger_act\0" in diag_image
    # a wrong table is reported: n narrowed to 32 bits, beta widened, and a parameter dropped
    params = [p for _, p in protos["ms_dagger_act"][1]]
    narrowed = list(table["ms_dagger_act"])
    narrowed[params.index("n")] = ctypes.c_int32
    errs = table_errors({"ms_dagger_act": narrowed}, L._RESTYPES, protos)
    assert errs and "int64_t n" in errs[0]
    widened = list(table["ms_dagger_act"])
    widened[params.index("beta")] = ctypes.c_double
    errs = table_errors({"ms_dagger_act": widened}, L._RESTYPES, protos)
    assert errs and "float beta" in errs[0]
    assert table_errors({"ms_dagger_act": table["ms_dagger_act"][:-1]}, L._RESTYPES, protos)
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3
    assert [k for k, _ in L.DAGGER_OUTPUTS] == params[params.index("action"):params.index("stream")]


def test_constants_match_the_header():
    from ms_amd import _lib as L
    from ms_amd import dagger as D
    defines = parse_headers([DAGGER_H])[2]
    names = ["MS_DAGGER_GREEDY", "MS_DAGGER_SAMPLE", "MS_DAGGER_SRC_UNIFORM", "MS_DAGGER_SRC_EXPERT",
             "MS_DAGGER_SRC_LEARNER", "MS_DAGGER_MAX_CELLS", "MS_DAGGER_C_LEARNER", "MS_DAGGER_C_BETA",
             "MS_DAGGER_C_EXPLORE"]
    assert sorted(defines) == sorted(names)
    for name in names:
        assert getattr(L, name) == defines[name], name
    assert (R.C_LEARNER, R.C_BETA, R.C_EXPLORE) == tuple(
        defines[n] for n in ("MS_DAGGER_C_LEARNER", "MS_DAGGER_C_BETA", "MS_DAGGER_C_EXPLORE"))
    assert (R.GREEDY, R.SAMPLE) == (defines["MS_DAGGER_GREEDY"], defines["MS_DAGGER_SAMPLE"])
    assert (R.SRC_UNIFORM, R.SRC_EXPERT, R.SRC_LEARNER) == (0, 1, 2) == tuple(
        defines[n] for n in ("MS_DAGGER_SRC_UNIFORM", "MS_DAGGER_SRC_EXPERT", "MS_DAGGER_SRC_LEARNER"))
    # three distinct 64-bit constants, none of them k_dropout's domain constant (csrc/msrollout.hip)
    cs = {defines[n] for n in ("MS_DAGGER_C_LEARNER", "MS_DAGGER_C_BETA", "MS_DAGGER_C_EXPLORE")}
    assert len(cs) == 3 and 0xD1B54A32D192ED03 not in cs and all(1 << 32 < c < 1 << 64 for c in cs)
    assert defines["MS_DAGGER_MAX_CELLS"] == 3968 == 64 * 62  # the board bound of include/msenv.h
    assert D.MODES == {"greedy": defines["MS_DAGGER_GREEDY"], "sample": defines["MS_DAGGER_SAMPLE"]}
    assert (D.SOURCE_UNIFORM, D.SOURCE_EXPERT, D.SOURCE_LEARNER) == (0, 1, 2)


def test_bad_arguments_are_refused_before_any_device_work():
    """Every pointer is a fake address: a call that got as far as a launch would not return 1."""
    from ms_amd import _lib as L
    lib = L.load()
    fake = ctypes.c_void_p(4096)

    def call(logits=fake, mask=fake, best=fake, expert=fake, kind=fake, n=4, A=81, row_begin=0, beta=0.5,
             explore=0.0, mode=0, action=fake, agree=fake):
        return lib.ms_dagger_act(logits, mask, best, expert, kind, n, A, row_begin, 1, 2, beta, explore, mode, action,
                                 fake, fake, agree, None)

    bad = [dict(beta=1.5), dict(beta=float("nan")), dict(beta=-0.01), dict(explore=1.5), dict(explore=float("nan")),
           dict(explore=-1.0), dict(mode=2), dict(mode=-1), dict(logits=None, beta=0.99), dict(logits=None, beta=0.0),
           dict(A=0), dict(A=-1), dict(A=3969), dict(n=0), dict(n=-1), dict(n=1 << 31), dict(row_begin=-1),
           dict(mask=None), dict(expert=None), dict(kind=None), dict(action=None), dict(best=None)]
    for kw in bad:
        assert call(**kw) == 1, kw  # MS_EINVAL
        assert b"ms_dagger_act" in lib.ms_last_error(), kw
    assert call(beta=1.5) == 1 and b"beta" in lib.ms_last_error()
    assert call(A=0) == 1 and b"3968" in lib.ms_last_error()
    assert call(logits=None) == 1 and b"logits" in lib.ms_last_error()
    from ms_amd.dagger import dagger_act
    import torch
    m = torch.ones((2, 4), dtype=torch.bool)
    tg = {"best": torch.zeros((2, 4), dtype=torch.uint8), "action": torch.zeros(2, dtype=torch.int64),
          "kind": torch.zeros(2, dtype=torch.uint8)}
    for kw in (dict(beta=1.5), dict(beta=float("nan")), dict(beta=0.5, explore=2.0), dict(beta=0.5, mode="argmax"),
               dict(beta=0.5)):  # the last one: no logits below beta 1
        with pytest.raises(ValueError):
            dagger_act(None, m, tg, seed=0, counter=0, **kw)


def test_beta_schedule():
    from ms_amd.dagger import beta_at
    assert beta_at(0, 1.0, 0.25, 40) == 1.0 and beta_at(40, 1.0, 0.25, 40) == 0.25
    assert beta_at(20, 1.0, 0.25, 40) == 0.625 and beta_at(10, 1.0, 0.0, 40) == 0.75
    assert beta_at(41, 1.0, 0.25, 40) == 0.25 and beta_at(10 ** 6, 1.0, 0.25, 40) == 0.25
    assert [beta_at(i, 1.0, 0.0, 2) for i in range(4)] == [1.0, 0.5, 0.0, 0.0]
    assert beta_at(0, 1.0, 0.25, 0) == 0.25 and beta_at(7, 1.0, 0.25, 0) == 0.25 and beta_at(0, 1.0, 0.3, -5) == 0.3
    assert beta_at(0, 0.2, 0.9, 10) == 0.2 and abs(beta_at(5, 0.2, 0.9, 10) - 0.55) < 1e-12  # may rise too
    assert all(beta_at(i, 1.0, 1.0, 0) == 1.0 for i in range(3))  # the defaults: every round the teacher's


def test_imitation_config_keys_and_the_dagger_yaml():
    from ms_amd.imitate import imitation_params
    from ms_amd.train import load_config
    d = imitation_params({})
    assert (d["beta_start"], d["beta_end"], d["beta_decay_iters"], d["learner"]) == (1.0, 1.0, 0, "greedy")
    got = imitation_params({"imitation": {"beta_end": 0.5, "learner": "sample"}})
    assert got["beta_end"] == 0.5 and got["learner"] == "sample" and got["beta_start"] == 1.0
    with pytest.raises(ValueError, match="unknown"):
        imitation_params({"imitation": {"beta_stop": 0.5}})
    sym = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium_sym.yaml"))
    dag = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium_dagger.yaml"))
    assert dag[1] == sym[1] and dag[2] == sym[2] and vars(dag[0]) == vars(sym[0])
    assert {k: v for k, v in dag[3].items() if k != "imitation"} == {k: v for k, v in sym[3].items() if k != "imitation"}
    il0, il1 = imitation_params(sym[3]), imitation_params(dag[3])
    four = ("beta_start", "beta_end", "beta_decay_iters", "learner")
    assert {k: v for k, v in il1.items() if k not in four} == {k: v for k, v in il0.items() if k not in four}
    assert set(dag[3]["imitation"]) - set(sym[3]["imitation"]) == set(four)
    assert all(il0[k] == d[k] for k in four)  # _sym stays the teacher's every round
    assert 0.0 <= il1["beta_end"] < 1.0 and 0.0 <= il1["beta_start"] <= 1.0 and il1["beta_decay_iters"] >= 0
    assert il1["learner"] in ("greedy", "sample")


def test_ref_coins_and_rule_order():
    n = 4096
    rows = np.arange(5, 5 + n)
    cb, ce = R.coin(9, R.C_BETA, 3, rows), R.coin(9, R.C_EXPLORE, 3, rows)
    assert cb.dtype == np.float32 and (cb >= 0).all() and (cb <= 1).all() and (ce >= 0).all() and (ce <= 1).all()
    assert not np.array_equal(cb, ce) and abs(float(cb.mean()) - 0.5) < 0.03 and abs(float(ce.mean()) - 0.5) < 0.03
    assert abs(float(np.corrcoef(cb, ce)[0, 1])) < 0.06  # ~4 sigma of 1/sqrt(n)
    # the coin of a row depends on its global index only
    assert np.array_equal(R.coin(9, R.C_BETA, 3, rows[100:200]), cb[100:200])
    assert not np.array_equal(R.coin(9, R.C_BETA, 4, rows), cb) and not np.array_equal(R.coin(8, R.C_BETA, 3, rows), cb)
    rng = np.random.default_rng(0)
    A = 7
    kind = rng.integers(0, 3, n).astype(np.uint8)
    u, l, e = (rng.integers(0, A, n) for _ in range(3))
    e = np.where(kind != 0, e, -1)
    best = rng.integers(0, 2, (n, A)).astype(np.uint8)
    kw = dict(seed=9, counter=3, row_begin=5)
    # beta 1, explore 0: the teacher where it has a target, a uniform click elsewhere; never the learner
    r = R.act(u, None, e, kind, best, beta=1.0, explore=0.0, **kw)
    assert np.array_equal(r["action"], np.where(kind != 0, e, u)) and np.array_equal(r["source"], (kind != 0) * 1)
    assert (r["learner_action"] == -1).all() and not r["agree"].any()
    # beta 0, explore 0: the learner everywhere, boards without a target included
    r = R.act(u, l, e, kind, best, beta=0.0, explore=0.0, **kw)
    assert np.array_equal(r["action"], l) and (r["source"] == 2).all()
    assert np.array_equal(r["agree"], ((kind != 0) & (best[np.arange(n), l] != 0)).astype(np.uint8))
    # explore 1 comes first: uniform whatever beta says (a coin of exactly 1.0 has probability 2^-24)
    for beta in (0.0, 0.3, 1.0):
        r = R.act(u, l, e, kind, best, beta=beta, explore=1.0, **kw)
        assert np.array_equal(r["action"], u) and not r["source"].any()
    # in between: each rule where its coin says so, in order
    r = R.act(u, l, e, kind, best, beta=0.3, explore=0.4, **kw)
    ex, le = ce < np.float32(0.4), cb >= np.float32(0.3)
    want = np.where(ex, 0, np.where(le, 2, np.where(kind != 0, 1, 0)))
    assert np.array_equal(r["source"], want) and len(set(want.tolist())) == 3
    assert abs(ex.mean() - 0.4) < 0.04 and abs((~ex & le).mean() - 0.6 * 0.7) < 0.04
    assert np.array_equal(r["action"], np.where(want == 0, u, np.where(want == 2, l, e)))
    assert np.array_equal(r["learner_action"], l)  # reported whoever plays


def test_ref_greedy():
    inf, nan = np.inf, np.nan
    lg = np.array([[1.0, 3.0, 3.0, 2.0],      # duplicated maxima: the lowest index
                   [9.0, 1.0, 2.0, 2.0],      # the maximum is masked
                   [1.0, 5.0, 2.0, 0.0],      # nothing legal: all legal
                   [-inf, -inf, -inf, -inf],  # no legal logit above -inf: the lowest legal cell
                   [0.0, nan, 1.0, 0.5],      # NaN where the arg-max would be
                   [nan, nan, nan, nan],      # every legal logit NaN
                   [nan, -inf, nan, -inf],    # NaN and -inf only
                   [inf, 1.0, inf, 0.0]], dtype=np.float32)
    mask = np.array([[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1],
                     [0, 1, 1, 1]], dtype=np.uint8)
    assert R.greedy(lg, mask).tolist() == [1, 2, 1, 1, 2, 2, 1, 2]
    assert R.lowest_legal(mask).tolist() == [0, 1, 0, 1, 0, 2, 1, 1]
    assert R.sampled([3, R.SENTINEL, 0, R.SENTINEL], mask[[0, 1, 2, 5]]).tolist() == [3, 1, 0, 2]
