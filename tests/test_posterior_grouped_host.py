"""The exact posterior with grouped counting on the host (include/msposterior_grouped.h:
ms_posterior_host_grouped) against brute-force enumeration (posterior_ref.py), the enumerating
host solver (bitwise wherever both decide), constructed boards only grouping can finish, the
fixture states of tests/golden/avoid_states.npz, and the argument checks and ctypes table of the
new header. No device needed."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import avoid_fixture as F
import posterior_ref as R
from conftest import ROOT
from test_abi_signatures import parse_headers, table_errors
from test_posterior_host import _numbers, _two_cells

BOARDS = ["9x9x10", "16x16x40", "30x16x99", "16x30x99"]
BUDGET = 1 << 16
GROUPED_H = os.path.join(ROOT, "include", "msposterior_grouped.h")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def stripe(W: int):
    """3 x W, the whole middle row revealed, one mine per column alternating top and bottom: every
    number is 3, the two ends 2, M = W. For W divisible by 3 the closure deduces nothing; the two
    hidden cells of a column share their constraints, each such group holds exactly one mine, so
    the grouped system has one solution and Z = 2^W with p = 1/2 everywhere."""
    rev = np.zeros((1, 3, W), dtype=np.uint8)
    rev[0, 1] = 1
    num = np.full((1, 3, W), 3, dtype=np.uint8)
    num[0, :, 0] = num[0, :, -1] = 2
    return rev, num


@functools.lru_cache(maxsize=None)
def fixture_host(board, method):
    """A host solver on the fixture states at 2^16 nodes, once per session."""
    from ms_amd.posterior import posterior_host
    z = F.load(board)
    num = _numbers(z["mine"])
    got = posterior_host(z["rev"], num, z["K"], host_budget=BUDGET, method=method)
    for v in got.values():
        v.setflags(write=False)
    return z, num, got


def test_oracle_set_grouped_equals_brute_force_and_enumerate():
    from ms_amd.posterior import posterior_host
    worst_p = worst_z = 0.0
    states = 0
    for (H, W, M), (rev, number, p, configs) in R.by_shape(R.oracle_states()).items():
        got = posterior_host(rev, number, M, method="grouped")
        ref = posterior_host(rev, number, M, method="enumerate")
        assert (got["status"] == 1).all(), (H, W, M)
        worst_p = max(worst_p, float(np.abs(got["prob"] - p).max()))
        worst_z = max(worst_z, float((np.abs(got["configs"] - configs) / configs).max()))
        assert not got["prob"][rev.reshape(len(rev), -1) != 0].any()
        assert np.array_equal(bits(got["prob"]), bits(ref["prob"])), (H, W, M)
        assert np.array_equal(bits(got["configs"]), bits(ref["configs"])), (H, W, M)
        assert np.array_equal(got["status"], ref["status"])
        states += len(rev)
    print(f"{states} states: worst |p - oracle| {worst_p:.3g}, worst relative configs error {worst_z:.3g}")
    assert states == 84
    assert worst_p <= 1e-12 and worst_z <= 1e-12


@pytest.mark.parametrize("W", [30, 36, 60])
def test_stripe_is_decided_by_grouping_only(W):
    """The test that fails without the feature: 2^W solutions, one grouped solution."""
    from ms_amd.posterior import posterior_host
    rev, num = stripe(W)
    got = posterior_host(rev, num, W, host_budget=BUDGET, method="grouped")
    print(f"W = {W}: grouped status {got['status'][0]}, configs {got['configs'][0]!r}, largest query "
          f"{got['max_nodes'][0]} nodes")
    assert got["status"][0] == 1
    assert got["configs"][0] == 2.0 ** W
    want = np.where(rev.reshape(-1) != 0, 0.0, 0.5)
    assert np.array_equal(bits(got["prob"][0]), bits(want))
    assert 0 < got["max_nodes"][0] < 1000
    ref = posterior_host(rev, num, W, host_budget=BUDGET)
    assert ref["status"][0] == 2 and not ref["prob"].any() and ref["configs"][0] == 0
    assert ref["max_nodes"][0] == BUDGET


@pytest.mark.parametrize("board", BOARDS)
def test_fixture_states(board):
    """2^16 nodes per query: grouped decides every state (no share is left out: a state left out
    would hide a failure), enumerate does not at expert density; bitwise equal where both decide;
    the invariants of test_posterior_host.py."""
    z, _, got = fixture_host(board, "grouped")
    _, _, ref = fixture_host(board, "enumerate")
    dec = got["status"] == 1
    both = dec & (ref["status"] == 1)
    print(f"{board}: grouped leaves {int((~dec).sum())} of {z['S']} states undecided at 2^16 nodes (largest query "
          f"{int(got['max_nodes'].max())}), enumerate {int((ref['status'] == 2).sum())} (largest decided query "
          f"{int(ref['max_nodes'][ref['status'] == 1].max())})")
    assert dec.all()
    assert ((ref["status"] == 1) | (ref["status"] == 2)).all()
    if board in ("30x16x99", "16x30x99"):
        assert (ref["status"] == 2).any()
    assert both.any()
    assert np.array_equal(bits(got["prob"][both]), bits(ref["prob"][both]))
    assert np.array_equal(bits(got["configs"][both]), bits(ref["configs"][both]))
    flat_rev, flat_mine = z["rev"].reshape(z["S"], -1), z["mine"].reshape(z["S"], -1)
    for i in range(z["S"]):
        p = got["prob"][i]
        assert abs(p.sum() - z["K"]) <= 1e-9, i
        assert (p >= 0).all() and (p <= 1).all() and not p[flat_rev[i] != 0].any(), i
        assert not p[z["safe"][i] != 0].any(), i
        assert (p[(flat_mine[i] != 0) & (flat_rev[i] == 0)] > 0).all(), i
    assert (got["configs"] >= 1).all()


def test_fixture_states_are_all_there():
    assert sum(F.load(b)["S"] for b in BOARDS) == 359


def test_edge_cases_grouped():
    from ms_amd import _lib as L
    from ms_amd.posterior import posterior_host
    rev, num = _two_cells()
    got = posterior_host(rev, num, 1, method="grouped")
    assert got["status"][0] == 1 and got["prob"][0].tolist() == [0.5, 0.5, 0, 0] and got["configs"][0] == 2
    assert got["max_nodes"][0] > 0
    for kw, r in ((dict(live=[0]), rev), ({}, np.zeros_like(rev))):
        got = posterior_host(r, num, 1, method="grouped", **kw)
        assert all(not v.any() for v in got.values()), kw
    got = posterior_host(rev, num, 1, host_budget=1, method="grouped")
    assert got["status"][0] == 2 and not got["prob"].any() and got["configs"][0] == 0 and got["max_nodes"][0] <= 1
    got = posterior_host(np.ones((1, 1, 1), dtype=np.uint8), np.zeros((1, 1, 1), dtype=np.uint8), 0, method="grouped")
    assert got["status"][0] == 1 and got["configs"][0] == 1 and not got["prob"].any()
    for bad_num, M in ((num, 3), (np.full_like(num, 3), 1), (num, 0)):
        with pytest.raises(L.MsEnvError, match="inconsistent"):
            posterior_host(rev, bad_num, M, method="grouped")


def test_bad_arguments_are_refused():
    """The three new entry points that take no handle, mirroring test_posterior_host.py, and the
    null-handle checks of the other two."""
    import ctypes

    from ms_amd import _lib as L
    lib = L.load()
    rev, num = _two_cells()
    p = lambda a: a.ctypes.data  # noqa: E731
    none4 = [None] * 4
    host = lib.ms_posterior_host_grouped
    assert host(None, p(num), 1, None, 1, 2, 2, 0, *none4) == 1
    assert b"ms_posterior_host_grouped" in lib.ms_last_error()
    assert host(p(rev), None, 1, None, 1, 2, 2, 0, *none4) == 1
    assert host(p(rev), p(num), 1, None, 0, 2, 2, 0, *none4) == 1
    assert host(p(rev), p(num), 1, None, 1, 0, 2, 0, *none4) == 1
    assert host(p(rev), p(num), 5, None, 1, 2, 2, 0, *none4) == 1
    assert host(p(rev), p(num), 1, None, 1, 2, 2, -1, *none4) == 1
    assert host(p(rev), p(num), 1, None, 1, 2, 2, 0, *none4) == 0  # every output optional
    assert host(p(rev), p(num), 2, None, 1, 2, 2, 0, *none4) == 1  # inconsistent
    assert b"inconsistent" in lib.ms_last_error()
    fake = ctypes.c_void_p(4096)  # never dereferenced: arguments are checked before any device work
    assert lib.ms_posterior_grouped(None, None, *none4, None) == 1
    assert b"ms_posterior_grouped: null handle" in lib.ms_last_error()
    assert lib.ms_posterior_labels_grouped(None, 1 << 11, None, None, None, None, None) == 1
    assert b"ms_posterior_labels_grouped: null handle" in lib.ms_last_error()
    st = lambda n, H, W, M, b, rv=fake: lib.ms_posterior_states_grouped(rv, fake, M, None, n, H, W, b, *none4, None)  # noqa: E731
    assert st(1, 3, 5, 2, 1 << 18, None) == 1
    assert b"ms_posterior_states_grouped" in lib.ms_last_error()
    assert st(0, 3, 5, 2, 1 << 18) == 1
    assert st(1, 65, 5, 2, 1 << 18) == 1 and st(1, 3, 63, 2, 1 << 18) == 1
    assert st(1, 3, 5, 16, 1 << 18) == 1 and st(1, 3, 5, -1, 1 << 18) == 1
    assert st(1, 3, 5, 2, 0) == 1
    assert b"budget" in lib.ms_last_error()


def test_grouped_table_matches_its_header():
    """SIGNATURES_GROUPED against include/msposterior_grouped.h, with the checker of
    test_abi_signatures.py; both libraries export the four functions; the ABI version stays 3."""
    import ctypes

    from conftest import PKG_DIR
    from ms_amd import _lib as L
    protos, structs, defines, diag_only = parse_headers([GROUPED_H])
    assert sorted(protos) == ["ms_posterior_grouped", "ms_posterior_host_grouped", "ms_posterior_labels_grouped",
                              "ms_posterior_states_grouped"]
    assert table_errors(L.SIGNATURES_GROUPED, L._RESTYPES, protos) == []
    assert not structs and not diag_only and not set(L.SIGNATURES_GROUPED) & set(L.SIGNATURES)
    assert defines == {"MS_POSTERIOR_MAX_GROUPS": L.MS_POSTERIOR_MAX_GROUPS}
    assert 64 <= L.MS_POSTERIOR_MAX_GROUPS <= L.MS_AVOID_MAX_VARS
    lib = L.load()
    with open(os.path.join(PKG_DIR, "libmsenv_diag.so"), "rb") as f:
        diag_image = f.read()
    for name, argtypes in L.SIGNATURES_GROUPED.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int, name
        assert argtypes == L.SIGNATURES[name[:-len("_grouped")]], name  # the counterpart's parameter list
        assert b"\0" + name.encode() + b"\0" in diag_image, f"libmsenv_diag.so lacks {name}"
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3
    # a wrong table is reported
    wrong = dict(L.SIGNATURES_GROUPED, ms_posterior_host_grouped=L.SIGNATURES["ms_posterior_states"])
    assert table_errors(wrong, L._RESTYPES, protos)


def test_unknown_method_is_a_value_error():
    """At every Python entry, before any device or library work."""
    from ms_amd.env import VecMinesweeper
    from ms_amd.eval import evaluate_vec
    from ms_amd.posterior import PosteriorModel, posterior_host, posterior_states, resolve_undecided
    from ms_amd.rollout import collect_rollout
    from ms_amd.train import main, posterior_method_param
    rev, num = _two_cells()
    no_vec = object.__new__(VecMinesweeper)  # the check comes before the handle is touched
    calls = [lambda: posterior_host(rev, num, 1, method="bogus"),
             lambda: posterior_states(None, None, 1, method="bogus"),
             lambda: resolve_undecided({}, None, None, 1, method="bogus"),
             lambda: PosteriorModel(1, method="bogus"),
             lambda: VecMinesweeper.mine_posterior(no_vec, method="bogus"),
             lambda: VecMinesweeper.resolve_posterior(no_vec, {}, method="bogus"),
             lambda: VecMinesweeper.posterior_labels(no_vec, method="bogus"),
             lambda: collect_rollout(None, None, 4, "cpu", belief_targets="posterior", posterior_method="bogus"),
             lambda: evaluate_vec(None, None, posterior=True, posterior_method="bogus"),
             lambda: posterior_method_param({"posterior_method": "bogus"}),
             lambda: posterior_method_param({}, "bogus")]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="method"):
            call()
    assert posterior_method_param({}) == "enumerate"
    assert posterior_method_param({"posterior_method": "grouped"}) == "grouped"
    assert posterior_method_param({"posterior_method": "grouped"}, "enumerate") == "enumerate"
    with pytest.raises(SystemExit):  # argparse refuses the value before anything is set up
        main(["--posterior_method", "bogus"])
