"""The avoidability analysis on the host (include/mssolve.h: ms_avoid_host, the plain C++ solver
that is also the exact fallback for boards the device search leaves undecided) against the
reference's analyze_avoidability on tests/golden/avoid_states.npz, on hand-made states whose
answers are plain, and the argument checks of the whole mssolve.h ABI. No device needed."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import avoid_fixture as F
from conftest import ROOT


def test_fixture_meets_its_quotas():
    assert F.boards() == ("9x9x10", "16x16x40", "30x16x99", "16x30x99")
    for b in F.boards():
        z = F.load(b)
        cls = z["cls"]
        assert z["S"] <= 120
        assert (cls == F.CLS_PROP).sum() >= 16 and (cls == F.CLS_EXACT_SAFE).sum() >= 8
        assert (cls == F.CLS_FORCED).sum() >= 8
        flat = z["rev"].reshape(z["S"], -1)
        assert flat[np.arange(z["S"]), z["chosen"]].any(), "no revealed chosen cell"
        assert (z["chosen_comp"] == 0).any() and (z["chosen_comp"] > 0).any()
    assert os.path.getsize(os.path.join(F.GOLDEN, "avoid_states.npz")) < 100_000


@pytest.mark.parametrize("board", ["9x9x10", "16x16x40", "30x16x99", "16x30x99"])
def test_host_solver_matches_reference(board):
    from ms_amd.avoid import avoid_host
    z = F.load(board)
    got = avoid_host(z["rev"], z["mine"], z["chosen"])
    F.assert_matches_reference(got, z, where=board)


def _wall():
    """Rows 1-2 revealed under a hidden row 0 with mines over columns 1 and 3: the counts read
    1 1 2 1 1, and subset + unit rules alone give safe {0, 2, 4} and mines {1, 3}."""
    rev = np.zeros((1, 3, 5), dtype=np.uint8)
    rev[0, 1:] = 1
    mine = np.zeros((1, 3, 5), dtype=np.uint8)
    mine[0, 0, [1, 3]] = 1
    return rev, mine


def test_hand_made_states():
    from ms_amd.avoid import avoid_host
    rev, mine = _wall()
    # before the first click, or not live: not analysed
    for kw in (dict(first_click=[0]), dict(live=[0])):
        got = avoid_host(rev, mine, [2], **kw)
        assert all(int(v.sum()) == 0 for v in got.values())
    # all hidden after the first click: nothing to reason from, the pick is a lone guess
    hid = np.zeros((1, 3, 5), dtype=np.uint8)
    got = avoid_host(hid, mine, [7], first_click=[1])
    assert (got["status"][0], got["avoidable"][0], got["chosen_comp"][0]) == (1, 0, 1)
    assert got["n_frontier"][0] == 0 and got["n_comp"][0] == 0 and got["max_nodes"][0] == 0
    # a revealed chosen cell belongs to no component
    got = avoid_host(rev, mine, [7])
    assert got["chosen_comp"][0] == 0 and got["chosen_safe"][0] == 0 and got["avoidable"][0] == 1
    # the wall: the closure alone finds the three safe cells, no search runs
    for chosen, safe in ((0, 1), (1, 0), (2, 1), (4, 1), (-13, 1), (15 + 3, 0)):  # wrapped like actions
        got = avoid_host(rev, mine, [chosen])
        assert got["status"][0] == 1 and got["avoidable"][0] == 1 and got["n_safe"][0] == 3
        assert got["safe_mask"][0].tolist() == [1, 0, 1, 0, 1] + [0] * 10
        assert got["chosen_safe"][0] == safe
        assert got["chosen_comp"][0] == 5 and got["n_comp"][0] == 1 and got["n_frontier"][0] == 5
        assert got["comp_size"][0].tolist() == [5] * 5 + [0] * 10
        assert got["max_nodes"][0] == 0


def test_search_only_state():
    """Two hidden cells over a revealed row reading 1 1: one mine among them and nothing else
    known. The closure finds nothing, the search runs and proves nothing: a forced guess."""
    from ms_amd.avoid import avoid_host
    rev = np.zeros((1, 2, 2), dtype=np.uint8)
    rev[0, 1] = 1
    mine = np.zeros((1, 2, 2), dtype=np.uint8)
    mine[0, 0, 0] = 1
    got = avoid_host(rev, mine, [0])
    assert (got["status"][0], got["avoidable"][0], got["n_safe"][0]) == (1, 0, 0)
    assert got["chosen_comp"][0] == 2 and got["max_nodes"][0] >= 2


def test_bad_arguments_are_refused():
    import ctypes

    from ms_amd import _lib as L
    from ms_amd.avoid import avoid_host
    lib = L.load()
    rev, mine = _wall()
    ch = np.zeros(1, dtype=np.int64)
    p = lambda a: a.ctypes.data  # noqa: E731
    none10 = [None] * 10
    assert lib.ms_avoid_host(None, p(mine), None, p(ch), None, 1, 3, 5, *none10) == 1
    assert b"ms_avoid_host" in lib.ms_last_error()
    assert lib.ms_avoid_host(p(rev), p(mine), None, p(ch), None, 0, 3, 5, *none10) == 1
    assert lib.ms_avoid_host(p(rev), p(mine), None, p(ch), None, 1, 0, 5, *none10) == 1
    assert lib.ms_avoid_host(p(rev), p(mine), None, p(ch), None, 1, 3, 5, *none10) == 0  # every output optional
    # the device entry points check their arguments before any device work (fake pointers are
    # never dereferenced)
    fake = ctypes.c_void_p(4096)
    assert lib.ms_avoid(None, fake, None, *none10, None) == 1
    assert b"null handle" in lib.ms_last_error()
    assert lib.ms_avoid_set_budget(None, 100) == 1
    st = lambda n, H, W, b, rv=fake: lib.ms_avoid_states(rv, fake, None, fake, None, n, H, W, b, *none10, None)  # noqa: E731
    assert st(1, 3, 5, 1 << 18, None) == 1
    assert st(0, 3, 5, 1 << 18) == 1
    assert st(1, 65, 5, 1 << 18) == 1 and st(1, 3, 63, 1 << 18) == 1
    assert st(1, 3, 5, 0) == 1
    assert b"budget" in lib.ms_last_error()
    with pytest.raises(ValueError):
        avoid_host(rev, mine[:, :2], [0])
    with pytest.raises(ValueError):
        avoid_host(rev, mine, [0, 1])


def test_library_exports_every_solver_header_symbol():
    from ms_amd import _lib as L
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mssolve.h")).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(ms_[a-z0-9_]+)\s*\(", src)))
    assert fns == ["ms_avoid", "ms_avoid_host", "ms_avoid_set_budget", "ms_avoid_states"]
    for name in fns:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
