"""The exact posterior on the host (include/msposterior.h: ms_posterior_host, the plain C++ twin
of the device kernel and the fallback for boards it leaves undecided) against brute-force
enumeration (posterior_ref.py), closed forms, invariants on tests/golden/avoid_states.npz, and
the argument checks of the whole msposterior.h ABI. No device needed."""
from __future__ import annotations

import math
import os
import re

import numpy as np
import pytest

import avoid_fixture as F
import posterior_ref as R
from conftest import ROOT


def test_oracle_set_meets_its_quotas():
    """Asserted from the oracle alone, so the equality test below cannot pass by omission."""
    st = R.oracle_states()
    for shape in R.SHAPES:
        assert sum((s["H"], s["W"], s["M"]) == shape for s in st) >= 10, shape
    assert any(s["n_comp"] >= 2 for s in st)
    assert any(s["U"] == 0 for s in st) and any(s["U"] > 0 for s in st)
    assert any(s["by_count"] for s in st), "no cell is decided through the global mine count alone"
    assert all(sum(s["counts"]) == s["M"] * s["configs"] for s in st)  # sum of p = M, exactly


def test_host_equals_brute_force():
    from ms_amd.posterior import posterior_host
    worst_p = worst_z = 0.0
    for (H, W, M), (rev, number, p, configs) in R.by_shape(R.oracle_states()).items():
        got = posterior_host(rev, number, M)
        assert (got["status"] == 1).all(), (H, W, M)
        worst_p = max(worst_p, float(np.abs(got["prob"] - p).max()))
        worst_z = max(worst_z, float((np.abs(got["configs"] - configs) / configs).max()))
        assert not got["prob"][rev.reshape(len(rev), -1) != 0].any()
    print(f"worst |p - oracle| {worst_p:.3g}, worst relative configs error {worst_z:.3g}")
    assert worst_p <= 1e-12 and worst_z <= 1e-12


@pytest.mark.parametrize("H,W,M", [(16, 16, 40), (30, 16, 99), (16, 32, 256)])
def test_closed_forms_one_revealed_cell(H, W, M):
    """One revealed cell showing t with d hidden neighbours: neighbours t/d, interior cells
    (M-t)/(A-1-d), configs C(d,t) C(A-1-d, M-t) (up to C(503, 254): the overflow range)."""
    from ms_amd.posterior import posterior_host
    A = H * W
    cells = [(0, 0), (0, W // 2), (H // 2, W // 2), (H - 1, W - 1)]
    cases = [(r, c, t) for r, c in cells for t in range(0, len(R.neighbours(H, W, r * W + c)) + 1, 2)]
    rev = np.zeros((len(cases), H, W), dtype=np.uint8)
    num = np.full((len(cases), H, W), 77, dtype=np.uint8)
    for k, (r, c, t) in enumerate(cases):
        rev[k, r, c] = 1
        num[k, r, c] = t
    got = posterior_host(rev, num, M)
    for k, (r, c, t) in enumerate(cases):
        nb = R.neighbours(H, W, r * W + c)
        d = len(nb)
        want = np.full(A, (M - t) / (A - 1 - d))
        want[nb] = t / d
        want[r * W + c] = 0.0
        assert got["status"][k] == 1
        assert np.abs(got["prob"][k] - want).max() <= 1e-12, (r, c, t)
        z = math.comb(d, t) * math.comb(A - 1 - d, M - t)
        assert abs(got["configs"][k] - z) <= 1e-12 * z, (r, c, t, got["configs"][k], z)
        assert abs(got["prob"][k].sum() - M) <= 1e-9


@pytest.mark.parametrize("board", ["9x9x10", "16x16x40", "30x16x99", "16x30x99"])
def test_fixture_invariants(board):
    """Every fixture state the host decides within 2^26 nodes per query: sum of p = M, the
    reference's provably safe cells have p = 0 exactly, every true mine has p > 0."""
    from ms_amd.posterior import posterior_host
    z = F.load(board)
    num = _numbers(z["mine"])
    got = posterior_host(z["rev"], num, z["K"], host_budget=1 << 26)
    dec = got["status"] == 1
    print(f"{board}: {int((~dec).sum())} of {z['S']} states undecided on the host at 2^26 nodes, "
          f"largest query {int(got['max_nodes'].max())} nodes")
    assert ((got["status"] == 1) | (got["status"] == 2)).all() and dec.any()
    flat_rev, flat_mine = z["rev"].reshape(z["S"], -1), z["mine"].reshape(z["S"], -1)
    for i in np.flatnonzero(dec):
        p = got["prob"][i]
        assert abs(p.sum() - z["K"]) <= 1e-9, i
        assert (p >= 0).all() and (p <= 1).all() and not p[flat_rev[i] != 0].any(), i
        assert not p[z["safe"][i] != 0].any(), i
        assert (p[(flat_mine[i] != 0) & (flat_rev[i] == 0)] > 0).all(), i
    assert not got["prob"][~dec].any() and not got["configs"][~dec].any()


def _numbers(mine):
    m = np.pad(mine.astype(np.uint8), ((0, 0), (1, 1), (1, 1)))
    H, W = mine.shape[1:]
    return sum(m[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)).astype(np.uint8)


def _two_cells():
    """Two hidden cells over a revealed row reading 1 1: one mine among them."""
    rev = np.zeros((1, 2, 2), dtype=np.uint8)
    rev[0, 1] = 1
    num = np.ones((1, 2, 2), dtype=np.uint8)
    return rev, num


def test_edge_cases():
    from ms_amd import _lib as L
    from ms_amd.posterior import posterior_host
    rev, num = _two_cells()
    got = posterior_host(rev, num, 1)
    assert got["status"][0] == 1 and got["prob"][0].tolist() == [0.5, 0.5, 0, 0] and got["configs"][0] == 2
    assert got["max_nodes"][0] > 0
    # not live, or nothing revealed: skipped, zero outputs
    for kw, r in ((dict(live=[0]), rev), ({}, np.zeros_like(rev))):
        got = posterior_host(r, num, 1, **kw)
        assert all(not v.any() for v in got.values()), kw
    # a budget the search cannot meet: undecided, zero probabilities
    got = posterior_host(rev, num, 1, host_budget=2)
    assert got["status"][0] == 2 and not got["prob"].any() and got["configs"][0] == 0
    # everything revealed
    got = posterior_host(np.ones((1, 1, 1), dtype=np.uint8), np.zeros((1, 1, 1), dtype=np.uint8), 0)
    assert got["status"][0] == 1 and got["configs"][0] == 1 and not got["prob"].any()
    # inconsistent boards: too many mines for the hidden cells, a number no layout reproduces
    for bad_num, M in ((num, 3), (np.full_like(num, 3), 1), (num, 0)):
        with pytest.raises(L.MsEnvError, match="inconsistent"):
            posterior_host(rev, bad_num, M)
    with pytest.raises(ValueError):
        posterior_host(rev, num[:, :1], 1)
    with pytest.raises(ValueError):
        posterior_host(rev[0], num[0], 1)
    with pytest.raises(ValueError):
        posterior_host(rev, num, 1, live=[1, 1])


def test_bad_arguments_are_refused():
    import ctypes

    from ms_amd import _lib as L
    lib = L.load()
    rev, num = _two_cells()
    p = lambda a: a.ctypes.data  # noqa: E731
    none4 = [None] * 4
    assert lib.ms_posterior_host(None, p(num), 1, None, 1, 2, 2, 0, *none4) == 1
    assert b"ms_posterior_host" in lib.ms_last_error()
    assert lib.ms_posterior_host(p(rev), None, 1, None, 1, 2, 2, 0, *none4) == 1
    assert lib.ms_posterior_host(p(rev), p(num), 1, None, 0, 2, 2, 0, *none4) == 1
    assert lib.ms_posterior_host(p(rev), p(num), 1, None, 1, 0, 2, 0, *none4) == 1
    assert lib.ms_posterior_host(p(rev), p(num), 5, None, 1, 2, 2, 0, *none4) == 1
    assert lib.ms_posterior_host(p(rev), p(num), 1, None, 1, 2, 2, -1, *none4) == 1
    assert lib.ms_posterior_host(p(rev), p(num), 1, None, 1, 2, 2, 0, *none4) == 0  # every output optional
    assert lib.ms_posterior_host(p(rev), p(num), 2, None, 1, 2, 2, 0, *none4) == 1  # inconsistent
    assert b"inconsistent" in lib.ms_last_error()
    # the device entry points check their arguments before any device work (fake pointers are
    # never dereferenced)
    fake = ctypes.c_void_p(4096)
    assert lib.ms_posterior(None, None, *none4, None) == 1
    assert b"null handle" in lib.ms_last_error()
    assert lib.ms_posterior_set_budget(None, 100) == 1
    st = lambda n, H, W, M, b, rv=fake: lib.ms_posterior_states(rv, fake, M, None, n, H, W, b, *none4, None)  # noqa: E731
    assert st(1, 3, 5, 2, 1 << 18, None) == 1
    assert st(0, 3, 5, 2, 1 << 18) == 1
    assert st(1, 65, 5, 2, 1 << 18) == 1 and st(1, 3, 63, 2, 1 << 18) == 1
    assert st(1, 3, 5, 16, 1 << 18) == 1 and st(1, 3, 5, -1, 1 << 18) == 1
    assert st(1, 3, 5, 2, 0) == 1
    assert b"budget" in lib.ms_last_error()


def test_library_exports_every_posterior_header_symbol():
    from ms_amd import _lib as L
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msposterior.h")).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(ms_[a-z0-9_]+)\s*\(", src)))
    assert fns == ["ms_posterior", "ms_posterior_host", "ms_posterior_set_budget", "ms_posterior_states"]
    for name in fns:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3
