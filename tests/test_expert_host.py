"""Expert targets on the host (include/msexpert.h: ms_expert_targets_host) against a numpy
restatement on hand-made rows and on the fixture states of tests/golden/avoid_states.npz, the
argument checks, and the ctypes tables of the two new headers (msexpert.h, msbc.h) against the
headers. No device needed."""
from __future__ import annotations

import ctypes
import itertools
import os

import numpy as np
import pytest

import expert_rows as X
from conftest import PKG_DIR, ROOT
from test_abi_signatures import SCALARS, parse_headers, table_errors
from test_posterior_grouped_host import BOARDS, fixture_host

EXPERT_H = os.path.join(ROOT, "include", "msexpert.h")
BC_H = os.path.join(ROOT, "include", "msbc.h")


def test_new_tables_match_their_headers(monkeypatch):
    """SIGNATURES_EXPERT / SIGNATURES_BC against include/msexpert.h / include/msbc.h with the
    checker of test_abi_signatures.py; the args struct mirror field by field; both libraries
    export every new function; the ABI version stays 3."""
    import test_abi_signatures as S
    from ms_amd import _lib as L
    lib = L.load()
    # the checker resolves `mc_bc_loss_args*` through its list of struct mirrors: add the new one
    # (checked field by field below)
    seven = S._mirrors()
    monkeypatch.setattr(S, "_mirrors", lambda: dict(seven, mc_bc_loss_args=L.McBcLossArgs))
    with open(os.path.join(PKG_DIR, "libmsenv_diag.so"), "rb") as f:
        diag_image = f.read()
    for header, table, names in ((EXPERT_H, L.SIGNATURES_EXPERT, ["ms_expert_targets", "ms_expert_targets_host"]),
                                 (BC_H, L.SIGNATURES_BC, ["mc_bc_loss_bwd", "mc_bc_loss_fwd", "mc_bc_loss_workspace"])):
        protos, structs, defines, diag_only = parse_headers([header])
        assert sorted(protos) == names
        assert table_errors(table, L._RESTYPES, protos) == []
        assert not diag_only and not set(table) & set(L.SIGNATURES) and not set(table) & set(L.SIGNATURES_GROUPED)
        for name, argtypes in table.items():
            fn = getattr(lib, name)
            assert list(fn.argtypes) == argtypes and fn.restype is L._RESTYPES.get(name, ctypes.c_int), name
            assert b"\0" + name.encode() + b"\0" in diag_image, f"libmsenv_diag.so lacks {name}"
        if header == EXPERT_H:
            assert not structs
            assert defines == {"MS_EXPERT_NONE": L.MS_EXPERT_NONE, "MS_EXPERT_SAFE": L.MS_EXPERT_SAFE,
                               "MS_EXPERT_GUESS": L.MS_EXPERT_GUESS}
            wrong = dict(table, ms_expert_targets_host=table["ms_expert_targets"])
        else:
            assert set(structs) == {"mc_bc_loss_args"} and not defines
            got = L.McBcLossArgs._fields_
            assert [f for f, _ in got] == [f for _, f in structs["mc_bc_loss_args"]]
            for (ct, fname), (_, ft) in zip(structs["mc_bc_loss_args"], got):
                want = ctypes.c_void_p if ct.endswith("*") else SCALARS[ct]
                assert ft is want, f"mc_bc_loss_args.{fname}: `{ct}` is mirrored as {ft.__name__}"
            args = L.McBcLossArgs  # 8 pointers, 5 floats, (pad), int64, int32
            assert ctypes.sizeof(args) == 104 and args.M.offset == 88 and args.A.offset == 96
            wrong = dict(table, mc_bc_loss_workspace=[ctypes.c_int32])
        assert table_errors(wrong, L._RESTYPES, protos)  # a wrong table is reported
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3
    assert lib.mc_bc_loss_workspace(0) == -1 and lib.mc_bc_loss_workspace(32768) == 2048 * 8 + 32768 * 4


@pytest.mark.parametrize("A", X.SIZES)
def test_hand_rows_equal_the_numpy_restatement(A):
    from ms_amd.expert import expert_targets_host
    status, prob, hidden, names = X.hand_rows(A)
    got = expert_targets_host({"status": status, "prob": prob}, hidden)
    want = X.numpy_targets(status, prob, hidden)
    for k in X.OUTPUTS:
        assert got[k].dtype == want[k].dtype, k
        for i, name in enumerate(names):
            assert np.array_equal(got[k][i].view(np.uint8) if k == "labels" else got[k][i],
                                  want[k][i].view(np.uint8) if k == "labels" else want[k][i]), (A, name, k)
    row = dict(zip(names, range(len(names))))
    assert got["action"][row["single minimum at the last cell"]] == A - 1
    assert got["n_best"][row["all hidden cells tied"]] == A and got["action"][row["all hidden cells tied"]] == 0
    assert got["n_best"][row["one hidden cell"]] == 1 and got["action"][row["one hidden cell"]] == A // 2
    assert got["kind"][row["several exact zeros: a safe move"]] == 1
    assert got["n_best"][row["several exact zeros: a safe move"]] == len(range(0, A, 3))
    assert got["kind"][row["smallest subnormal: a forced guess"]] == 2
    if A > 1:
        i = row["revealed zero"]
        assert got["best"][i, 0] == 0 and got["kind"][i] == 2 and got["action"][i] > 0
    for name in ("status 0", "status 2", "nothing hidden"):
        i = row[name]
        assert got["kind"][i] == 0 and got["action"][i] == -1 and got["n_best"][i] == 0, name
        assert not got["best"][i].any() and not got["labels"][i].any(), name


def test_every_null_output_combination():
    from ms_amd import _lib as L
    lib = L.load()
    status, prob, hidden, _ = X.hand_rows(65)
    n, A = prob.shape
    want = X.numpy_targets(status, prob, hidden)
    dts = dict(best=np.uint8, action=np.int64, kind=np.uint8, n_best=np.int32, labels=np.float32)
    for keep in itertools.product((False, True), repeat=5):
        out = {k: np.full((n, A) if k in ("best", "labels") else (n,), 7, dts[k]) for k in X.OUTPUTS}
        ptrs = [out[k].ctypes.data if on else None for k, on in zip(X.OUTPUTS, keep)]
        assert lib.ms_expert_targets_host(status.ctypes.data, prob.ctypes.data, hidden.ctypes.data, n, A, *ptrs) == 0
        for k, on in zip(X.OUTPUTS, keep):
            assert np.array_equal(out[k], want[k]) if on else (out[k] == 7).all(), (keep, k)


def test_bad_arguments_are_refused():
    from ms_amd import _lib as L
    lib = L.load()
    status, prob, hidden, _ = X.hand_rows(9)
    p = lambda a: a.ctypes.data  # noqa: E731
    none5 = [None] * 5
    host = lib.ms_expert_targets_host
    assert host(None, p(prob), p(hidden), 1, 9, *none5) == 1
    assert b"ms_expert_targets_host" in lib.ms_last_error()
    assert host(p(status), None, p(hidden), 1, 9, *none5) == 1
    assert host(p(status), p(prob), None, 1, 9, *none5) == 1
    assert host(p(status), p(prob), p(hidden), 0, 9, *none5) == 1
    assert host(p(status), p(prob), p(hidden), 1, 0, *none5) == 1
    assert host(p(status), p(prob), p(hidden), 1, 513, *none5) == 1
    assert b"512" in lib.ms_last_error()
    assert host(p(status), p(prob), p(hidden), 1, 9, *none5) == 0
    fake = ctypes.c_void_p(4096)  # never dereferenced: arguments are checked before any device work
    dev = lib.ms_expert_targets
    assert dev(None, fake, fake, 1, 9, *none5, None) == 1
    assert b"ms_expert_targets:" in lib.ms_last_error()
    assert dev(fake, fake, fake, 0, 9, *none5, None) == 1 and dev(fake, fake, fake, 1 << 31, 9, *none5, None) == 1
    assert dev(fake, fake, fake, 1, 0, *none5, None) == 1 and dev(fake, fake, fake, 1, 513, *none5, None) == 1
    # the loss entry points refuse A = 0, A = 513, M < 0 and NULL logits before anything touches the device
    a = L.McBcLossArgs()
    for f in ("logits", "action_mask", "best", "weight", "counts"):
        setattr(a, f, 4096)
    ws = 1 << 20

    def fwd_bwd(M, A, logits=4096):
        a.M, a.A, a.logits = M, A, logits
        return (lib.mc_bc_loss_fwd(ctypes.byref(a), fake, fake, ws, None),
                lib.mc_bc_loss_bwd(ctypes.byref(a), fake, fake, ws, fake, None, None))
    for M, A, lg in ((4, 0, 4096), (4, 513, 4096), (-1, 16, 4096), (0, 16, 4096), (4, 16, None)):
        assert fwd_bwd(M, A, lg) == (1, 1), (M, A, lg)
        assert b"mc_bc_loss_bwd: bad argument" in lib.mc_last_error()
    a.M, a.A, a.logits = 4, 16, 4096
    assert lib.mc_bc_loss_fwd(ctypes.byref(a), fake, fake, 10, None) == 1  # workspace too small
    assert lib.mc_bc_loss_fwd(None, fake, fake, ws, None) == 1


@pytest.mark.parametrize("board", BOARDS)
def test_fixture_states(board):
    """Every fixture state is decided by the grouped host solver at 2^16 nodes
    (tests/test_posterior_grouped_host.py), so every state with a hidden cell has a target: none
    may come back kind 0. Where the reference's avoidability analysis found provably safe cells,
    the move is safe and those cells are all in best (they have p = 0)."""
    from ms_amd.expert import expert_targets_host
    z, _, post = fixture_host(board, "grouped")
    S = z["S"]
    hidden = (z["rev"].reshape(S, -1) == 0).astype(np.uint8)
    got = expert_targets_host(post, hidden)
    want = X.numpy_targets(post["status"], post["prob"], hidden)
    for k in X.OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
    has_target = (post["status"] == 1) & hidden.any(axis=1)
    none = int((has_target & (got["kind"] == 0)).sum())
    safe = z["safe"].reshape(S, -1) != 0
    with_safe = safe.any(axis=1)
    print(f"{board}: {S} states, {int(has_target.sum())} decided with a hidden cell, {none} of them kind 0; kinds "
          f"{np.bincount(got['kind'], minlength=3).tolist()}; {int(with_safe.sum())} states with a fixture safe cell")
    assert has_target.all() and none == 0
    rows = np.arange(S)
    assert (got["best"][rows, got["action"]] == 1).all()
    assert not (got["best"].astype(bool) & ~hidden.astype(bool)).any()
    assert np.array_equal(got["n_best"], got["best"].sum(axis=1))
    assert (got["kind"][with_safe] == 1).all()
    assert not (safe & ~got["best"].astype(bool))[with_safe].any()
    # a kind-1 move is never a mine; a kind-2 state has no p = 0 cell
    mine = z["mine"].reshape(S, -1) != 0
    k1 = got["kind"] == 1
    assert not mine[rows[k1], got["action"][k1]].any()
    assert (np.where(hidden.astype(bool), post["prob"], 1.0).min(axis=1)[got["kind"] == 2] > 0).all()


def test_shipped_imitation_config_and_early_argument_checks():
    """configs/imitation/16x16x40_medium.yaml gives the Trainer the training config's env and
    model and a complete imitation section; an unknown imitation key, a bad method and a bad
    explore raise before any device work."""
    from ms_amd.imitate import collect_expert, imitation_params
    from ms_amd.train import load_config
    cfg, env_d, model_d, extras = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium.yaml"))
    _, tenv, tmodel, _ = load_config(os.path.join(ROOT, "configs", "training", "16x16x40_medium.yaml"))
    assert env_d == tenv and model_d == tmodel and (cfg.H, cfg.W, cfg.mine_count) == (16, 16, 40)
    il = imitation_params(extras)
    assert il == imitation_params({"imitation": dict(il)}) and il["method"] == "grouped"
    assert set(il) == set(imitation_params({})) and 1 <= il["budget"] <= 1 << 30
    with pytest.raises(ValueError, match="unknown"):
        imitation_params({"imitation": {"guess_wieght": 0.0}})
    with pytest.raises(ValueError, match="method"):
        collect_expert(None, 4, budget=16, method="bogus", seed=0)
    with pytest.raises(ValueError, match="explore"):
        collect_expert(None, 4, budget=16, explore=1.5, seed=0)
