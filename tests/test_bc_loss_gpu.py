"""The HIP behaviour-cloning loss (csrc/msbc.hip via ms_amd/bc_loss.py) against the f64 restatement
of tests/bc_loss_ref.py, at the bounds of tests/test_ppo_loss_gpu.py: terms rel 1e-5 / abs 1e-6,
each gradient tensor rel-L2 1e-5, dlogits exactly 0 at masked cells and on rows of weight 0.

Shapes: A on both sides of every 64-cell slice and of the NQ dispatch (128 / 256), M of one row,
of a partial workgroup, of several workgroups, and M = 8,195 = 4 rows x MAX_GRID (2,048
workgroups, csrc/msbc.hip) + 3, where the grid-stride loop takes a second pass."""
from __future__ import annotations

import ctypes

import pytest
import torch

import bc_loss_ref as R
from ppo_loss_ref import ref_grads, rel_l2

pytestmark = pytest.mark.gpu

KW = dict(ent_coef=0.01, aux_mine_weight=0.05, aux_mine_calib_weight=0.01)
GRID_ROWS = 4 * 2048  # rows in flight of a full grid: loss_grid() of csrc/msbc.hip


def _run(b, dev, gout, *, with_mine=True, counts=None, world=1, **kw):
    """-> (terms f32 [8] on the CPU, dlogits, dmine or None) of the HIP passes for sum_k gout[k] out[k]."""
    from ms_amd.bc_loss import bc_loss_terms
    lg = b["logits"].to(dev).requires_grad_(True)
    mi = b["mine"].to(dev).requires_grad_(True) if with_mine else None
    t = bc_loss_terms(lg, mi, b["mask"].to(dev), b["best"].to(dev), b["weight"].to(dev),
                      labels=b["labels"].to(dev) if with_mine else None,
                      valid=b["valid"].to(dev) if (with_mine and b.get("valid") is not None) else None,
                      counts=None if counts is None else counts.to(dev), world=world, **kw)
    (t * torch.as_tensor(gout, dtype=torch.float32, device=dev)).sum().backward()
    return t.detach().cpu(), lg.grad.cpu(), (mi.grad.cpu() if with_mine else None)


def _absmax(t) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


def _check(b, dev, gout, *, with_mine=True, counts=None, world=1, where="", **kw):
    got, dl, dm = _run(b, dev, gout, with_mine=with_mine, counts=counts, world=world, **kw)
    terms, leaves = R.ref_terms(b, with_mine=with_mine, counts=counts, world=world, **kw)
    for k, name in enumerate(R.TERMS):
        want = float(terms[k].detach())
        print(f"{where} {name}: hip {float(got[k])!r} ref {want!r}")
        assert float(got[k]) == pytest.approx(want, rel=1e-5, abs=1e-6), (where, name)
    assert float(got[7]) == 0.0
    if any(float(g) != 0.0 and t.requires_grad for g, t in zip(gout, terms)):
        gl, gm = ref_grads(terms, leaves, gout)
    else:  # only outputs without a gradient (agree, bad_rows, the padding) carry a cotangent
        gl, gm = (None if x is None else torch.zeros_like(x) for x in leaves)
    e = rel_l2(dl, gl) if float(gl.norm()) > 0 else _absmax(dl)
    print(f"{where} dlogits rel-L2 {e:.3g}")
    assert e <= 1e-5, (where, "dlogits")
    mask, w = b["mask"].ne(0), b["weight"]
    assert _absmax(dl[~mask]) == 0.0 and _absmax(dl[w == 0]) == 0.0, where
    if with_mine:
        e = rel_l2(dm.reshape(gm.shape), gm) if float(gm.norm()) > 0 else _absmax(dm)
        print(f"{where} dmine rel-L2 {e:.3g}")
        assert e <= 1e-5, (where, "dmine")
        if b.get("valid") is not None:
            assert _absmax(dm.reshape(mask.shape)[~b["valid"].ne(0)]) == 0.0, where
    return got, dl, dm


def _gout(seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(8, generator=g) * 2).tolist()


@pytest.mark.parametrize("M", [1, 3, 130])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 81, 256, 480, 512])
def test_terms_and_gradients(gpu, A, M):
    b = R.make_batch(M, A, seed=A * 1000 + M)
    _check(b, gpu, _gout(A + M), where=f"A={A} M={M}", **KW)


def test_grid_stride_rows(gpu):
    M = GRID_ROWS + 3
    b = R.make_batch(M, 65, seed=5, w_zero_rows=(1, GRID_ROWS, M - 1))
    _check(b, gpu, _gout(5), where=f"M={M}", **KW)


def test_per_term_cotangents(gpu):
    """One basis vector of gout at a time: each output's own gradient (agree, bad_rows and the
    padding have none)."""
    b = R.make_batch(130, 81, seed=17)
    for k in range(8):
        gout = [0.0] * 8
        gout[k] = 1.5
        got, dl, dm = _check(b, gpu, gout, where=f"gout[{k}]", **KW)
        if k in (1, 6, 7):
            assert not dl.any() and not dm.any()
        if k in (0, 2):
            assert dl.any() and not dm.any()
        if k in (3, 4):
            assert dm.any() and not dl.any()


def test_without_belief_terms_and_without_valid(gpu):
    b = R.make_batch(67, 81, seed=23)
    got, _, dm = _check(b, gpu, _gout(1), with_mine=False, where="no mine", ent_coef=0.01)
    assert dm is None and float(got[3]) == 0.0 and float(got[4]) == 0.0
    b["valid"] = None  # every cell counts
    _check(b, gpu, _gout(2), where="valid=None", **KW)


def test_global_counts_and_world(gpu):
    """counts of a larger "global" minibatch and world = 4, as a data-parallel rank would pass."""
    b = R.make_batch(130, 64, seed=29)
    counts = R.local_counts(b) * torch.tensor([3.0, 2.5, 3.5])
    _check(b, gpu, _gout(3), counts=counts, world=4, where="world=4", **KW)


def test_best_of_one_cell_and_of_every_legal_cell(gpu):
    b = R.make_batch(66, 81, seed=31)
    one = torch.zeros_like(b["best"])
    first = b["mask"].float().argmax(1)
    one[torch.arange(66), first] = 1
    b["best"] = one
    got1, _, _ = _check(b, gpu, _gout(4), where="n_best=1", **KW)
    b["best"] = b["mask"].to(torch.uint8)
    got_all, _, _ = _check(b, gpu, _gout(4), where="n_best=legal", **KW)
    assert float(got_all[1]) == pytest.approx(1.0, rel=1e-6)  # the argmax is always a legal cell
    assert float(got1[1]) < 1.0


def test_agree_breaks_logit_ties_by_the_lowest_index(gpu):
    """Rows whose maximum is attained twice (bitwise): only the lower of the two cells counts."""
    M, A = 8, 130
    b = R.make_batch(M, A, seed=37, w_zero_rows=())
    b["mask"][:] = True
    b["weight"][:] = 1.0
    lo, hi = [3, 3, 64, 70, 0, 63, 5, 100], [7, 64, 65, 129, 129, 64, 128, 101]
    best = torch.zeros(M, A, dtype=torch.uint8)
    for r in range(M):
        b["logits"][r, lo[r]] = b["logits"][r, hi[r]] = 50.0
        best[r, hi[r] if r % 2 else lo[r]] = 1  # odd rows mark only the higher cell: no agreement
    b["best"] = best
    b["valid"] = b["valid"] & b["mask"]
    got, _, _ = _check(b, gpu, _gout(6), where="ties", **KW)
    assert float(got[1]) == pytest.approx(0.5, rel=1e-6)


def test_empty_weight_sum_gives_zero_terms(gpu):
    b = R.make_batch(20, 65, seed=41)
    b["weight"][:] = 0.0
    got, dl, dm = _check(b, gpu, _gout(7), where="all w=0", **KW)
    assert got[:3].tolist() == [0.0, 0.0, 0.0] and not dl.any() and dm.any()
    # counts[0] = 0 handed in with non-zero weights: still 0, not NaN or inf
    b = R.make_batch(20, 65, seed=43)
    counts = R.local_counts(b)
    counts[0] = 0.0
    got, dl, _ = _check(b, gpu, _gout(8), counts=counts, where="counts[0]=0", **KW)
    assert got[:3].tolist() == [0.0, 0.0, 0.0] and not dl.any() and bool(torch.isfinite(got).all())


def test_valid_all_zero(gpu):
    b = R.make_batch(33, 81, seed=47)
    b["valid"][:] = False
    got, _, dm = _check(b, gpu, _gout(9), where="valid=0", **KW)
    assert float(got[3]) == 0.0 and float(got[4]) == 0.0 and not dm.any()


def test_exact_labels(gpu):
    """Labels of exactly 0, 1 and 2^-24 (the smallest posterior a 16x16 board's f32 label holds
    apart from 0 is far larger; 2^-24 is half an f32 ulp of 1)."""
    b = R.make_batch(40, 96, seed=53)
    vals = torch.tensor([0.0, 1.0, 2.0 ** -24])
    b["labels"] = vals[torch.arange(40 * 96).reshape(40, 96) % 3]
    _check(b, gpu, _gout(10), where="exact labels", **KW)


def test_weight_zero_rows_are_not_read(gpu):
    """NaN logits on a row of weight 0 reach nothing: finite terms, and that row's dlogits are 0."""
    b = R.make_batch(12, 81, seed=59, w_zero_rows=(1, 5))
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    b["logits"][1] = float("nan")
    b["logits"][5, ::2] = float("inf")
    b["best"][5] = 0  # an empty best on an excluded row is not a bad row
    gout = _gout(11)
    got, dl, dm = _run(b, gpu, gout, **KW)
    want, wdl, wdm = _run(clean, gpu, gout, **KW)
    assert bool(torch.isfinite(got).all()) and float(got[6]) == 0.0
    assert torch.equal(got, want) and torch.equal(dl, wdl) and torch.equal(dm, wdm)
    assert not dl[1].any() and not dl[5].any()


def test_bad_rows_are_counted_and_do_not_touch_other_rows(gpu):
    """An empty best and a best bit on a masked cell, on rows of weight > 0: both counted in [6],
    policy_ce and loss NaN, those rows' dlogits NaN at their legal cells and 0 at masked ones; every
    other row's gradients, and the terms that do not involve best, are what they are when the two
    rows are excluded by weight 0 under the same counts."""
    M, A = 30, 81
    b = R.make_batch(M, A, seed=61, w_zero_rows=(1,))
    counts = R.local_counts(b)
    bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    bad["best"][4] = 0
    masked = int((~b["mask"][9]).float().argmax())
    assert not b["mask"][9, masked]
    bad["best"][9, masked] = 1
    gout = _gout(12)
    got, dl, dm = _run(bad, gpu, gout, counts=counts, **KW)
    excl = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    excl["weight"][4] = excl["weight"][9] = 0.0
    want, wdl, wdm = _run(excl, gpu, gout, counts=counts, **KW)
    assert float(got[6]) == 2.0 and float(want[6]) == 0.0
    assert bool(torch.isnan(got[0])) and bool(torch.isnan(got[5]))
    assert torch.equal(got[3:5], want[3:5])
    others = [r for r in range(M) if r not in (4, 9)]
    assert torch.equal(dl[others], wdl[others]) and torch.equal(dm, wdm)
    for r in (4, 9):
        legal = b["mask"][r]
        assert bool(torch.isnan(dl[r][legal]).all()) and not dl[r][~legal].any()
    ref = R.ref_terms(bad, counts=counts, **KW)[0]
    assert float(ref[6]) == 2.0 and bool(torch.isnan(ref[0]))


def test_two_runs_are_bitwise_equal(gpu):
    b = R.make_batch(GRID_ROWS + 3, 256, seed=67)
    gout = _gout(13)
    x, y = _run(b, gpu, gout, **KW), _run(b, gpu, gout, **KW)
    for p, q in zip(x, y):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))


def test_sixteen_bit_logits_use_the_short_mask_fill(gpu):
    """fp16 logits: read as f32 with masked cells at -1e4 (as the PPO loss does)."""
    b = R.make_batch(50, 81, seed=71)
    b["logits"] = b["logits"].half().float()
    h = dict(b, logits=b["logits"].half())
    got, dl, _ = _run(h, gpu, _gout(14), **KW)
    terms, leaves = R.ref_terms(b, mask_fill=-1e4, **KW)
    for k in range(7):
        assert float(got[k]) == pytest.approx(float(terms[k].detach()), rel=1e-5, abs=1e-6), R.TERMS[k]
    assert dl.dtype == torch.float16 or dl.dtype == torch.float32


def test_c_api_refuses_bad_arguments(gpu):
    """A = 0, A = 513, M < 0 and NULL logits, with real device tensors behind every other pointer."""
    from ms_amd import _lib as L
    lib = L.load()
    M, A = 4, 16
    t = {k: torch.zeros(M * 513, dtype=dt, device=gpu) for k, dt in
         (("logits", torch.float32), ("action_mask", torch.uint8), ("best", torch.uint8), ("weight", torch.float32),
          ("counts", torch.float32))}
    out = torch.zeros(8, device=gpu)
    ws = int(lib.mc_bc_loss_workspace(M))
    work = torch.zeros(ws, device=gpu)
    a = L.McBcLossArgs()
    for k, v in t.items():
        setattr(a, k, L.ptr(v))
    a.mask_fill, a.world = -1e9, 1.0
    for m, n, null_logits in ((M, 0, False), (M, 513, False), (-1, A, False), (M, A, True)):
        a.M, a.A, a.logits = m, n, (None if null_logits else L.ptr(t["logits"]))
        assert lib.mc_bc_loss_fwd(ctypes.byref(a), L.ptr(out), L.ptr(work), ws, L.stream_ptr(gpu)) == 1
        assert b"mc_bc_loss_fwd: bad argument" in lib.mc_last_error()
        assert lib.mc_bc_loss_bwd(ctypes.byref(a), L.ptr(out), L.ptr(work), ws, L.ptr(t["logits"]), None,
                                  L.stream_ptr(gpu)) == 1
    a.M, a.A, a.logits = M, A, L.ptr(t["logits"])
    assert lib.mc_bc_loss_fwd(ctypes.byref(a), L.ptr(out), L.ptr(work), ws - 1, L.stream_ptr(gpu)) == 1
    a.mine = L.ptr(t["logits"])  # mine logits without labels
    assert lib.mc_bc_loss_fwd(ctypes.byref(a), L.ptr(out), L.ptr(work), ws, L.stream_ptr(gpu)) == 1
