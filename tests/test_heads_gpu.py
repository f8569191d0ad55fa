"""The heads kernels (csrc/msheads.hip: k_heads_fwd, k_heads_bwd, k_heads_reduce) against the f64
reference of tests/heads_ref.py, bit for bit, on inputs on which f32 arithmetic is exact (see that
module): through the C ABI (mc_heads_fwd, mc_heads_bwd) and through ms_amd.fused.heads_apply, in
bf16 and fp16. Every comparison is torch.equal; the only set comparisons are the NaN tests'.

The shapes come from the device's CU count (the backward runs one workgroup per CU), read from
mc_heads_bwd_workspace; each assertion message carries the tile count ntiles, the workgroup count
G and the range of per-workgroup tile counts nloc that the shape gave on this device."""
from __future__ import annotations

import gc

import pytest
import torch

import heads_ref as R

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float16]
GUARD = 64  # sentinel rows behind every row-indexed output
CUS_SHAPES = 256  # parametrize ids are built without a device; the shapes are rebuilt from the real count


@pytest.fixture(scope="module")
def cus(gpu):
    from ms_amd import _lib as L
    n = int(L.load().mc_heads_bwd_workspace(1 << 30))
    assert n > 0 and n % R.PART == 0
    return n // R.PART


def _geo(M, P, cus):
    nt, G, lo, hi = R.geometry(M, cus)
    return f"M {M} P {P} cus {cus}: ntiles {nt} G {G} nloc {lo}..{hi}"


def _dev(c, with_mine=True):
    """The case's operands as the kernels take them."""
    d = {"f": c.f.float().to(c.dtype), "w1": c.w1.float().to(c.dtype), "b1": c.b1.float(), "w2": c.w2.float(),
         "b2": c.b2.float(), "dlp": c.dlp.float(), "dlm": None if c.dlm is None else c.dlm.float(),
         "gadd": None if c.gadd is None else c.gadd.float().contiguous()}
    return d


def _eq(got, want, what, msg):
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {first} "
                         f"(got {float(got[first])}, want {float(want[first])}), last at "
                         f"{tuple(int(i) for i in idx[-1])}; {msg}")


def _fwd(d, M, dt, with_mine, f=None):
    from ms_amd import _lib as L
    from ms_amd import fused as F
    dev = d["f"].device
    f = d["f"] if f is None else f
    lp = torch.full((M + GUARD,), -7.0, device=dev)
    lm = torch.full((M + GUARD,), -7.0, device=dev)
    L.check_mc(L.load().mc_heads_fwd(L.ptr(f), L.ptr(d["w1"]), L.ptr(d["b1"]), L.ptr(d["w2"]), L.ptr(d["b2"]),
                                     L.ptr(lp), L.ptr(lm) if with_mine else None, M, F.DTYPES[dt],
                                     L.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert bool((lp[M:] == -7.0).all()) and bool((lm[M if with_mine else 0:] == -7.0).all()), "store past row M"
    return lp[:M], (lm[:M] if with_mine else None)


def _bwd(d, M, P, dt, gadd=True, dlm=True, f=None):
    """mc_heads_bwd -> df [M, 96], dW1 [192, 96], db1, dw2 [192]."""
    from ms_amd import _lib as L
    from ms_amd import fused as F
    lib = L.load()
    dev = d["f"].device
    f = d["f"] if f is None else f
    df = torch.full((M + GUARD, 96), -7.0, device=dev, dtype=dt)
    dw1, db1, dw2 = torch.empty(192, 96, device=dev), torch.empty(192, device=dev), torch.empty(192, device=dev)
    nws = int(lib.mc_heads_bwd_workspace(M))
    work = torch.full((nws,), float("nan"), device=dev)
    L.check_mc(lib.mc_heads_bwd(L.ptr(f), L.ptr(d["dlp"]), L.ptr(d["dlm"]) if dlm else None, L.ptr(d["w1"]), None,
                                L.ptr(d["b1"]), L.ptr(d["w2"]), L.ptr(d["gadd"]) if gadd else None, P, L.ptr(df),
                                L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(work), nws, M, F.DTYPES[dt],
                                L.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert bool((df[M:] == -7.0).all()), "df store past row M"
    return df[:M], dw1, db1, dw2


def _check_bwd(out, r, msg):
    for got, want, what in zip(out, (r.df, r.dW1.float(), r.db1.float(), r.dw2.float()), ("df", "dW1", "db1", "dw2")):
        _eq(got, want, what, msg)


def _case_bwd(gpu, cus, M, P, dt, gadd=True, dlm=True, twice=False):
    c = R.grid_case(M, P, dt, seed=M, gadd=gadd, dlm=dlm, device=gpu)
    r = R.heads_ref(c)
    d = _dev(c)
    msg = _geo(M, P, cus) + f" gadd {gadd} dlm {dlm}"
    print(msg)
    out = _bwd(d, M, P, dt, gadd, dlm)
    _check_bwd(out, r, msg)
    if twice:
        for a, b, what in zip(out, _bwd(d, M, P, dt, gadd, dlm), ("df", "dW1", "db1", "dw2")):
            _eq(b, a, what + " (second run)", msg)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.fwd_rows(CUS_SHAPES))))
@pytest.mark.parametrize("with_mine", [True, False])
@pytest.mark.parametrize("dt", DT)
def test_heads_fwd_bitwise(gpu, cus, i, with_mine, dt):
    """k_heads_fwd at the row counts around its 32-row wave share and 128-row tile, and past one
    grid of 2 x CUs tiles: both logits equal the reference cast to f32."""
    M = R.fwd_rows(cus)[i]
    c = R.grid_case(M, 1, dt, seed=M, gadd=False, device=gpu)
    r = R.heads_ref(c)
    msg = f"M {M}: {-(-M // R.TR)} tiles on a grid of {min(-(-M // R.TR), 2 * cus)}"
    lp, lm = _fwd(_dev(c), M, dt, with_mine)
    _eq(lp, r.lp.float(), "policy logits", msg)
    if with_mine:
        _eq(lm, r.lm.float(), "mine logits", msg)


@pytest.mark.parametrize("i", range(len(R.bwd_tile_shapes(CUS_SHAPES))))
@pytest.mark.parametrize("dt", DT)
def test_heads_bwd_tile_and_reduce_edges(gpu, cus, i, dt):
    """Single tiles (full, partial, one row), and G = ntiles around k_heads_reduce's slice count and
    unrolled stride with a last tile of 37 rows: rows past M must not reach dW1 / db1 / dw2."""
    M, P = R.bwd_tile_shapes(cus)[i]
    _case_bwd(gpu, cus, M, P, dt)


@pytest.mark.parametrize("i", range(len(R.RING_KJ)))
@pytest.mark.parametrize("dt", DT)
def test_heads_bwd_ring_edges(gpu, cus, i, dt):
    """ntiles = k CUs + j: the workgroups of one launch run nloc and nloc + 1 tiles through the
    5-slot ring, across every case of its counted waits; run twice, bitwise the same."""
    M, P = R.bwd_ring_shapes(cus)[i]
    _case_bwd(gpu, cus, M, P, dt, twice=True)


@pytest.mark.parametrize("i", range(len(R.bwd_gadd_shapes(CUS_SHAPES))))
@pytest.mark.parametrize("dt", DT)
def test_heads_bwd_gadd_paths(gpu, cus, i, dt):
    """gadd[row // P] by plain loads (P < 16) and through the LDS-DMA window (aligned, unaligned,
    the production boards, a sample longer than a tile, a single sample), small and past 4 CUs
    tiles: every row takes its own sample's gadd."""
    M, P = R.bwd_gadd_shapes(cus)[i]
    _case_bwd(gpu, cus, M, P, dt)


@pytest.mark.parametrize("i", range(len(R.bwd_optional_shapes(CUS_SHAPES))))
@pytest.mark.parametrize("gadd,dlm", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("dt", DT)
def test_heads_bwd_optional_arguments(gpu, cus, i, gadd, dlm, dt):
    M, P = R.bwd_optional_shapes(cus)[i]
    _case_bwd(gpu, cus, M, P, dt, gadd=gadd, dlm=dlm)


# ---------------------------------------------------------------------------------------------
def _nn_heads(c, dev, which=(0, 1)):
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(96, 96, 1), torch.nn.ReLU(),  # noqa: E731
                                     torch.nn.Conv2d(96, 1, 1)).to(dev)
    out = []
    for i in which:
        h, sl = mk(), slice(i * 96, (i + 1) * 96)
        with torch.no_grad():
            h[0].weight.copy_(c.w1[sl].reshape(96, 96, 1, 1))
            h[0].bias.copy_(c.b1[sl])
            h[2].weight.copy_(c.w2[sl].reshape(1, 96, 1, 1))
            h[2].bias.copy_(c.b2[i:i + 1])
        out.append(h)
    return out


@pytest.mark.parametrize("with_mine", [True, False])
@pytest.mark.parametrize("pooled_given", [True, False])
@pytest.mark.parametrize("f_grad", [True, False])
@pytest.mark.parametrize("dt", DT)
def test_heads_apply_bitwise(gpu, with_mine, pooled_given, f_grad, dt):
    """heads_apply under autograd: the logits, and the gradients of f and of all eight head
    parameters (db2 = sum dl among them), equal the reference."""
    from ms_amd.fused import heads_apply
    n, P = 9, 17
    M = n * P
    c = R.grid_case(M, P, dt, seed=77, dlm=with_mine, device=gpu)
    r = R.heads_ref(c)
    heads = _nn_heads(c, gpu, (0, 1) if with_mine else (0,))
    pol, mine = heads[0], (heads[1] if with_mine else None)
    f = c.f.float().to(dt).view(n, P, 96).requires_grad_(f_grad)
    pre = f.detach().float().mean(1) if pooled_given else None
    lp, pooled, lm = heads_apply(f, pol, mine, pre)
    _eq(lp.detach().reshape(M), r.lp.float(), "policy logits", "")
    assert (lm is None) == (not with_mine)
    loss = (lp * c.dlp.float().view(n, P)).sum() + (pooled * (c.gadd.float() * P)).sum()
    if with_mine:
        _eq(lm.detach().reshape(M), r.lm.float(), "mine logits", "")
        loss = loss + (lm * c.dlm.float().view(n, P)).sum()
    loss.backward()
    if f_grad:
        _eq(f.grad.reshape(M, 96), r.df, "df", "")
    else:
        assert f.grad is None
    for i, h in enumerate(heads):
        sl = slice(i * 96, (i + 1) * 96)
        _eq(h[0].weight.grad.reshape(96, 96), r.dW1[sl].float(), f"dW1 of head {i}", "")
        _eq(h[0].bias.grad, r.db1[sl].float(), f"db1 of head {i}", "")
        _eq(h[2].weight.grad.reshape(96), r.dw2[sl].float(), f"dw2 of head {i}", "")
        _eq(h[2].bias.grad.reshape(()), r.db2[i].float(), f"db2 of head {i}", "")


def test_heads_weight_cache_follows_the_parameters(gpu):
    """The packed-weight cache of ms_amd.fused (_hcache) after an optimizer step, after a
    load_state_dict, and for new heads of the same shapes made after the first pair is dropped:
    each forward equals one on freshly built heads with the same weights, and the reference."""
    from ms_amd.fused import heads_forward
    n, P, dt = 5, 20, torch.float16
    M = n * P
    cs = [R.grid_case(M, P, dt, seed=200 + k, device=gpu) for k in range(4)]
    for k in range(1, 4):  # same features throughout: only the weights change
        cs[k].f = cs[0].f
    rs = [R.heads_ref(c) for c in cs]
    f = cs[0].f.float().to(dt).view(n, P, 96)

    def check(pol, mine, k, what):
        lp, lm = heads_forward(f, pol, mine)
        fresh = _nn_heads(cs[k], gpu)
        for h, g in zip((pol, mine), fresh):
            for a, b in zip(h.parameters(), g.parameters()):
                assert torch.equal(a, b), what
        _eq(lp.reshape(M), rs[k].lp.float(), "policy logits " + what, "")
        _eq(lm.reshape(M), rs[k].lm.float(), "mine logits " + what, "")
        lp2, lm2 = heads_forward(f, *fresh)
        assert torch.equal(lp, lp2) and torch.equal(lm, lm2), what

    def fill(pol, mine, k):  # leaves the pair in the cache
        heads_forward(f, pol, mine)
        return pol, mine

    for rnd in range(2):
        pol, mine = _nn_heads(cs[0], gpu)
        check(pol, mine, 0, f"new heads (pair {rnd})")
        # an SGD step with lr 1 and grad = old - new lands on case 1's weights exactly
        fill(pol, mine, 0)
        tgt = _nn_heads(cs[1], gpu)
        params = list(pol.parameters()) + list(mine.parameters())
        opt = torch.optim.SGD(params, lr=1.0)
        for p, q in zip(params, list(tgt[0].parameters()) + list(tgt[1].parameters())):
            p.grad = p.detach() - q.detach()
        opt.step()
        check(pol, mine, 1, f"after optimizer.step (pair {rnd})")
        fill(pol, mine, 1)
        src = _nn_heads(cs[2], gpu)
        pol.load_state_dict(src[0].state_dict())
        mine.load_state_dict(src[1].state_dict())
        check(pol, mine, 2, f"after load_state_dict (pair {rnd})")
        fill(pol, mine, 2)
        del pol, mine, params, opt, tgt, src
        gc.collect()
        cs[0], rs[0] = cs[3], rs[3]  # the second pair starts from other weights than the cached ones


# ---------------------------------------------------------------------------------------------
NAN_ROW, INF_ROW = 37, 200  # in different forward tiles and backward tiles


def _poisoned(gpu, dt):
    M = 300
    c = R.grid_case(M, 1, dt, seed=31, device=gpu)
    d = _dev(c)
    k = next(k for k in range(96) if all(bool((c.w1[sl, k] > 0).any()) and bool((c.w1[sl, k] < 0).any())
                                         for sl in (slice(0, 96), slice(96, 192))))
    fp = d["f"].clone()
    fp[NAN_ROW] = float("nan")
    fp[INF_ROW, k] = float("inf")
    clean = torch.ones(M, dtype=torch.bool, device=gpu)
    clean[[NAN_ROW, INF_ROW]] = False
    return c, d, fp, clean


def _torch_f32(d, fp):
    """The heads as PyTorch runs them in f32 on the poisoned features -> logits and the
    gradients of W1, b1, w2 (both heads stacked)."""
    w1, b1, w2 = (d[k].float().clone().requires_grad_(True) for k in ("w1", "b1", "w2"))
    a = torch.relu(torch.nn.functional.linear(fp.float(), w1, b1))
    lp = a[:, :96] @ w2[:96] + d["b2"][0]
    lm = a[:, 96:] @ w2[96:] + d["b2"][1]
    ((lp * d["dlp"]).sum() + (lm * d["dlm"]).sum()).backward()
    return lp.detach(), lm.detach(), (w1.grad, b1.grad, w2.grad)


@pytest.mark.parametrize("dt", DT)
def test_heads_fwd_propagates_nan(gpu, dt):
    """A NaN feature row and a row with one +inf feature: the logits are non-finite exactly where
    the f32 PyTorch heads' are (torch.relu keeps a NaN; fmaxf(x, 0) made it 0 and the logits
    finite), and every other row is bitwise what it is without the poison."""
    c, d, fp, clean = _poisoned(gpu, dt)
    lp0, lm0 = _fwd(d, c.M, dt, True)
    lp, lm = _fwd(d, c.M, dt, True, f=fp)
    lpo, _ = _fwd(d, c.M, dt, False, f=fp)  # the policy-only kernel
    tp, tm, _ = _torch_f32(d, fp)
    assert not bool(torch.isfinite(tp[[NAN_ROW, INF_ROW]]).any())  # the test's own premise
    for got, ref, what in ((lp, tp, "policy"), (lm, tm, "mine"), (lpo, tp, "policy, no mine head")):
        bad, want = ~torch.isfinite(got), ~torch.isfinite(ref)
        assert torch.equal(bad, want), (f"{what} logits: non-finite rows {bad.nonzero().flatten().tolist()}, "
                                        f"PyTorch's {want.nonzero().flatten().tolist()}")
    assert torch.equal(lp[clean], lp0[clean]) and torch.equal(lm[clean], lm0[clean])
    assert torch.equal(lpo[clean], lp0[clean])


@pytest.mark.parametrize("dt", DT)
def test_heads_bwd_propagates_nan(gpu, dt):
    """The same poisoned features in the backward: every parameter gradient that PyTorch's f32
    path makes non-finite is non-finite here (the GradScaler's skip relies on it), and df of the
    clean rows does not change. (The backward gates on h > 0 and held this before the forward's
    ReLU was fixed: 0 * NaN in dh^T f and NaN * 0 in dw2 carry the NaN; this pins it.)"""
    c, d, fp, clean = _poisoned(gpu, dt)
    df0, *_ = _bwd(d, c.M, 1, dt)
    df, dw1, db1, dw2 = _bwd(d, c.M, 1, dt, f=fp)
    _, _, tg = _torch_f32(d, fp)
    assert not bool(torch.isfinite(tg[0]).all())  # the test's own premise
    for got, ref, what in zip((dw1, db1, dw2), tg, ("dW1", "db1", "dw2")):
        for sl, head in ((slice(0, 96), "policy"), (slice(96, 192), "mine")):
            if not bool(torch.isfinite(ref[sl]).all()):
                assert not bool(torch.isfinite(got[sl]).all()), f"{what} of the {head} head is finite"
    assert torch.equal(df[clean], df0[clean])
