"""Pins tests/trunk_ref.py (the staged f64 trunk layer that the HIP kernels of csrc/mscnn*.hip are compared
with element by element) to PyTorch itself on the CPU, and shows without a device that its bounds are
neither vacuous nor too tight:
  * every stage equals PyTorch in f64 (conv2d, group_norm with the affine applied by hand, autograd for
    gn_bwd, dgrad and wgrad): torch.equal on the exact grid, rtol 1e-12 elsewhere;
  * at every board of the GPU test and in both 16-bit types, an f32 torch evaluation of each stage that
    sums in another order than the reference passes the bound on every element, and each of eight
    single-element mistakes (MUTANTS) fails it on at least one;
  * every exact-grid case tests/test_trunk_elementwise_gpu.py builds for 256 and for 304 CUs meets the
    grid's preconditions."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import trunk_ref as R

C = R.C


def _nchw(t, H, W):
    n, p, c = t.shape
    return t.view(n, H, W, c).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    n, c, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, H * W, c)


def _conv_w(w):  # [9, 96, cin] (tap, co, ci) -> nn.Conv2d's [96, cin, 3, 3]
    return w.view(3, 3, C, w.shape[-1]).permute(2, 3, 0, 1).contiguous()


def _close(a, b, scale=None):
    """rtol 1e-12; sums that cancel are compared relative to ``scale``, their sum of absolute terms."""
    atol = 0.0 if scale is None else 1e-12 * float(scale)
    torch.testing.assert_close(a, b, rtol=1e-12, atol=atol)


def _case(H, W, cin, dtype, seed, n=R.NBASE):
    """One layer's operands as f64 holding 16-bit / f32 values: the GPU test's general case."""
    g = torch.Generator().manual_seed(seed)
    P = H * W
    c = R.random_params(g, cin)
    c.H, c.W, c.P, c.cin, c.dtype, c.N = H, W, P, cin, dtype, n
    c.w = R.q16(c.w, dtype)
    c.x = R.q16(torch.randn((n, P, cin), generator=g) * (0.5 if cin == C else 1.0), dtype)
    c.x[R.ZERO_X_ROW % n] = 0
    c.res = R.q16(torch.randn((n, P, C), generator=g), dtype)
    c.dmask = R.random_dmask(g, n, zero_row=R.ZERO_DMASK_ROW % n)
    c.dout = R.q16(torch.randn((n, P, C), generator=g), dtype)
    c.addend = R.q16(torch.randn((n, P, C), generator=g), dtype)
    c.wT = R.q16(torch.randn((9, C, C), generator=g) / (3.0 * C ** 0.5), dtype)
    return c


# ---------------------------------------------------------------------------------------------
# the reference is PyTorch

@pytest.mark.parametrize("H,W,cin", [(5, 7, 16), (1, 1, 96), (6, 9, 96), (16, 16, 96)])
def test_grid_stages_equal_torch(H, W, cin):
    """Exact grid: y, dx and dw of the reference are PyTorch's conv2d and its autograd, bit for bit."""
    c = R.grid_case(3, H, W, cin, torch.bfloat16, seed=H * W + cin)
    x = _nchw(c.x, H, W).requires_grad_(True)
    w = _conv_w(c.w).requires_grad_(True)
    y = F.conv2d(x, w, c.bias, padding=1)
    y.backward(_nchw(c.dy, H, W))
    assert torch.equal(_nhwc(y.detach()), R.conv_y(c.x, c.w, c.bias, H, W)[0])
    assert torch.equal(_conv_w(R.wgrad(c.dy, c.x, H, W)[0]), w.grad)
    if cin == C:
        wT = c.w.permute(0, 2, 1).contiguous()  # [9, ci, co]
        assert torch.equal(R.dgrad(c.dy, wT, H, W)[0], _nhwc(x.grad))


@pytest.mark.parametrize("H,W,cin", [(5, 7, 16), (1, 1, 96), (3, 43, 96), (12, 12, 96)])
@pytest.mark.parametrize("with_res", [False, True])
def test_stages_equal_torch(H, W, cin, with_res):
    """Random 16-bit operands: every stage against conv2d / group_norm / autograd in f64."""
    dt = torch.float16
    c = _case(H, W, cin, dt, seed=H + W + cin, n=3)
    res = c.res if with_res else None
    dmask = None if with_res else c.dmask
    x = _nchw(c.x, H, W).requires_grad_(True)
    w = _conv_w(c.w).requires_grad_(True)
    bias, gamma, beta = (t.clone().requires_grad_(True) for t in (c.bias, c.gamma, c.beta))
    y = F.conv2d(x, w, bias, padding=1)
    y.retain_grad()
    z = F.group_norm(y, R.NG, None, None, eps=R.EPS) * gamma[None, :, None, None] + beta[None, :, None, None]
    if with_res:
        z = z + _nchw(res, H, W)
    o = torch.relu(z)
    if dmask is not None:
        o = o * dmask[:, :, None, None]
    o.backward(_nchw(c.dout, H, W))

    yr, mag = R.conv_y(c.x, c.w, c.bias, H, W)
    _close(yr, _nhwc(y.detach()), mag.max())
    st, _ = R.gn_stats(yr, torch.zeros_like(yr))
    yg = y.detach().reshape(3, R.NG, -1)
    _close(st[..., 0], yg.mean(-1), yg.abs().max())
    _close(st[..., 1], torch.rsqrt(yg.var(-1, unbiased=False) + R.EPS))
    outr, _ = R.gn_out(yr, st, c.gamma, c.beta, res, dmask)
    _close(outr, _nhwc(o.detach()), outr.abs().max() + 1)
    _close(R.pooled(outr)[0], o.detach().mean((2, 3)), outr.abs().max() + 1)
    # the backward from the forward's own ReLU decisions; dz is kept unrounded (e_dout given) as autograd keeps it
    b = R.gn_bwd(c.dout, torch.zeros_like(c.dout), yr, st, outr > 0, c.gamma, dmask, dt)
    scale = (b.dy.abs() + b.dz.abs()).max() * 16 * c.P
    _close(b.dy, _nhwc(y.grad), scale)
    dgn, _ = R.dgn_total(b.terms, b.e_terms)
    _close(dgn[0], gamma.grad, scale)
    _close(dgn[1], beta.grad, scale)
    _close(dgn[2], bias.grad, scale)
    dw, wmag = R.wgrad(_nhwc(y.grad), c.x, H, W)
    _close(_conv_w(dw), w.grad, wmag.max())
    if cin == C:
        dx, dmag = R.dgrad(_nhwc(y.grad), c.w.permute(0, 2, 1).contiguous(), H, W)
        _close(dx, _nhwc(x.grad), dmag.max())


def test_exact_dz_is_the_f32_product_rounded_once():
    """e_dout None: dz is 16-bit(f32(dout * dmask)) where the ReLU bit is set, exactly, bound 0."""
    dt = torch.bfloat16
    c = _case(5, 7, 96, dt, seed=1)
    y, _ = R.conv_y(c.x, c.w, c.bias, 5, 7)
    st, _ = R.gn_stats(y, torch.zeros_like(y))
    bits = torch.rand(y.shape, generator=torch.Generator().manual_seed(2)) < 0.5
    b = R.gn_bwd(c.dout, None, R.q16(y, dt), st.float().double(), bits, c.gamma, c.dmask, dt)
    want = (c.dout.float() * c.dmask.float()[:, None]).to(dt).double() * bits
    assert torch.equal(b.dz, want) and not b.e_dz.any()
    assert bool((want != c.dout * c.dmask[:, None] * bits).any())  # the rounding is exercised


def test_half_ulp16():
    for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        a = torch.tensor([1.0, 1.5, 1.999, 2.0, 0.75, 1000.0], dtype=torch.float64)
        want = torch.tensor([0, 0, 0, 1, -1, 9], dtype=torch.float64)
        assert torch.equal(R.half_ulp16(a, dt), torch.exp2(want - bits))
        # the spacing of the type around a, measured: nextafter in the 16-bit type
        v = a.to(dt)
        up = torch.nextafter(v, torch.full_like(v, float("inf")))
        assert torch.equal((up.double() - v.double()) / 2, R.half_ulp16(v.double(), dt))
    sub = torch.tensor([0.0, 2.0 ** -20, 2.0 ** -14], dtype=torch.float64)
    assert torch.equal(R.half_ulp16(sub, torch.float16), torch.full((3,), 2.0 ** -25, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------
# an f32 evaluation of every stage, summed in another order than the reference, with optional mistakes

def _f32_layer(c, with_res, mut=None):
    """Forward and backward of one layer in f32 torch ops, rounding to 16 bits where the kernels do. The
    sums run in other orders than trunk_ref's: taps last to first with the bias added at the end, pixels
    and samples reversed. ``mut`` applies one of MUTANTS. Returns the 'kernel outputs' as a namespace."""
    H, W, P, dt, N = c.H, c.W, c.P, c.dtype, c.N
    f = lambda t: t.float()  # noqa: E731
    o = R.SimpleNamespace()
    x32, w32 = f(c.x), f(c.w)
    if mut == "zero_row":  # the last pixel taken from the zero row
        x32 = x32.clone()
        x32[:, P - 1] = 0
    y32 = torch.zeros((N, P, C), dtype=torch.float32)
    for tap in reversed(range(9)):
        y32 += R.shifted(x32, H, W, tap) @ w32[tap].t()
    if mut == "corner_tap":  # tap 0 of pixel 0 lies off the board; it reads the last pixel instead
        y32[:, 0] += x32[:, P - 1] @ w32[0].t()
    if mut == "dropped_product":  # one product of one output element missing: the largest of its centre tap
        prod = x32[1, P // 2] * w32[4, 3]
        y32[1, P // 2, 3] -= prod[prod.abs().argmax()]
    y32 = y32 + f(c.bias)
    o.y = y32.to(dt)
    yg = R._groups(y32).flip(-1)
    mean = yg.sum(-1) / yg.shape[-1]
    var = ((yg - mean[..., None]) ** 2).sum(-1) / yg.shape[-1]
    o.stats = torch.stack([mean, torch.rsqrt(var + torch.tensor(R.EPS, dtype=torch.float32))], -1)
    # out, from the stored y and statistics
    st = o.stats.clone()
    if mut == "group_stats":
        st[:, 5] = st[:, 4]
    m, r = R._per_channel(st)
    beta = f(c.beta).clone()
    if mut == "beta":
        beta[40] += 2.0 ** -7
    dm = f(c.dmask)
    if mut == "dmask_shift":  # sample n's mask applied to sample n + 1
        dm = dm.roll(1, 0)
    a = f(c.gamma) * r
    b = beta - m * a
    z = f(o.y) * a[:, None] + b[:, None]
    if with_res:
        z = z + f(c.res)
    z = torch.relu(z)
    if not with_res:
        z = z * dm[:, None]
    o.out = z.to(dt)
    o.bits = f(o.out) > 0
    o.pooled = f(o.out).flip(1).sum(1) / P
    # backward from the stored y, statistics and bits
    m, r = R._per_channel(o.stats)
    d = f(c.dout) * (dm[:, None] if not with_res else 1.0)
    o.dz = torch.where(o.bits, d, torch.zeros_like(d)).to(dt)
    dz = f(o.dz)
    yh = (f(o.y) - m[:, None]) * r[:, None]
    S1, S2, S3 = dz.flip(1).sum(1), (dz * yh).flip(1).sum(1), yh.flip(1).sum(1)
    g32 = f(c.gamma)
    n = R.GC * P
    m1 = (g32 * S1).view(N, R.NG, R.GC).flip(-1).sum(-1).repeat_interleave(R.GC, 1) / n
    m2 = (g32 * S2).view(N, R.NG, R.GC).flip(-1).sum(-1).repeat_interleave(R.GC, 1) / n
    A, Bg, Cg = r * g32, -r * r * m2, r * (r * m2 * m - m1)
    o.dy = (A[:, None] * dz + (Bg[:, None] * f(o.y) + Cg[:, None])).to(dt)
    o.dgn = torch.stack([S2.flip(0).sum(0), S1.flip(0).sum(0), (r * (g32 * S1 - P * m1 - m2 * S3)).flip(0).sum(0)])
    dy32 = f(o.dy)
    dx = torch.zeros((N, P, C), dtype=torch.float32)
    for tap in reversed(range(9)):
        dx += R.shifted(dy32, H, W, tap, sign=-1) @ f(c.wT)[tap].t()
    ad = f(c.addend).clone()
    if mut == "addend":  # left out at one pixel
        ad[3 % N, P // 3] = 0
    o.dx = (f(dx.to(dt)) + ad).to(dt)
    ns = N - 1 if mut == "dw_last_sample" else N
    xs, dys = f(c.x)[:ns].flip(0), dy32[:ns].flip(0)
    o.dw = torch.stack([dys.reshape(-1, C).t() @ R.shifted(xs, H, W, tap).reshape(ns * P, -1) for tap in range(9)])
    return o


def _failures(c, o, with_res):
    """Count of failing elements per stage: the reference's stages on what the 'kernel' stored upstream."""
    H, W, dt, N, P = c.H, c.W, c.dtype, c.N, c.P
    d = lambda t: t.double()  # noqa: E731
    res = c.res if with_res else None
    dmask = None if with_res else c.dmask
    bad = {}
    y, mag = R.conv_y(c.x, c.w, c.bias, H, W)
    e_y = R.y_err(mag, c.cin)
    bad["y"] = R.bad(o.y, y, R.tol16(y, e_y, dt))
    st, e_st = R.gn_stats(y, e_y)
    bad["stats"] = R.bad(o.stats, st, e_st)
    out, e_out = R.gn_out(d(o.y), d(o.stats), c.gamma, c.beta, res, dmask)
    bad["out"] = R.bad(o.out, out, R.tol16(out, e_out, dt))
    bad["bits"] = o.bits != (d(o.out) > 0)
    pl, e_pl = R.pooled(d(o.out))
    bad["pooled"] = R.bad(o.pooled, pl, e_pl)
    b = R.gn_bwd(c.dout, None, d(o.y), d(o.stats), o.bits, c.gamma, dmask, dt)
    bad["dz"] = d(o.dz) != b.dz
    bad["dy"] = R.bad(o.dy, b.dy, R.tol16(b.dy, b.e_dy, dt))
    dgn, e_dgn = R.dgn_total(b.terms, b.e_terms)
    bad["dgn"] = R.bad(o.dgn, dgn, e_dgn)
    dx, dmag = R.dgrad(d(o.dy), c.wT, H, W)
    dxa, e_dx = R.add16_err(dx, R.dgrad_err(dmag), c.addend, dt)
    bad["dx"] = R.bad(o.dx, dxa, R.tol16(dxa, e_dx, dt))
    dw, wmag = R.wgrad(d(o.dy), c.x, H, W)
    bad["dw"] = R.bad(o.dw, dw, R.wgrad_err(wmag, N, P))
    return {k: int(v.sum()) for k, v in bad.items()}


# mistake -> the stages that must reject it (at least one element each)
MUTANTS = {
    "corner_tap": ("y",),             # one tap read from the wrong neighbour at a corner pixel
    "zero_row": ("y",),               # the last pixel P - 1 taken from the zero row
    "dropped_product": ("y",),        # one product of one output element dropped
    "beta": ("out",),                 # beta of one channel off by 2^-7
    "group_stats": ("out",),          # the statistics of group 5 taken from group 4
    "dmask_shift": ("out", "dz", "dy"),  # dmask of sample n applied to sample n + 1
    "addend": ("dx",),                # addend left out at one pixel
    "dw_last_sample": ("dw",),        # dw missing the last sample
}
BOARDS = [(h, w, C) for h, w in R.BOARDS_96] + [(h, w, 16) for h, w in R.BOARDS_16]


@pytest.mark.parametrize("H,W,cin", BOARDS, ids=[f"{h}x{w}-c{c}" for h, w, c in BOARDS])
@pytest.mark.parametrize("dt", R.DTYPES, ids=["bf16", "fp16"])
def test_bound_accepts_f32_and_rejects_mutants(H, W, cin, dt):
    c = _case(H, W, cin, dt, seed=1000 * H + W + cin)
    for with_res in (False, True):
        n_bad = _failures(c, _f32_layer(c, with_res), with_res)
        assert not any(n_bad.values()), f"f32 evaluation rejected (res {with_res}): {n_bad}"
    for mut, stages in MUTANTS.items():
        if mut == "dropped_product":  # certain to show only if it exceeds twice the rounding plus the bound
            y, mag = R.conv_y(c.x, c.w, c.bias, H, W)
            y, e = y[1, c.P // 2, 3], R.y_err(mag, cin)[1, c.P // 2, 3]
            if float((c.x[1, c.P // 2] * c.w[4, 3]).abs().max()) <= float(2 * R.half_ulp16(y.abs() + e, dt) + 3 * e):
                continue
        with_res = mut not in ("dmask_shift",)  # the mask belongs to the layers without a residual
        n_bad = _failures(c, _f32_layer(c, with_res, mut), with_res)
        for s in stages:
            assert n_bad[s] > 0, f"{mut} passes stage {s}: {n_bad}"


def test_corner_tap_is_seen_on_most_channels():
    """At 16x16x96 the wrapped corner tap is rejected on at least 98 % of the channels of pixel 0."""
    for dt in R.DTYPES:
        c = _case(16, 16, 96, dt, seed=5)
        o = _f32_layer(c, False, "corner_tap")
        y, mag = R.conv_y(c.x, c.w, c.bias, 16, 16)
        bad = R.bad(o.y, y, R.tol16(y, R.y_err(mag, 96), dt))
        live = [n for n in range(c.N) if n != R.ZERO_X_ROW]
        assert float(bad[live, 0].double().mean()) >= 0.98
        assert not bad[:, 1:].any()


def test_f32_equals_f64_on_the_grid():
    c = R.grid_case(R.NBASE, 16, 16, 96, torch.float16, seed=3)
    o = _f32_layer(R.SimpleNamespace(**{**vars(_case(16, 16, 96, torch.float16, 0)), "x": c.x, "w": c.w,
                                        "bias": c.bias}), False)
    y, _ = R.conv_y(c.x, c.w, c.bias, 16, 16)
    assert torch.equal(o.y, R.round16(y, torch.float16))


# ---------------------------------------------------------------------------------------------
# every exact-grid case of the GPU test, for both CU counts in the field

@pytest.mark.parametrize("cus", [256, 304])
def test_gpu_grid_cases_meet_preconditions(cus):
    cases = R.grid_cases(cus)
    assert len(cases) == len(R.BOARDS_96) + len(R.BOARDS_16) + len(R.BOARDS_LONG) + len(R.loop_cases(cus))
    for n, h, w, cin in cases:
        for dt in R.DTYPES:
            c = R.grid_case(n, h, w, cin, dt, seed=h * 100 + w, check=False)
            R.assert_grid_preconditions(c)
            assert c.x.shape == (n, h * w, cin) and c.dy.shape == (n, h * w, C)
    # the loop cases: an odd tail after more than one iteration, for pairs and for single samples
    for n in R.pair_ns(cus):
        assert (n + 1) // 2 > cus
    assert [n % 2 for n in R.pair_ns(cus)] == [1, 0, 1, 1]
    assert all(cus < n for n in R.one_ns(cus))
