"""The fused residual-CNN kernels (csrc/mscnn.hip, mscnn_bwd.hip, mscnn_trunk.hip) through the C ABI
(include/mscnn.h) against the staged f64 reference tests/trunk_ref.py, ELEMENT BY ELEMENT: every stage of
every layer is compared with f64 computed from the tensors the kernel itself stored upstream, under the
derived f32 bounds of trunk_ref (no norms, no exempt elements), and bitwise on the exact grid. Every output
lies between 64 sentinel rows, every workspace is exactly mc_*_workspace long, filled with NaN, between
sentinels; the sentinels are checked after every call. tests/test_trunk_ref.py pins the reference and its
bounds on the CPU; tests/test_trunk_gpu.py keeps the bitwise one-launch == per-layer chain checks.

Which case launches which (kernel, template instance); P = H * W, boards from trunk_ref.BOARDS_*:
  k_conv_gn_fwd<cin, NPT, FULL>, k_bwd_data<NPT, DGRAD, NCH, RM = 1> (test_per_layer; DGRAD 0 at cin 16):
    <1, 0> NCH 13   1x1, 1x9, 9x1, 5x7 (both cin), 8x16 (P = 128: the P <= 128 boundary)
    <2, 0> NCH 13   3x43 (129), 12x12 (both cin), 15x17 (255)
    <2, 1> NCH 13   16x16 (both cin)
    <3, 0> NCH 25   6x43 (258), 18x18 (both cin), 6x64 (384: the boundary)
    <4, 0> NCH 25   7x55 (385), 30x16, 16x32 and 8x64 (512, W = 64); 1x512, 512x1 forward only
  k_wgrad<cin, PF 0>: every board but 16x16; <96, PF 1, SG 0 / 1>: 16x16 variants 1 / 2; k_wgrad_c96<GN 0>: 16x16
    variants 0 / 3; k_wgrad_c96<GN 1>: test_nan_through_wgrad_gn_recompute
  k_trunk_fwd2<NPT, FULL> (test_one_launch[..-fwd2], mc_set_variant(3, 1)) and
  k_trunk_fwd_pp<NPT, FULL, SAVE = 1> (test_one_launch[..-pp], variant 2):
    <1, 0> P < 128: 1x1 .. 5x7   <1, 1> (pp) 8x16   <2, 0> 3x43, 12x12, 15x17   <2, 1> 16x16
    (k_trunk_fwd2 runs 8x16 as <1, 0>); k_trunk_fwd_pp<.., SAVE = 0>: test_nan_through_relu and the no-save run
    of test_one_launch
  k_trunk_fwd<NPT, 0> (test_one_launch[..-fwd]): <3> 6x43, 18x18, 6x64   <4> 7x55, 30x16, 16x32, 8x64
  k_trunk_bwd<NPT, NCH> (test_one_launch, every board): <1, 13> P <= 128, <2, 13> P <= 256 (skip gradient held
    in registers), <3, 25> P <= 384, <4, 25> above (skip gradient through the workspace slot)
  depth (test_depth): 10 layers = PP_MAXL run k_trunk_fwd_pp under variant 2, 12 and 16 layers fall back to
    k_trunk_fwd2; 18 layers MS_EINVAL
  loops (test_loop_odd_tail): 5x7 and 9x9 at N = 2 cus + 1, 2 cus + 2, 4 cus - 1, 4 cus + 3 through k_trunk_fwd2 and
    k_trunk_fwd_pp (an odd N leaves team B one sample short after more than one iteration), k_trunk_bwd and
    k_wgrad looping over samples; 18x18 at N = cus + 1, 2 cus + 1 through k_trunk_fwd and k_trunk_bwd (one
    workgroup a CU: a second iteration for one / every workgroup, two partial rows a workgroup)."""
from __future__ import annotations

import pytest
import torch

import trunk_ref as R

pytestmark = pytest.mark.gpu

C = R.C
GUARD = 64
MS_EINVAL = 1  # include/msenv.h
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def _lib():
    from ms_amd import _lib as L
    return L, L.load()


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


# ---------------------------------------------------------------------------------------------
# guarded allocations

class Guards:
    """Outputs and workspaces carved out of larger byte buffers filled with a sentinel."""
    SENT = 0xA5

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def out(self, shape, dtype, fill=None, row=None):
        """A tensor with GUARD rows (``row`` elements each; default: its last dimension) of sentinel bytes
        before and after it. The tensor itself starts as sentinel bytes too, or as the byte ``fill``."""
        item = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= s
        pad = -(-GUARD * (row or shape[-1]) * item // 16) * 16
        buf = torch.full((pad + n * item + pad,), self.SENT, dtype=torch.uint8, device=self.dev)
        if fill is not None:
            buf[pad:pad + n * item] = fill
        self.bufs.append((buf, pad, n * item))
        return buf[pad:pad + n * item].view(dtype).view(shape)

    def work(self, nbytes):
        """A workspace of exactly ``nbytes`` bytes of NaN (0xFF in every type), between sentinels."""
        assert nbytes > 0
        return self.out((int(nbytes),), torch.uint8, fill=0xFF, row=256)

    def check(self, what):
        torch.cuda.synchronize()
        for i, (buf, pad, n) in enumerate(self.bufs):
            ok = bool((buf[:pad] == self.SENT).all()) and bool((buf[pad + n:] == self.SENT).all())
            assert ok, f"{what}: sentinel rows around allocation {i} ({n} bytes) overwritten"

    @staticmethod
    def untouched(t):
        return bool((t.contiguous().view(torch.uint8) == Guards.SENT).all())


def _report(stage, layer, got, ref, tol, extra=""):
    """Assert that no element is off by more than its tolerance; the message names the stage, the layer,
    the count of bad elements, the first and the last of them and got / want / tol there."""
    badm = R.bad(got, ref, tol)
    nbad = int(badm.sum())
    if nbad == 0:
        return
    idx = badm.nonzero()
    msg = [f"stage {stage}, layer {layer}{extra}: {nbad} of {badm.numel()} elements out of tolerance"]
    for name, i in (("first", idx[0]), ("last", idx[-1])):
        t = tuple(int(k) for k in i)
        msg.append(f"  {name} at {t}: got {float(got[t]):.9g} want {float(ref[t]):.9g} tol {float(tol[t]):.3g}")
    raise AssertionError("\n".join(msg))


def _same(stage, layer, got, want, extra=""):
    if got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want):
        return
    ne = (got != want) if got.shape == want.shape else None
    assert ne is not None, f"stage {stage}, layer {layer}{extra}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    idx = ne.nonzero()
    msg = [f"stage {stage}, layer {layer}{extra}: {int(ne.sum())} of {ne.numel()} elements differ (bitwise check)"]
    for name, i in (("first", idx[0]), ("last", idx[-1])):
        t = tuple(int(k) for k in i)
        msg.append(f"  {name} at {t}: got {float(got[t]):.9g} want {float(want[t]):.9g} tol 0")
    raise AssertionError("\n".join(msg))


# ---------------------------------------------------------------------------------------------
# operands

def _zero_rows(n):
    """(sample with an all-zero dmask row, sample with an all-zero input)."""
    return (R.ZERO_DMASK_ROW, R.ZERO_X_ROW) if n > R.ZERO_X_ROW else (n - 1, 0)


def _acts(g, shape, dt, dev, scale=1.0):
    return R.q16(torch.randn(shape, generator=g) * scale, dt).to(dev)


class Layer:
    """One layer's parameters on the device: f64 values (p.*) and the tensors the kernels read."""

    def __init__(self, g, cin, dt, dev, n, dmask, zero_dmask_row=None):
        self.p = R.random_params(g, cin, dev)
        self.p.w = R.q16(self.p.w, dt)
        self.cin, self.dt = cin, dt
        self.w = self.p.w.to(dt).contiguous()
        self.wT = self.p.w.permute(0, 2, 1).to(dt).contiguous() if cin == C else None
        self.bias, self.gamma, self.beta = (t.float().contiguous() for t in (self.p.bias, self.p.gamma, self.p.beta))
        self.dm64 = R.random_dmask(g, n, dev, zero_row=zero_dmask_row) if dmask else None
        self.dmask = self.dm64.float().contiguous() if dmask else None

    def tile(self, idx):
        if self.dm64 is not None:
            self.dm64 = self.dm64[idx]
            self.dmask = self.dm64.float().contiguous()


def _fwd_outputs(G, n, P, dt):
    o = R.SimpleNamespace()
    o.out, o.y = G.out((n, P, C), dt), G.out((n, P, C), dt)
    o.stats = G.out((n, R.NG, 2), torch.float32)
    o.rmask = G.out((n, P, C // 8), torch.uint8)
    return o


def _check_forward_layer(lay, H, W, x64, o, res64, layer, tag=""):
    """Stages y, stats, out and the ReLU bits of one layer from its input and the kernel's stored tensors."""
    dt = lay.dt
    y, mag = R.conv_y(x64, lay.p.w, lay.p.bias, H, W)
    e_y = R.y_err(mag, lay.cin)
    _report("y", layer, o.y, y, R.tol16(y, e_y, dt), tag)
    st, e_st = R.gn_stats(y, e_y)
    _report("stats", layer, o.stats, st, e_st, tag)
    out, e_out = R.gn_out(o.y.double(), o.stats.double(), lay.p.gamma, lay.p.beta, res64, lay.dm64)
    _report("out", layer, o.out, out, R.tol16(out, e_out, dt), tag)
    _same("bits", layer, R.unpack_bits(o.rmask), o.out.float() > 0, tag)


def _dtc(dt):
    from ms_amd.fused import DTYPES
    return DTYPES[dt]


# ---------------------------------------------------------------------------------------------
# per-layer kernels

def _call_fwd(lib, L, lay, x, res, o, n, H, W, dev):
    return lib.mc_conv_gn_fwd(L.ptr(x), L.ptr(lay.w), L.ptr(lay.bias), L.ptr(lay.gamma), L.ptr(lay.beta), L.ptr(res),
                              L.ptr(lay.dmask), L.ptr(o.out), L.ptr(o.y), L.ptr(o.stats), L.ptr(o.rmask), n, H, W,
                              lay.cin, R.EPS, _dtc(lay.dt), L.stream_ptr(dev))


def _wgrad(lib, L, G, dy, x, n, H, W, cin, dt, dev):
    dw = G.out((9, C, cin), torch.float32)
    nws = int(lib.mc_conv_gn_bwd_workspace(n, H, W, cin))
    work = G.work(4 * nws)
    rc = lib.mc_conv_wgrad(L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(work), nws, n, H, W, cin, _dtc(dt), L.stream_ptr(dev))
    return rc, dw


def _grid_checks(lib, L, gpu, H, W, cin, dt, n, long_board=False):
    """Exact grid: ysave of mc_conv_gn_fwd and dw of mc_conv_wgrad under variants 0 .. 3, bit for bit."""
    from ms_amd import fused as F
    G = Guards(gpu)
    c = R.grid_case(n, H, W, cin, dt, seed=100 * H + W, device=gpu)
    g = torch.Generator().manual_seed(7)
    lay = Layer(g, cin, dt, gpu, n, dmask=False)
    lay.w, lay.bias = c.w.to(dt).contiguous(), c.bias.float().contiguous()
    o = _fwd_outputs(G, n, c.P, dt)
    assert _call_fwd(lib, L, lay, c.x.to(dt).contiguous(), None, o, n, H, W, gpu) == 0
    G.check("mc_conv_gn_fwd (grid)")
    y, _ = R.conv_y(c.x, c.w, c.bias, H, W)
    _same("y (exact grid)", 0, o.y, R.round16(y, dt))
    dw_ref = R.wgrad(c.dy, c.x, H, W)[0].float()
    for v in (0, 1, 2, 3):
        with F.kernel_variant(F.VARIANT_WGRAD, v):
            rc, dw = _wgrad(lib, L, G, c.dy.to(dt).contiguous(), c.x.to(dt).contiguous(), n, H, W, cin, dt, gpu)
        G.check(f"mc_conv_wgrad variant {v} (grid)")
        if long_board and rc != 0:
            assert rc == MS_EINVAL and Guards.untouched(dw), "mc_conv_wgrad refused a board after touching dw"
            continue
        assert rc == 0, lib.mc_last_error()
        _same("dw (exact grid)", 0, dw, dw_ref, f" wgrad variant {v}")


def _per_layer(gpu, H, W, cin, with_res, dt, long_board=False):
    L, lib = _lib()
    n, P = R.NBASE, H * W
    zd, zx = _zero_rows(n)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + cin + int(with_res))
    G = Guards(gpu)
    lay = Layer(g, cin, dt, gpu, n, dmask=not with_res, zero_dmask_row=zd)
    x64 = _acts(g, (n, P, cin), dt, gpu, 0.5 if cin == C else 1.0)
    x64[zx] = 0
    if cin == 16:
        x64[:, :, 10:] = 0
    res64 = _acts(g, (n, P, C), dt, gpu) if with_res else None
    dout64 = _acts(g, (n, P, C), dt, gpu)
    want_dx = cin == C
    add64 = _acts(g, (n, P, C), dt, gpu) if (with_res and want_dx) else None
    x = x64.to(dt).contiguous()
    res = res64.to(dt).contiguous() if with_res else None
    o = _fwd_outputs(G, n, P, dt)
    assert _call_fwd(lib, L, lay, x, res, o, n, H, W, gpu) == 0, lib.mc_last_error()
    G.check("mc_conv_gn_fwd")
    _check_forward_layer(lay, H, W, x64, o, res64, 0)

    dy, dx = G.out((n, P, C), dt), (G.out((n, P, C), dt) if want_dx else None)
    dz = G.out((n, P, C), dt) if with_res else None
    dw, dgn = G.out((9, C, cin), torch.float32), G.out((3, C), torch.float32)
    nws = int(lib.mc_conv_gn_bwd_workspace(n, H, W, cin))
    work = G.work(4 * nws)
    dout = dout64.to(dt).contiguous()
    add = add64.to(dt).contiguous() if add64 is not None else None
    rc = lib.mc_conv_gn_bwd(L.ptr(dout), None, L.ptr(o.rmask), L.ptr(o.y), L.ptr(o.stats), L.ptr(lay.gamma),
                            L.ptr(lay.dmask), L.ptr(x), L.ptr(lay.wT if want_dx else None), L.ptr(add), L.ptr(dy),
                            L.ptr(dz), L.ptr(dx), L.ptr(dw), L.ptr(dgn), L.ptr(work), nws, n, H, W, cin, _dtc(dt),
                            L.stream_ptr(gpu))
    G.check("mc_conv_gn_bwd")
    if long_board and rc != 0:  # refused before anything touched the device; include/mscnn.h states the limit
        assert rc == MS_EINVAL
        assert all(t is None or Guards.untouched(t) for t in (dy, dx, dz, dw, dgn))
    else:
        assert rc == 0, lib.mc_last_error()
        b = R.gn_bwd(dout64, None, o.y.double(), o.stats.double(), R.unpack_bits(o.rmask), lay.p.gamma, lay.dm64, dt)
        if dz is not None:
            _same("dz", 0, dz.double(), b.dz)
        _report("dy", 0, dy, b.dy, R.tol16(b.dy, b.e_dy, dt))
        ref, e = R.dgn_total(b.terms, b.e_terms)
        _report("dgn", 0, dgn, ref, e)
        if want_dx:
            acc, mag = R.dgrad(dy.double(), lay.p.w.permute(0, 2, 1), H, W)
            if add64 is not None:
                ref, e = R.add16_err(acc, R.dgrad_err(mag), add64, dt)
            else:
                ref, e = acc, R.dgrad_err(mag)
            _report("dx", 0, dx, ref, R.tol16(ref, e, dt))
        ref, mag = R.wgrad(dy.double(), x64, H, W)
        _report("dw", 0, dw, ref, R.wgrad_err(mag, n, P))
    if not with_res:
        _grid_checks(lib, L, gpu, H, W, cin, dt, n, long_board)


PER_LAYER = [(h, w, C) for h, w in R.BOARDS_96] + [(h, w, 16) for h, w in R.BOARDS_16]


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize("H,W,cin", PER_LAYER, ids=[f"{h}x{w}-c{c}" for h, w, c in PER_LAYER])
def test_per_layer(gpu, H, W, cin, dt, with_res):
    """mc_conv_gn_fwd, mc_conv_gn_bwd (with mc_conv_wgrad's kernels inside) and mc_conv_wgrad at every tile
    class: all stages under the bound, the exact-grid y and dw bitwise; with and without residual + addend."""
    _per_layer(gpu, H, W, cin, with_res, dt)


@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize("H,W", R.BOARDS_LONG, ids=[f"{h}x{w}" for h, w in R.BOARDS_LONG])
def test_per_layer_longest_boards(gpu, H, W, dt):
    """One row / one column of 512 cells: the results pass, or the entry point returns MS_EINVAL before
    touching the device (the weight gradient's LDS image: include/mscnn.h states the limit)."""
    _per_layer(gpu, H, W, C, False, dt, long_board=True)
    hdr = open(__file__.replace("tests/test_trunk_elementwise_gpu.py", "include/mscnn.h")).read()
    assert "1 x 512" in hdr and "MS_EINVAL" in hdr


@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
def test_per_layer_too_large_board(gpu, dt):
    """23x23 = 529 cells: every per-layer entry point returns MS_EINVAL and writes nothing."""
    L, lib = _lib()
    H, W = R.BOARD_TOO_LARGE
    n, P = 2, H * W
    G = Guards(gpu)
    g = torch.Generator().manual_seed(0)
    lay = Layer(g, C, dt, gpu, n, dmask=False)
    x = _acts(g, (n, P, C), dt, gpu).to(dt)
    o = _fwd_outputs(G, n, P, dt)
    assert _call_fwd(lib, L, lay, x, None, o, n, H, W, gpu) == MS_EINVAL
    dy, dx, dw, dgn = G.out((n, P, C), dt), G.out((n, P, C), dt), G.out((9, C, C), torch.float32), G.out((3, C), torch.float32)
    nws = max(int(lib.mc_conv_gn_bwd_workspace(n, H, W, C)), 4)
    work = G.work(4 * nws)
    st = torch.zeros((n, R.NG, 2), device=gpu)
    rm = torch.zeros((n, P, C // 8), dtype=torch.uint8, device=gpu)
    rc = lib.mc_conv_gn_bwd(L.ptr(x), None, L.ptr(rm), L.ptr(x), L.ptr(st), L.ptr(lay.gamma), None, L.ptr(x),
                            L.ptr(lay.wT), None, L.ptr(dy), None, L.ptr(dx), L.ptr(dw), L.ptr(dgn), L.ptr(work), nws, n,
                            H, W, C, _dtc(dt), L.stream_ptr(gpu))
    assert rc == MS_EINVAL
    rc = lib.mc_conv_wgrad(L.ptr(x), L.ptr(x), L.ptr(dw), L.ptr(work), nws, n, H, W, C, _dtc(dt), L.stream_ptr(gpu))
    assert rc == MS_EINVAL
    G.check("refused calls")
    assert all(Guards.untouched(t) for t in (o.out, o.y, o.stats, o.rmask, dy, dx, dw, dgn))


# ---------------------------------------------------------------------------------------------
# one-launch kernels

class Trunk:
    """A stem layer (cin 16, run through mc_conv_gn_fwd: its output is the stack's x0) and 2 * blocks
    residual layers, with the eight base samples; ``idx`` tiles them to a larger batch."""

    def __init__(self, gpu, H, W, blocks, dt, n, seed, grid=False):
        L, lib = _lib()
        self.gpu, self.H, self.W, self.P, self.dt, self.nb, self.nl = gpu, H, W, H * W, dt, n, 2 * blocks
        g = torch.Generator().manual_seed(seed)
        zd, zx = _zero_rows(n)
        # the stem's "dropout" row of zeros makes sample zx's x0 all zero
        self.stem = Layer(g, 16, dt, gpu, n, dmask=True)
        self.stem.dm64 = torch.ones_like(self.stem.dm64)
        self.stem.dm64[zx] = 0
        self.stem.dmask = self.stem.dm64.float().contiguous()
        self.layers = [Layer(g, C, dt, gpu, n, dmask=(l % 2 == 0), zero_dmask_row=zd) for l in range(self.nl)]
        xs = _acts(g, (n, self.P, 16), dt, gpu)
        xs[:, :, 10:] = 0
        self.grid = None
        if grid:  # exact-grid x0 and first-layer weights: x0 is given, not the stem's output
            self.grid = R.grid_case(n, H, W, C, dt, seed=seed, device=gpu)
            self.layers[0].w = self.grid.w.to(dt).contiguous()
            self.layers[0].bias = self.grid.bias.float().contiguous()
            self.layers[0].p.w, self.layers[0].p.bias = self.grid.w, self.grid.bias
        self.xs64, self.dout64 = xs, _acts(g, (n, self.P, C), dt, gpu)
        self.idx = None

    def tile(self, N):
        self.idx = torch.arange(N, device=self.gpu) % self.nb
        for lay in [self.stem] + self.layers:
            lay.tile(self.idx)

    def n(self):
        return self.nb if self.idx is None else int(self.idx.numel())

    def run_stem(self, G):
        L, lib = _lib()
        n = self.n()
        xs = self.xs64 if self.idx is None else self.xs64[self.idx]
        self.xs = xs.to(self.dt).contiguous()
        self.so = _fwd_outputs(G, n, self.P, self.dt)
        assert _call_fwd(lib, L, self.stem, self.xs, None, self.so, n, self.H, self.W, self.gpu) == 0, lib.mc_last_error()
        G.check("mc_conv_gn_fwd (stem)")
        if self.grid is not None:
            x0 = self.grid.x if self.idx is None else self.grid.x[self.idx]
            return x0.to(self.dt).contiguous()
        return self.so.out

    def forward(self, G, x0, variant, save=True, pooled=True):
        """mc_trunk_fwd_pooled with every output of every layer (``save``), or with none but the last out
        (block outputs through the workspace)."""
        from ms_amd import fused as F
        L, lib = _lib()
        n, P, dt = self.n(), self.P, self.dt
        arr = (L.McFwdLayer * self.nl)()
        outs = []
        for l, lay in enumerate(self.layers):
            if save:
                o = _fwd_outputs(G, n, P, dt)
            else:
                o = R.SimpleNamespace(out=G.out((n, P, C), dt) if l == self.nl - 1 else None, y=None, stats=None, rmask=None)
            outs.append(o)
            arr[l] = L.McFwdLayer(L.ptr(lay.w), L.ptr(lay.bias), L.ptr(lay.gamma), L.ptr(lay.beta), L.ptr(lay.dmask),
                                  L.ptr(o.out), L.ptr(o.y), L.ptr(o.stats), L.ptr(o.rmask))
        nws = int(lib.mc_trunk_fwd_workspace(n, self.H, self.W))
        work = G.work(nws)
        pl = G.out((n, C), torch.float32) if pooled else None
        with F.kernel_variant(F.VARIANT_TRUNK_FWD, variant):
            rc = lib.mc_trunk_fwd_pooled(L.ptr(x0), arr, self.nl, L.ptr(work), nws, L.ptr(pl), n, self.H, self.W, R.EPS,
                                         _dtc(dt), L.stream_ptr(self.gpu))
        assert rc == 0, lib.mc_last_error()
        G.check(f"mc_trunk_fwd_pooled (variant {variant}, save {save})")
        return outs, pl

    def backward(self, G, outs):
        L, lib = _lib()
        n, P, dt, nl = self.n(), self.P, self.dt, self.nl + 1
        arr = (L.McBwdLayer * nl)()
        dys = []
        for li, (lay, o) in enumerate(zip([self.stem] + self.layers, [self.so] + outs)):
            dy = G.out((n, P, C), dt)
            dys.append(dy)
            arr[li] = L.McBwdLayer(L.ptr(o.y), L.ptr(o.stats), L.ptr(lay.gamma), L.ptr(o.rmask), L.ptr(lay.dmask),
                                   L.ptr(lay.wT if li else None), L.ptr(dy))
        dgn = G.out((nl, 3, C), torch.float32)
        nws = int(lib.mc_trunk_bwd_workspace(nl, n, self.H, self.W))
        work = G.work(nws)
        d64 = self.dout64 if self.idx is None else self.dout64[self.idx]
        self.dout = d64.to(dt).contiguous()
        rc = lib.mc_trunk_bwd(L.ptr(self.dout), arr, nl, L.ptr(dgn), L.ptr(work), nws, n, self.H, self.W, _dtc(dt),
                              L.stream_ptr(self.gpu))
        assert rc == 0, lib.mc_last_error()
        G.check("mc_trunk_bwd")
        return dys, dgn

    def check_forward(self, x0, outs, pl, tag):
        x064 = x0.double()
        for l, (lay, o) in enumerate(zip(self.layers, outs)):
            xin = x064 if l == 0 else outs[l - 1].out.double()
            res = None if l % 2 == 0 else (x064 if l == 1 else outs[l - 2].out.double())
            _check_forward_layer(lay, self.H, self.W, xin, o, res, l, tag)
        if self.grid is not None:
            y, _ = R.conv_y(self.grid.x, self.grid.w, self.grid.bias, self.H, self.W)
            _same("y (exact grid)", 0, outs[0].y, R.round16(y, self.dt), tag)
        if pl is not None:
            ref, e = R.pooled(outs[-1].out.double())
            _report("pooled", self.nl - 1, pl, ref, e, tag)

    def check_backward(self, outs, dys, dgn, tag, check_dy=True):
        """Per layer dy and the per-sample dgn terms, top down. A layer's dout is the dgrad of the dy the
        kernel stored for the layer above (+ the skip gradient dz of the block's conv2), rounded to 16 bits
        inside the kernel: known to within a bound, which gn_bwd carries. Returns the per-layer terms."""
        H, W, dt = self.H, self.W, self.dt
        lays, fo = [self.stem] + self.layers, [self.so] + outs
        nl = len(lays)
        dout, e_dout = self.dout.double(), None
        held = {}
        terms = []
        for li in range(nl - 1, -1, -1):
            lay, o = lays[li], fo[li]
            b = R.gn_bwd(dout, e_dout, o.y.double(), o.stats.double(), R.unpack_bits(o.rmask), lay.p.gamma, lay.dm64, dt)
            if check_dy:
                _report("dy", li, dys[li], b.dy, R.tol16(b.dy, b.e_dy, dt), tag)
            terms.append((li, b.terms, b.e_terms))
            if li % 2 == 0 and li >= 2:
                held[li] = (b.dz, b.e_dz)  # the skip gradient of layer li - 2's output
            if li == 0:
                break
            acc, mag = R.dgrad(dys[li].double(), lay.p.w.permute(0, 2, 1), H, W)
            e_acc = R.dgrad_err(mag)
            if li % 2 == 1 and li + 1 in held:  # the block input: dx + dz of the block's conv2
                dout, e = R.add16_err(acc, e_acc, held.pop(li + 1), dt)
                e_dout = R.round16_err(dout, e, dt)
            else:
                dout, e_dout = acc, R.round16_err(acc, e_acc, dt)
        for li, t, e in terms:
            ref, eb = R.dgn_total(t, e)
            _report("dgn", li, dgn[li], ref, eb, tag)
        return {li: (t, e) for li, t, e in terms}


def _variants(P):
    return [(1, "fwd2"), (2, "pp")] if P <= 256 else [(0, "fwd")]


ONE_LAUNCH = [(h, w, v, name) for h, w in R.BOARDS_TRUNK for v, name in _variants(h * w)]


@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize("H,W,variant,name", ONE_LAUNCH, ids=[f"{h}x{w}-{nm}" for h, w, _, nm in ONE_LAUNCH])
def test_one_launch(gpu, H, W, variant, name, dt):
    """mc_trunk_fwd_pooled (2 blocks, every output of every layer) stage by stage per layer, the pooled mean,
    mc_trunk_bwd's per-layer dy and dgn; every call twice, bitwise the same; the forward without saves (block
    outputs through the workspace) bitwise the saving forward's features; the exact-grid first-layer y."""
    G = Guards(gpu)
    t = Trunk(gpu, H, W, 2, dt, R.NBASE, seed=31 * H + W)
    x0 = t.run_stem(G)
    tag = f" [{H}x{W} {DT_ID[dt]} {name}]"
    outs, pl = t.forward(G, x0, variant)
    t.check_forward(x0, outs, pl, tag)
    outs2, pl2 = t.forward(G, x0, variant)
    for l, (a, b) in enumerate(zip(outs, outs2)):
        for k in ("out", "y", "stats", "rmask"):
            _same(f"{k} (second run)", l, getattr(b, k), getattr(a, k), tag)
    _same("pooled (second run)", t.nl - 1, pl2, pl, tag)
    outs3, pl3 = t.forward(G, x0, variant, save=False)
    _same("out (no-save run)", t.nl - 1, outs3[-1].out, outs[-1].out, tag)
    _same("pooled (no-save run)", t.nl - 1, pl3, pl, tag)
    dys, dgn = t.backward(G, outs)
    t.check_backward(outs, dys, dgn, tag)
    dys2, dgn2 = t.backward(G, outs)
    for li, (a, b) in enumerate(zip(dys, dys2)):
        _same("dy (second run)", li, b, a, tag)
    _same("dgn (second run)", -1, dgn2, dgn, tag)
    # exact grid: the first layer's accumulators start from (or end with) the bias
    tg = Trunk(gpu, H, W, 2, dt, R.NBASE, seed=31 * H + W, grid=True)
    x0g = tg.run_stem(G)
    outs_g, pl_g = tg.forward(G, x0g, variant)
    tg.check_forward(x0g, outs_g, pl_g, tag + " grid")


@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
def test_one_launch_too_wide_board(gpu, dt):
    """4x65: mc_trunk_fwd and mc_trunk_bwd return MS_EINVAL (W <= 64) and write nothing."""
    L, lib = _lib()
    H, W = R.BOARD_TOO_WIDE
    G = Guards(gpu)
    t = Trunk(gpu, H, W, 1, dt, 2, seed=1)
    x0 = t.run_stem(G)
    n, P = 2, H * W
    arr = (L.McFwdLayer * 2)()
    outs = [_fwd_outputs(G, n, P, dt) for _ in range(2)]
    for l, (lay, o) in enumerate(zip(t.layers, outs)):
        arr[l] = L.McFwdLayer(L.ptr(lay.w), L.ptr(lay.bias), L.ptr(lay.gamma), L.ptr(lay.beta), L.ptr(lay.dmask),
                              L.ptr(o.out), L.ptr(o.y), L.ptr(o.stats), L.ptr(o.rmask))
    rc = lib.mc_trunk_fwd(L.ptr(x0), arr, 2, None, 0, n, H, W, R.EPS, _dtc(dt), L.stream_ptr(gpu))
    assert rc == MS_EINVAL
    barr = (L.McBwdLayer * 3)()
    dys = [G.out((n, P, C), dt) for _ in range(3)]
    for li, (lay, o) in enumerate(zip([t.stem] + t.layers, [t.so] + outs)):
        barr[li] = L.McBwdLayer(L.ptr(t.so.y), L.ptr(t.so.stats), L.ptr(lay.gamma), L.ptr(t.so.rmask), L.ptr(lay.dmask),
                                L.ptr(lay.wT if li else None), L.ptr(dys[li]))
    dgn, work = G.out((3, 3, C), torch.float32), G.work(1 << 20)
    rc = lib.mc_trunk_bwd(L.ptr(x0), barr, 3, L.ptr(dgn), L.ptr(work), 1 << 20, n, H, W, _dtc(dt), L.stream_ptr(gpu))
    assert rc == MS_EINVAL
    G.check("refused calls")
    assert all(Guards.untouched(t_) for o in outs for t_ in (o.out, o.y, o.stats, o.rmask))
    assert all(Guards.untouched(t_) for t_ in dys + [dgn])
    hdr = open(__file__.replace("tests/test_trunk_elementwise_gpu.py", "include/mscnn.h")).read()
    assert "w_ <= 64" in hdr


# ---------------------------------------------------------------------------------------------
# depth

DEPTH = [(h, w, b, v, nm) for h, w in R.DEPTH_BOARDS for b in R.DEPTH_BLOCKS for v, nm in _variants(h * w)]


@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize("H,W,blocks,variant,name", DEPTH, ids=[f"{h}x{w}-{b}blocks-{nm}" for h, w, b, _, nm in DEPTH])
def test_depth(gpu, H, W, blocks, variant, name, dt):
    """5 blocks (10 layers = PP_MAXL: k_trunk_fwd_pp's bias table is full), 6 and 8 blocks (variant 2 hands
    over to k_trunk_fwd2 and must still pass), three samples: every stage of every layer, both directions."""
    G = Guards(gpu)
    t = Trunk(gpu, H, W, blocks, dt, 3, seed=7 * H + blocks)
    x0 = t.run_stem(G)
    tag = f" [{H}x{W} {DT_ID[dt]} {blocks} blocks {name}]"
    outs, pl = t.forward(G, x0, variant)
    t.check_forward(x0, outs, pl, tag)
    dys, dgn = t.backward(G, outs)
    t.check_backward(outs, dys, dgn, tag)
    outs2, pl2 = t.forward(G, x0, variant)  # determinism: a second run of both directions, bitwise
    for l, (a, b) in enumerate(zip(outs, outs2)):
        for k in ("out", "y", "stats", "rmask"):
            _same(f"{k} (second run)", l, getattr(b, k), getattr(a, k), tag)
    _same("pooled (second run)", t.nl - 1, pl2, pl, tag)
    dys2, dgn2 = t.backward(G, outs)
    for li, (a, b) in enumerate(zip(dys, dys2)):
        _same("dy (second run)", li, b, a, tag)
    _same("dgn (second run)", -1, dgn2, dgn, tag)


def test_depth_too_deep(gpu):
    """9 blocks = 18 layers > MC_TRUNK_MAX_LAYERS: MS_EINVAL from both directions, nothing written."""
    L, lib = _lib()
    dt, H, W, n = torch.float16, 5, 7, 3
    nl = 2 * R.DEPTH_TOO_DEEP
    G = Guards(gpu)
    t = Trunk(gpu, H, W, 1, dt, n, seed=2)
    x0 = t.run_stem(G)
    o = _fwd_outputs(G, n, H * W, dt)
    arr = (L.McFwdLayer * nl)()
    for l in range(nl):
        lay = t.layers[l % 2]
        arr[l] = L.McFwdLayer(L.ptr(lay.w), L.ptr(lay.bias), L.ptr(lay.gamma), L.ptr(lay.beta), L.ptr(lay.dmask),
                              L.ptr(o.out), L.ptr(o.y), L.ptr(o.stats), L.ptr(o.rmask))
    assert lib.mc_trunk_fwd(L.ptr(x0), arr, nl, None, 0, n, H, W, R.EPS, _dtc(dt), L.stream_ptr(gpu)) == MS_EINVAL
    barr = (L.McBwdLayer * (nl + 1))()
    dy, dgn, work = G.out((n, H * W, C), dt), G.out((nl + 1, 3, C), torch.float32), G.work(1 << 20)
    for li in range(nl + 1):
        lay = t.layers[li % 2] if li else t.stem
        barr[li] = L.McBwdLayer(L.ptr(t.so.y), L.ptr(t.so.stats), L.ptr(lay.gamma), L.ptr(t.so.rmask), None,
                                L.ptr(lay.wT if li else None), L.ptr(dy))
    assert lib.mc_trunk_bwd(L.ptr(x0), barr, nl + 1, L.ptr(dgn), L.ptr(work), 1 << 20, n, H, W, _dtc(dt),
                            L.stream_ptr(gpu)) == MS_EINVAL
    assert lib.mc_trunk_bwd_workspace(nl + 1, n, H, W) < 0
    G.check("refused calls")
    assert all(Guards.untouched(t_) for t_ in (o.out, o.y, o.stats, o.rmask, dy, dgn))


# ---------------------------------------------------------------------------------------------
# loops and odd tails

LOOPS = [(h, w, k, v, nm) for h, w in R.PAIR_BOARDS for k in range(4) for v, nm in _variants(h * w)] + \
        [R.ONE_BOARD + (k, 0, "fwd") for k in range(2)]
LOOP_N = {True: ("2cus+1", "2cus+2", "4cus-1", "4cus+3"), False: ("cus+1", "2cus+1")}


@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize("H,W,k,variant,name", LOOPS,
                         ids=[f"{h}x{w}-N{LOOP_N[h * w <= 256][k]}-{nm}" for h, w, k, _, nm in LOOPS])
def test_loop_odd_tail(gpu, H, W, k, variant, name, dt):
    """The persistent loops past one grid, with odd tails: 1 block, the eight checked samples tiled to N.
    Every per-sample output of both directions is bitwise that of the 8-sample run; dgn is within the
    bound of the f64 sums; mc_conv_wgrad at the same N is bitwise on the exact grid."""
    L, lib = _lib()
    cus = _cus(gpu)
    N = (R.pair_ns(cus) if H * W <= 256 else R.one_ns(cus))[k]
    assert (H, W, N) in R.loop_cases(cus)
    tag = f" [{H}x{W} {DT_ID[dt]} {name} N={N}]"
    G = Guards(gpu)
    base = Trunk(gpu, H, W, 1, dt, R.NBASE, seed=5 * H + W)
    x0 = base.run_stem(G)
    outs, pl = base.forward(G, x0, variant)
    base.check_forward(x0, outs, pl, tag + " base")
    dys, dgn = base.backward(G, outs)
    terms = base.check_backward(outs, dys, dgn, tag + " base")

    big = Trunk(gpu, H, W, 1, dt, R.NBASE, seed=5 * H + W)
    big.tile(N)
    idx = big.idx
    G2 = Guards(gpu)
    X0 = big.run_stem(G2)
    for kk in ("out", "y", "stats", "rmask"):
        _same(f"stem {kk} (tiled)", -1, getattr(big.so, kk), getattr(base.so, kk)[idx], tag)
    OUTS, PL = big.forward(G2, X0, variant)
    for l, (a, b) in enumerate(zip(OUTS, outs)):
        for kk in ("out", "y", "stats", "rmask"):
            _same(f"{kk} (tiled)", l, getattr(a, kk), getattr(b, kk)[idx], tag)
    _same("pooled (tiled)", big.nl - 1, PL, pl[idx], tag)
    if H * W <= 256:  # the rollout's forward: nothing saved, block outputs through the workspace
        O3, P3 = big.forward(G2, X0, variant, save=False)
        _same("out (no-save run, tiled)", big.nl - 1, O3[-1].out, outs[-1].out[idx], tag)
        _same("pooled (no-save run, tiled)", big.nl - 1, P3, pl[idx], tag)
    DYS, DGN = big.backward(G2, OUTS)
    for li, (a, b) in enumerate(zip(DYS, dys)):
        _same("dy (tiled)", li, a, b[idx], tag)
    for li, (t, e) in terms.items():
        ref, eb = R.dgn_total(t, e, idx)
        _report("dgn", li, DGN[li], ref, eb, tag)
    del OUTS, DYS, G2
    # mc_conv_wgrad over N samples on the exact grid
    c = R.grid_case(N, H, W, C, dt, seed=100 * H + W, device=gpu)
    G3 = Guards(gpu)
    rc, dw = _wgrad(lib, L, G3, c.dy.to(dt).contiguous(), c.x.to(dt).contiguous(), N, H, W, C, dt, gpu)
    assert rc == 0, lib.mc_last_error()
    G3.check("mc_conv_wgrad (tiled grid)")
    cnt = torch.bincount(c.idx, minlength=R.NBASE).double()
    ref = sum(cnt[i] * R.wgrad(c.dyb[i:i + 1], c.xb[i:i + 1], H, W)[0] for i in range(R.NBASE))
    _same("dw (exact grid)", 0, dw, ref.float(), tag)


# ---------------------------------------------------------------------------------------------
# NaN through the trunk's ReLU

NAN_CASES = [(16, 16, -1, "layer"), (16, 16, 1, "fwd2"), (16, 16, 2, "pp"), (5, 7, 1, "fwd2"), (5, 7, 2, "pp"),
             (18, 18, 0, "fwd")]


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
@pytest.mark.parametrize("H,W,variant,name", NAN_CASES, ids=[f"{h}x{w}-{nm}" for h, w, _, nm in NAN_CASES])
def test_nan_through_relu(gpu, H, W, variant, name, dt, poison):
    """One element of x0 of one sample is NaN (or +inf: inf - inf in the GroupNorm statistics). That sample's
    features are all NaN, with cleared ReLU bits, through each forward kernel -- saving and not -- and the
    other samples are bitwise those of the clean run (include/mscnn.h, as torch.relu; fmaxf gave zeros)."""
    L, lib = _lib()
    P, n, bad_n = H * W, R.NBASE, 3
    tag = f" [{H}x{W} {DT_ID[dt]} {name}]"
    G = Guards(gpu)
    t = Trunk(gpu, H, W, 1, dt, n, seed=3 * H + W)
    x0 = t.run_stem(G).clone()
    xp = x0.clone()
    xp[bad_n, P // 2, 17] = poison
    keep = [i for i in range(n) if i != bad_n]
    if variant < 0:  # mc_conv_gn_fwd
        lay = t.layers[0]
        runs = []
        for x in (x0, xp):
            o = _fwd_outputs(G, n, P, dt)
            assert _call_fwd(lib, L, lay, x, None, o, n, H, W, gpu) == 0
            G.check("mc_conv_gn_fwd")
            runs.append(o)
        clean, pois = runs
        finals = [(clean.out, pois.out, pois.rmask)]
    else:
        finals = []
        for save in (True, False):
            oc, _ = t.forward(G, x0, variant, save=save)
            op, plp = t.forward(G, xp, variant, save=save)
            finals.append((oc[-1].out, op[-1].out, op[-1].rmask))
            assert bool(plp[bad_n].isnan().all()), f"pooled of the poisoned sample is finite{tag}"
    for clean_out, pois_out, rmask in finals:
        assert bool(pois_out[bad_n].isnan().all()), \
            f"{int((~pois_out[bad_n].isnan()).sum())} features of the poisoned sample are not NaN{tag}"
        if rmask is not None:
            assert not bool(rmask[bad_n].any()), f"ReLU bits set where out is NaN{tag}"
        _same("out (other samples)", -1, pois_out[keep], clean_out[keep], tag)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("dt", R.DTYPES, ids=DT_ID.values())
def test_nan_through_wgrad_gn_recompute(gpu, dt, poison):
    """mc_conv_wgrad_gn recomputes a conv1 output from its y and statistics with the forward's ReLU: on a
    poisoned sample it sees the NaN the forward wrote, and on the clean samples it stays bitwise
    mc_conv_wgrad on the forward's x."""
    L, lib = _lib()
    H = W = 16
    P, n, bad_n = 256, R.NBASE, 3
    G = Guards(gpu)
    t = Trunk(gpu, H, W, 1, dt, n, seed=11)
    x0 = t.run_stem(G).clone()
    x0[bad_n, 100, 5] = poison
    lay = t.layers[0]
    o = _fwd_outputs(G, n, P, dt)
    assert _call_fwd(lib, L, lay, x0, None, o, n, H, W, gpu) == 0
    assert bool(o.out[bad_n].isnan().all())
    dy = t.dout64.to(dt).contiguous()

    def run(sel):
        m = len(sel)
        dw = G.out((9, C, C), torch.float32)
        nws = int(lib.mc_conv_gn_bwd_workspace(m, H, W, C))
        work = G.work(4 * nws)
        a = [tt[sel].contiguous() for tt in (dy, o.y, o.stats, lay.dmask, o.out)]
        assert lib.mc_conv_wgrad_gn(L.ptr(a[0]), L.ptr(a[1]), L.ptr(a[2]), L.ptr(lay.gamma), L.ptr(lay.beta), L.ptr(a[3]),
                                    L.ptr(dw), L.ptr(work), nws, m, H, W, _dtc(dt), L.stream_ptr(gpu)) == 0
        dw2 = G.out((9, C, C), torch.float32)
        work2 = G.work(4 * nws)
        assert lib.mc_conv_wgrad(L.ptr(a[0]), L.ptr(a[4]), L.ptr(dw2), L.ptr(work2), nws, m, H, W, C, _dtc(dt),
                                 L.stream_ptr(gpu)) == 0
        G.check("mc_conv_wgrad_gn / mc_conv_wgrad")
        return dw, dw2

    dw, dw2 = run(list(range(n)))
    assert bool(dw.isnan().all()) and bool(dw2.isnan().all()), "the poisoned sample's NaN did not reach dw"
    keep = [i for i in range(n) if i != bad_n]
    dw, dw2 = run(keep)
    _same("dw (recompute, clean samples)", 0, dw, dw2)
    assert bool(dw.isfinite().all())
