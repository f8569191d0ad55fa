"""An f64 restatement of the residual-CNN trunk layer (csrc/mscnn.hip, mscnn_bwd.hip, mscnn_trunk.hip;
include/mscnn.h mc_conv_gn_fwd / mc_conv_gn_bwd / mc_conv_wgrad / mc_trunk_fwd / mc_trunk_bwd) as plain
torch ops on any device, in STAGES, each with a running bound of what f32 arithmetic may do to it.
tests/test_trunk_ref.py pins every stage to PyTorch (conv2d, group_norm, autograd) in f64 on the CPU and
shows that the bounds accept an f32 evaluation and reject single-element mistakes;
tests/test_trunk_elementwise_gpu.py compares the HIP kernels with it element by element.

Stages. A stage takes the tensors the kernel itself stored upstream (its 16-bit y, its f32 statistics, its
ReLU bits, its 16-bit dy), so errors do not compound and no ReLU decision is re-derived:
  y      conv3x3(x, w) + bias                        conv_y
  stats  mean, rstd per (sample, group) of that y    gn_stats
  out    relu(y16 * a + b + res) * d                 gn_out       (a = gamma rstd, b = beta - mean a)
  pooled mean over the pixels of the kernel's out    pooled
  gn_bwd dz, dy, d gamma / d beta / d bias           gn_bwd       (formulas: header of csrc/mscnn_bwd.hip)
  dgrad  dx = sum_tap shift(dy16) . wT[tap] + addend dgrad
  wgrad  dw[tap][co][ci] = sum dy16 x16              wgrad
Every function returns the f64 value and, beside it, either ``mag`` (the same expression with every term
replaced by its absolute value) or the bound ``e`` itself.

The bound, with u = 2^-24:
  * an f32 sum of n terms is off by at most 2 n u sum|terms|, in any order: one full ulp per add, so it does
    not depend on how an MFMA rounds inside (sum_err);
  * any other f32 operation is off by at most 2 u |result| (op_err);
  * rsqrtf by 2^-22 relative (the instruction's documented 1 ulp, doubled);
  * an input known only to within e contributes e times the factor it is multiplied by.
A 16-bit output then passes iff |got - ref| <= half_ulp16(|ref| + e) + 2 e, an f32 output iff
|got - ref| <= e (tol16 / bad): no element is exempt and no norm is taken. The bounds are derived from
the operations the kernels perform, not measured; where a value is rounded to 16 bits inside a kernel
and not stored (the dx and the skip gradient between two layers of mc_trunk_bwd), the rounding's
half-ulp is added to the running bound (round16_err).

The exact grid (grid_case): x, w, dy integers in [-3, 3], bias an integer in [-4, 4]. Every partial sum
of a y or a dw element is an integer below 2^24, exact in f32 in any order, so ysave of a first layer and
mc_conv_wgrad's dw must equal the reference bit for bit (assert_grid_preconditions).

Shape lists of the GPU test are functions of the CU count (loop_cases), so the CPU test checks the
grid's preconditions for every one of them without a device."""
from __future__ import annotations

from types import SimpleNamespace

import torch

C, NG, GC = 96, 6, 16
U = 2.0 ** -24
RSQRT_REL = 2.0 ** -22
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the eps the C ABI receives (a float argument)
DTYPES = (torch.bfloat16, torch.float16)


# ---------------------------------------------------------------------------------------------
# bounds

def half_ulp16(a, dtype):
    """Half a unit in the last place of ``dtype`` at magnitude ``a`` (f64 >= 0): 2^-8 of the binade for
    bf16 (8 significand bits), 2^-11 for fp16; below the smallest normal the spacing stays that of the
    lowest binade (fp16 subnormals: 2^-25)."""
    bits, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    ex = torch.frexp(a)[1].double() - 1  # a = m 2^(ex), m in [1, 2)
    ex = torch.where(a > 0, ex, torch.full_like(ex, emin)).clamp_min(emin)
    return torch.exp2(ex - bits)


def tol16(ref, e, dtype):
    return half_ulp16(ref.abs() + e, dtype) + 2 * e


def round16_err(ref, e, dtype):
    """The bound after a value known to within e is rounded to 16 bits inside a kernel."""
    return e + half_ulp16(ref.abs() + e, dtype)


def bad(got, ref, tol):
    """Mask of the failing elements; a NaN on either side fails."""
    return ~((got.double() - ref).abs() <= tol)


def sum_err(n, mag):
    return 2.0 * n * U * mag


def op_err(mag):
    return 2.0 * U * mag


def round16(x, dtype):
    """f64 -> f32 -> one round-to-nearest-even cast (exact inputs: what the kernel's cast gives)."""
    return x.float().to(dtype)


# ---------------------------------------------------------------------------------------------
# stages

def shifted(x, H, W, tap, sign=1):
    """x [N, P, c] -> the value at pixel p + sign * s(tap), zero off the board; tap = 3 (dy + 1) + (dx + 1)."""
    N, P, c = x.shape
    ky, kx = tap // 3, tap % 3
    if sign < 0:
        ky, kx = 2 - ky, 2 - kx
    xp = torch.nn.functional.pad(x.view(N, H, W, c), (0, 0, 1, 1, 1, 1))
    return xp[:, ky:ky + H, kx:kx + W, :].reshape(N, P, c)


def conv_y(x, w, bias, H, W):
    """Stage y. x [N, P, cin], w [9, 96, cin] (tap, co, ci), bias [96], all f64 -> (y, mag) [N, P, 96]."""
    N, P, cin = x.shape
    assert P == H * W and w.shape == (9, C, cin)
    y = bias.expand(N, P, C).clone()
    mag = bias.abs().expand(N, P, C).clone()
    for tap in range(9):
        xs = shifted(x, H, W, tap)
        y += xs @ w[tap].t()
        mag += xs.abs() @ w[tap].abs().t()
    return y, mag


def y_err(mag, cin):
    return sum_err(9 * cin + 1, mag)


def _groups(t):
    N, P, _ = t.shape
    return t.view(N, P, NG, GC).permute(0, 2, 1, 3).reshape(N, NG, P * GC)


def gn_stats(y, e_y, eps=EPS):
    """Stage stats. y: the f64 conv output before its 16-bit rounding, e_y its bound (the kernel's f32
    accumulators are within e_y of y). -> (stats, e) [N, 6, 2] = mean, rstd = rsqrt(var + eps), two-pass."""
    n = y.shape[1] * GC
    yg, eg = _groups(y), _groups(e_y)
    mean = yg.mean(-1)
    e_sum = eg.sum(-1) + sum_err(n, yg.abs().sum(-1) + eg.sum(-1))
    e_mean = e_sum / n
    e_mean = e_mean + 2 * op_err(mean.abs() + e_mean)  # 1 / (16 P) rounded, and the product
    d = yg - mean[..., None]
    e_d = eg + e_mean[..., None]
    e_d = e_d + op_err(d.abs() + e_d)  # the subtraction (the bias add is one of the conv's 9 cin + 1 terms)
    sq = d * d
    e_sq = 2 * d.abs() * e_d + e_d * e_d
    e_sq = e_sq + op_err(sq + e_sq)
    var = sq.mean(-1)
    e_var = (e_sq.sum(-1) + sum_err(n, sq.sum(-1) + e_sq.sum(-1))) / n
    v = var + eps
    e_v = e_var + 3 * op_err(v + e_var)  # 1 / (16 P), the product, + eps
    assert bool((e_v < v).all()), "variance not resolved: the rstd bound does not exist"
    rstd = v.rsqrt()
    e_r = 0.5 * e_v * (v - e_v) ** -1.5
    e_r = e_r + RSQRT_REL * (rstd + e_r)
    return torch.stack([mean, rstd], -1), torch.stack([e_mean, e_r], -1)


def _per_channel(stats):
    """stats [N, 6, 2] -> mean, rstd [N, 96]."""
    return stats[..., 0].repeat_interleave(GC, 1), stats[..., 1].repeat_interleave(GC, 1)


def gn_out(y16, stats, gamma, beta, res=None, dmask=None):
    """Stage out, from the kernel's own y (16-bit values as f64) and statistics (f32 values as f64):
    a = gamma rstd, b = beta - mean a, out = relu(fma(y, a, b) + res) * d -> (out, e) [N, P, 96]."""
    m, r = _per_channel(stats)
    a = gamma * r
    e_a = op_err(a.abs())
    ma = m * a
    e_ma = m.abs() * e_a
    e_ma = e_ma + op_err(ma.abs() + e_ma)
    b = beta - ma
    e_b = e_ma + op_err(b.abs() + e_ma)
    t = y16 * a[:, None] + b[:, None]
    e_t = y16.abs() * e_a[:, None] + e_b[:, None]
    e_t = e_t + op_err(t.abs() + e_t)
    z = t if res is None else t + res
    e_z = e_t + op_err(z.abs() + e_t)
    o = torch.relu(z)  # 1-Lipschitz: the bound carries over
    if dmask is None:
        return o, e_z
    d = dmask[:, None]
    o = o * d
    e_o = e_z * d.abs()
    return o, e_o + op_err(o.abs() + e_o)


def pooled(out16):
    """Stage pooled: the f32 mean over the pixels of the kernel's own 16-bit out -> (pooled, e) [N, 96]."""
    P = out16.shape[1]
    ref = out16.mean(1)
    e = sum_err(P, out16.abs().sum(1)) / P
    return ref, e + 2 * op_err(ref.abs() + e)  # 1 / P rounded, and the product


def unpack_bits(rmask):
    """u8 [N, P, 12] -> bool [N, P, 96]: bit j of byte c8 is channel 8 c8 + j."""
    sh = torch.arange(8, device=rmask.device, dtype=torch.int32)
    return (((rmask.to(torch.int32)[..., None] >> sh) & 1) != 0).reshape(*rmask.shape[:-1], C)


def gn_bwd(dout, e_dout, y16, stats, bits, gamma, dmask, dtype):
    """Stage gn_bwd (csrc/mscnn_bwd.hip header): with yhat = (y - mean) rstd,
      dz = bits * dout * dmask                                   (rounded to 16 bits by the kernel)
      S1 = sum_p dz, S2 = sum_p dz yhat, S3 = sum_p yhat         per (sample, channel)
      m1, m2 = the group means of gamma S1, gamma S2 over 16 P elements
      dy = rstd gamma dz - rstd^2 m2 (y - mean) - rstd m1 = fma(A, dz, fma(Bg, y, Cg))
      A = rstd gamma, Bg = -rstd^2 m2, Cg = rstd (rstd m2 mean - m1)
      d gamma = sum_n S2, d beta = sum_n S1, d bias = sum_n rstd (gamma S1 - P m1 - m2 S3) (= sum dy).
    dout is known to within e_dout (None: exactly; dz is then the kernel's 16-bit dz bit for bit and its
    bound 0). Returns a namespace: dz, e_dz, dy, e_dy [N, P, 96]; terms, e_terms [N, 3, 96], the
    per-sample contributions to dgn (dgn_total sums them)."""
    N, P, _ = y16.shape
    n = GC * P
    m, r = _per_channel(stats)
    dm = torch.ones_like(m) if dmask is None else dmask
    o = SimpleNamespace()
    d = dout * dm[:, None]
    if e_dout is None:
        d32 = d.float().double()  # dout (16 bits) x dmask (f32) is exact in f64: this is the f32 product
        o.dz = torch.where(bits, round16(d32, dtype).double(), torch.zeros_like(d))
        o.e_dz = torch.zeros_like(d)
    else:
        e_d = e_dout * dm[:, None].abs()
        e_d = e_d + op_err(d.abs() + e_d)
        o.dz = torch.where(bits, d, torch.zeros_like(d))
        o.e_dz = torch.where(bits, round16_err(d, e_d, dtype), torch.zeros_like(d))
    dz, e_dz = o.dz, o.e_dz
    yc = y16 - m[:, None]
    yh = yc * r[:, None]
    e_yh = op_err(yc.abs()) * r[:, None] + op_err(yh.abs() * (1 + 2 * U))
    S1 = dz.sum(1)
    e_S1 = e_dz.sum(1) + sum_err(P, (dz.abs() + e_dz).sum(1))
    t2 = dz * yh
    e_t2 = e_dz * yh.abs() + dz.abs() * e_yh + e_dz * e_yh
    S2 = t2.sum(1)
    e_S2 = e_t2.sum(1) + sum_err(P, (t2.abs() + e_t2).sum(1))
    S3 = yh.sum(1)
    e_S3 = e_yh.sum(1) + sum_err(P, (yh.abs() + e_yh).sum(1))

    def gmean(S, e_S):  # group mean of gamma S over the 16 P elements: 16 channel terms, then / (16 P)
        gS = gamma * S
        e_g = gamma.abs() * e_S
        e_g = e_g + op_err(gS.abs() + e_g)
        tot = gS.view(N, NG, GC).sum(-1)
        e_tot = e_g.view(N, NG, GC).sum(-1) + sum_err(GC, (gS.abs() + e_g).view(N, NG, GC).sum(-1))
        mm = tot / n
        e_mm = e_tot / n
        e_mm = e_mm + 2 * op_err(mm.abs() + e_mm)
        return gS, e_g, mm.repeat_interleave(GC, 1), e_mm.repeat_interleave(GC, 1)

    gS1, e_gS1, m1, e_m1 = gmean(S1, e_S1)
    _, _, m2, e_m2 = gmean(S2, e_S2)
    A = r * gamma
    e_A = op_err(A.abs())
    Bg = -r * r * m2
    e_Bg = r * r * e_m2
    e_Bg = e_Bg + 2 * op_err(Bg.abs() + e_Bg)
    q = r * m2 * m
    e_q = (r * m).abs() * e_m2
    e_q = e_q + 2 * op_err(q.abs() + e_q)
    s = q - m1
    e_s = e_q + e_m1
    e_s = e_s + op_err(s.abs() + e_s)
    Cg = r * s
    e_Cg = r * e_s
    e_Cg = e_Cg + op_err(Cg.abs() + e_Cg)
    inner = Bg[:, None] * y16 + Cg[:, None]
    e_in = e_Bg[:, None] * y16.abs() + e_Cg[:, None]
    e_in = e_in + op_err(inner.abs() + e_in)
    o.dy = A[:, None] * dz + inner
    e_dy = e_A[:, None] * (dz.abs() + e_dz) + A.abs()[:, None] * e_dz + e_in
    o.e_dy = e_dy + op_err(o.dy.abs() + e_dy)
    # d bias of one sample: rstd (gamma S1 - P m1 - m2 S3)
    pm1 = P * m1
    e_pm1 = P * e_m1
    e_pm1 = e_pm1 + op_err(pm1.abs() + e_pm1)
    ms3 = m2 * S3
    e_ms3 = m2.abs() * e_S3 + S3.abs() * e_m2 + e_m2 * e_S3
    e_ms3 = e_ms3 + op_err(ms3.abs() + e_ms3)
    par = gS1 - pm1 - ms3
    e_par = e_gS1 + e_pm1 + e_ms3
    e_par = e_par + 2 * op_err(gS1.abs() + pm1.abs() + ms3.abs() + e_par)  # two subtractions
    B = r * par
    e_B = r * e_par
    e_B = e_B + op_err(B.abs() + e_B)
    o.terms = torch.stack([S2, S1, B], 1)
    o.e_terms = torch.stack([e_S2, e_S1, e_B], 1)
    return o


def dgn_total(terms, e_terms, idx=None):
    """dgn [3, 96] of a batch whose sample i is base sample idx[i] (None: the batch itself): the
    per-sample terms summed over the batch, one more f32 sum of N terms in any order."""
    if idx is not None:
        terms, e_terms = terms[idx], e_terms[idx]
    N = terms.shape[0]
    return terms.sum(0), e_terms.sum(0) + sum_err(N, (terms.abs() + e_terms).sum(0))


def dgrad(dy16, wT, H, W):
    """Stage dgrad before the addend: dx[q][ci] = sum_tap sum_co dy[q - s(tap)][co] wT[tap][ci][co],
    wT [9, 96 ci, 96 co] -> (dx, mag) [N, P, 96]."""
    dx = torch.zeros_like(dy16)
    mag = torch.zeros_like(dy16)
    for tap in range(9):
        ds = shifted(dy16, H, W, tap, sign=-1)
        dx += ds @ wT[tap].t()
        mag += ds.abs() @ wT[tap].abs().t()
    return dx, mag


def dgrad_err(mag):
    return sum_err(9 * C, mag)


def add16_err(ref_a, e_a, b, dtype):
    """The kernels' dx + addend: the f32 accumulator (ref_a within e_a) is rounded to 16 bits, widened,
    added to the 16-bit b (exact, or a (ref, e) pair) in f32; the caller's check / round16_err covers the
    last rounding. -> (ref, e) before it."""
    b, e_b = b if isinstance(b, tuple) else (b, torch.zeros_like(b))
    e = round16_err(ref_a, e_a, dtype) + e_b
    ref = ref_a + b
    return ref, e + op_err(ref.abs() + e)


def wgrad(dy16, x16, H, W):
    """Stage wgrad: dw[tap][co][ci] = sum_{n, p} dy[n][p][co] x[n][p + s(tap)][ci] -> (dw, mag) [9, 96, cin]."""
    N, P, cin = x16.shape
    dyf = dy16.reshape(N * P, C)
    dw, mag = [], []
    for tap in range(9):
        xs = shifted(x16, H, W, tap).reshape(N * P, cin)
        dw.append(dyf.t() @ xs)
        mag.append(dyf.abs().t() @ xs.abs())
    return torch.stack(dw), torch.stack(mag)


def wgrad_err(mag, N, P):
    return sum_err(N * P, mag)


# ---------------------------------------------------------------------------------------------
# the exact grid

ALIGNED = list(range(5, C, 12))  # output channels whose weights are positive: |y| reaches the thousands


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def grid_case(N, H, W, cin, dtype, seed, device="cpu", check=True):
    """x [N, P, cin], dy [N, P, 96], w [9, 96, cin] integers in [-3, 3], bias [96] an integer in [-4, 4],
    as f64 on ``device``. The stem's (cin 16) channels 10 .. 15 are zero, as the observation's. Sample 0 is
    non-negative and the ALIGNED output channels have positive weights, so that y there needs more than
    11 significant bits and the cast to fp16 rounds too; the corner pixels and the last pixel of every
    sample are non-zero in x and dy."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = H * W
    c = SimpleNamespace(N=N, H=H, W=W, P=P, cin=cin, dtype=dtype)
    nb = min(N, NBASE)  # N > NBASE: the NBASE distinct samples tiled, sample i = base sample i % NBASE
    c.x = _ints(g, (nb, P, cin), -3, 3)
    c.dy = _ints(g, (nb, P, C), -3, 3)
    c.w = _ints(g, (9, C, cin), -3, 3)
    c.bias = _ints(g, (C,), -4, 4)
    c.x[0] = c.x[0].abs()
    c.w[:, ALIGNED] = c.w[:, ALIGNED].abs().clamp_min(1)
    edge = sorted({0, W - 1, P - W, P - 1})
    for t in (c.x, c.dy):
        t[:, edge] = torch.where(t[:, edge] == 0, torch.ones_like(t[:, edge]), t[:, edge])
    if cin == 16:
        c.x[:, :, 10:] = 0
        c.w[:, :, 10:] = 0
    for k in ("x", "dy", "w", "bias"):
        setattr(c, k, getattr(c, k).to(device))
    c.idx = torch.arange(N, device=device) % nb
    c.xb, c.dyb = c.x, c.dy  # the distinct samples
    if N > nb:
        c.x, c.dy = c.x[c.idx], c.dy[c.idx]
    if check:
        assert_grid_preconditions(c)
    return c


def assert_grid_preconditions(c):
    """What the bitwise comparisons rest on (conditions on the inputs, not tolerances), and what makes a
    wrong tap or a dropped pixel visible."""
    for name in ("xb", "dyb", "w"):  # (a tiled batch holds the distinct samples xb, dyb and nothing else)
        t = getattr(c, name)
        assert torch.equal(round16(t, c.dtype).double(), t), f"{name} is not exact in {c.dtype}"
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3, name
    assert torch.equal(c.x, c.xb[c.idx]) and torch.equal(c.dy, c.dyb[c.idx])
    assert torch.equal(c.bias, c.bias.round()) and float(c.bias.abs().max()) <= 4
    y, mag = conv_y(c.xb, c.w, c.bias, c.H, c.W)
    assert float(mag.max()) < 2.0 ** 24, "a partial sum of y may leave the exact f32 integers"
    assert torch.equal(y.float().double(), y)
    assert 9 * c.N * c.P < 2 ** 24, f"wgrad: 9 N P = {9 * c.N * c.P} >= 2^24"
    cnt = torch.bincount(c.idx, minlength=c.xb.shape[0]).double()
    wmag = sum(cnt[i] * wgrad(c.dyb[i:i + 1], c.xb[i:i + 1], c.H, c.W)[1] for i in range(c.xb.shape[0]))
    assert float(wmag.max()) < 2.0 ** 24, "a partial sum of dw may leave the exact f32 integers"
    P, W = c.P, c.W
    for p_ in sorted({0, W - 1, P - W, P - 1}):
        assert bool((c.xb[:, p_, :10] != 0).all()) and bool((c.dyb[:, p_] != 0).all()), f"pixel {p_} has a zero"
    if c.cin == C and min(c.H, c.W) >= 3:  # the 16-bit cast of y rounds somewhere, in either type
        assert bool((round16(y, c.dtype).double() != y).any()), f"y is exact in {c.dtype} everywhere"


# ---------------------------------------------------------------------------------------------
# general (rounded-random) operands

def random_params(g, cin, device="cpu"):
    """One layer's parameters as f64 holding f32 / 16-bit-roundable values: w [9, 96, cin] ~ N(0, 1 / (9 cin)),
    gamma uniform(-1.5, 1.5) with channel 7 exactly 0, beta and bias ~ N(0, 0.3^2)."""
    p = SimpleNamespace()
    p.w = torch.randn((9, C, cin), generator=g) / (3.0 * cin ** 0.5)
    p.gamma = torch.rand(C, generator=g) * 3.0 - 1.5
    p.gamma[7] = 0.0
    p.beta = torch.randn(C, generator=g) * 0.3
    p.bias = torch.randn(C, generator=g) * 0.3
    for k, v in vars(p).items():
        setattr(p, k, v.float().double().to(device))
    return p


def random_dmask(g, N, device="cpu", zero_row=None, p=0.25):
    """Dropout2d scale [N, 96]: 0 with probability p, else 1 / (1 - p) as f32; row ``zero_row`` all 0."""
    d = (torch.rand((N, C), generator=g) >= p).float() * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    if zero_row is not None:
        d[zero_row] = 0
    return d.double().to(device)


def q16(t, dtype):
    """The 16-bit rounding of a tensor, as f64."""
    return t.float().to(dtype).double()


# ---------------------------------------------------------------------------------------------
# shapes of the GPU test

NBASE = 8                       # distinct samples of every case
ZERO_DMASK_ROW, ZERO_X_ROW = 2, 5
BOARDS_96 = [(1, 1), (1, 9), (9, 1), (5, 7), (8, 16), (3, 43), (12, 12), (15, 17), (16, 16), (6, 43), (18, 18),
             (6, 64), (7, 55), (30, 16), (16, 32), (8, 64)]
BOARDS_16 = [(5, 7), (12, 12), (16, 16), (18, 18)]
BOARDS_LONG = [(1, 512), (512, 1)]
BOARD_TOO_LARGE = (23, 23)
BOARD_TOO_WIDE = (4, 65)
BOARDS_TRUNK = [b for b in BOARDS_96 if b[1] <= 64]
DEPTH_BOARDS = [(5, 7), (16, 16)]
DEPTH_BLOCKS = [5, 6, 8]        # 5 blocks = 10 layers = PP_MAXL; above it variant 2 falls back to k_trunk_fwd2
DEPTH_TOO_DEEP = 9              # 18 layers > MC_TRUNK_MAX_LAYERS
PAIR_BOARDS = [(5, 7), (9, 9)]  # k_trunk_fwd2 / k_trunk_fwd_pp: one workgroup a CU, a sample pair at a time
ONE_BOARD = (18, 18)            # k_trunk_fwd / k_trunk_bwd above 256 cells: one workgroup a CU


def pair_ns(cus):
    """More than one iteration of the pair loop with an odd tail (team B one sample short), an even one, an
    odd tail on the second and on the third iteration of some workgroups."""
    return [2 * cus + 1, 2 * cus + 2, 4 * cus - 1, 4 * cus + 3]


def one_ns(cus):
    return [cus + 1, 2 * cus + 1]


def loop_cases(cus):
    """(H, W, N) of every loop / odd-tail case."""
    return [(h, w, n) for h, w in PAIR_BOARDS for n in pair_ns(cus)] + [ONE_BOARD + (n,) for n in one_ns(cus)]


def grid_cases(cus):
    """(N, H, W, cin) of every exact-grid case the GPU test builds."""
    out = [(NBASE, h, w, C) for h, w in BOARDS_96] + [(NBASE, h, w, 16) for h, w in BOARDS_16]
    out += [(NBASE, h, w, C) for h, w in BOARDS_LONG]
    return out + [(n, h, w, C) for h, w, n in loop_cases(cus)]
