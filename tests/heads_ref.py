"""An f64 restatement of the policy / mine heads (csrc/msheads.hip, include/mscnn.h mc_heads_fwd and
mc_heads_bwd) as plain torch ops, with no tiling and no kernels, and the inputs on which the HIP
kernels must agree with it bit for bit. tests/test_heads_ref.py pins it to PyTorch's own Conv2d
heads and autograd in f64; tests/test_heads_gpu.py compares the kernels with it.

The exact grid. Every operand is drawn from a small set of dyadic values (GRID below). On such
values each product and each partial sum of an output is a multiple of that output's unit (UNITS)
and, as long as the sum of the absolute terms stays below 2^24 units, is exactly representable in
f32 -- in whatever order MFMAs, in-lane accumulators, per-workgroup partials and the reduction add
them. The kernels' f32 outputs must then equal the f64 ones exactly, and df must equal the exact
sum after one round-to-nearest-even cast to the 16-bit type. ``assert_exact_preconditions`` checks
the condition on every generated case: it is a condition on the inputs, not a tolerance.
With independent signs |df| stays below 8 at a step of 1/32 and the bf16 cast would be exact
everywhere, so eight columns of the policy W1 are sign-aligned with w2 (ALIGNED): there df reaches
26 and about 1.4 % of all df elements (in 60 % of the rows) are rounded, most of them exact ties.
The fp16 cast (11 bits) is exact on this grid: fp16's rounding of df is not exercised.

Shapes. The lists of (M, P) that the GPU test runs are built here from the CU count, so that the
CPU test can check the preconditions of every one of them without a device."""
from __future__ import annotations

from types import SimpleNamespace

import torch

C, NH = 96, 192
TR, TRB = 128, 64          # rows per forward / backward tile (csrc/msheads.hip)
NS, HR_S = 5, 4            # ring slots of k_heads_bwd, slices of k_heads_reduce
PART = NH * C + 2 * NH     # floats of one workgroup's partial: dW1 | dw2 | db1
LAST = 37                  # rows of the partial last tile of the tile / reduce shapes

# operand -> (magnitudes, share of zeros); signs are drawn uniformly
GRID = {
    "f": ((0.25, 0.5, 0.75, 1.0), 0.25),
    "w1": ((0.25, 0.5, 1.0), 0.25),
    "b1": ((0.5, 1.0, 2.0), 0.0),
    "w2": ((0.25, 0.5, 1.0), 0.0),
    "dl": ((0.5, 1.0), 0.10),
}
B2 = (0.375, -1.25)
GADD_K = 8  # gadd = k / 8 for k in -8 .. 8
ALIGNED = list(range(5, 96, 12))  # eight feature columns of the policy W1, see grid_case
# the smallest step of each operand's grid and, from them, of every term of each output
_U = {"f": 0.25, "w1": 0.25, "b1": 0.5, "w2": 0.25, "b2": 0.125, "dl": 0.5, "gadd": 0.125}
UNITS = {
    "h": min(_U["f"] * _U["w1"], _U["b1"]),                 # f . W1 + b1
    "logit": min(_U["f"] * _U["w1"] * _U["w2"], _U["b2"]),  # relu(h) . w2 + b2
    "dh": _U["dl"] * _U["w2"],
    "df": min(_U["dl"] * _U["w2"] * _U["w1"], _U["gadd"]),  # dh_p . W1_p + gadd
    "dW1": _U["dl"] * _U["w2"] * _U["f"],                   # dh^T . f
    "db1": _U["dl"] * _U["w2"],
    "dw2": _U["f"] * _U["w1"] * _U["dl"],                   # relu(h)^T . dl
}


def _draw(g, shape, name):
    vals, pzero = GRID[name]
    v = torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=g)]
    v = v * (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    if pzero > 0:
        v = v * (torch.rand(shape, generator=g) >= pzero).double()
    return v


def grid_case(M, P, dtype, seed, gadd=True, dlm=True, device="cpu", check=True):
    """The operands of one heads call on the exact grid, as f64 tensors on ``device``:
    f [M, 96], w1 [192, 96] (policy rows first), b1 / w2 [192], b2 [2], dlp / dlm [M],
    gadd [M / P, 96]; dlm / gadd None when not asked for. Row M - 1 and the first row of the last
    backward tile get non-zero logit gradients, adjacent samples' gadd rows differ in every
    channel. ``check``: run assert_exact_preconditions on the case."""
    assert M > 0 and P > 0 and M % P == 0
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = SimpleNamespace(M=M, P=P, dtype=dtype, dlm=None, gadd=None)
    c.f = _draw(g, (M, C), "f")
    c.w1 = _draw(g, (NH, C), "w1")
    c.b1 = _draw(g, (NH,), "b1")
    c.w2 = _draw(g, (NH,), "w2")
    c.b2 = torch.tensor(B2, dtype=torch.float64)
    # Elsewhere |df| stays below 8 at a step of 1/32, which bf16 holds exactly. In the ALIGNED columns
    # the policy W1 has no zeros and the sign of its channel's w2, so df = dh_p W1_p adds up there
    # and needs 9 or more significant bits: the kernel's cast to bf16 rounds (mostly exact ties).
    mag = torch.where(c.w1[:C, ALIGNED] == 0, torch.full((), 0.5, dtype=torch.float64), c.w1[:C, ALIGNED].abs())
    c.w1[:C, ALIGNED] = mag * c.w2[:C].sign()[:, None]
    edge = [M - 1, (M - 1) // TRB * TRB]
    c.dlp = _draw(g, (M,), "dl")
    c.dlp[edge] = torch.where(c.dlp[edge] == 0, torch.full((2,), -0.5, dtype=torch.float64), c.dlp[edge])
    if dlm:
        c.dlm = _draw(g, (M,), "dl")
        c.dlm[edge] = torch.where(c.dlm[edge] == 0, torch.full((2,), 1.0, dtype=torch.float64), c.dlm[edge])
    if gadd:
        n = M // P
        k0 = torch.randint(0, 2 * GADD_K + 1, (1, C), generator=g)
        step = torch.randint(1, 2 * GADD_K + 1, (n, C), generator=g)  # never 0 mod 17: neighbours differ
        step[0] = 0
        c.gadd = ((k0 + step.cumsum(0)) % (2 * GADD_K + 1) - GADD_K).double() / GADD_K
    for k, v in vars(c).items():
        if torch.is_tensor(v):
            setattr(c, k, v.to(device))
    if check:
        assert_exact_preconditions(c)
    return c


def round16(x, dtype):
    """The exact f64 value -> f32 (exact on the grid) -> one round-to-nearest-even cast."""
    return x.float().to(dtype)


def heads_ref(c):
    """Both directions of both heads in f64: h = f W1^T + b1, the logits lp / lm [M], dh =
    dl w2 [h > 0] (the mine half 0 without dlm), df_exact = dh_p W1_p (+ gadd[row // P]) and its
    16-bit rounding df, dW1 [192, 96], db1, dw2 [192], db2 [2] (= sum dl)."""
    r = SimpleNamespace()
    r.h = c.f @ c.w1.t() + c.b1
    a = torch.relu(r.h)
    r.lp = a[:, :C] @ c.w2[:C] + c.b2[0]
    r.lm = a[:, C:] @ c.w2[C:] + c.b2[1]
    dlm = c.dlm if c.dlm is not None else torch.zeros_like(c.dlp)
    dl = torch.cat([c.dlp[:, None].expand(-1, C), dlm[:, None].expand(-1, C)], 1)
    r.dh = dl * c.w2 * (r.h > 0).double()
    r.df_exact = r.dh[:, :C] @ c.w1[:C]
    if c.gadd is not None:
        r.df_exact = r.df_exact + c.gadd.repeat_interleave(c.P, 0)
    r.df = round16(r.df_exact, c.dtype)
    r.dW1 = r.dh.t() @ c.f
    r.db1 = r.dh.sum(0)
    r.dw2 = torch.cat([a[:, :C].t() @ c.dlp, a[:, C:].t() @ dlm])
    r.db2 = torch.stack([c.dlp.sum(), dlm.sum()])
    return r


def abs_term_sums(c, r):
    """Per output, the largest sum of absolute terms over its elements (an upper bound of every
    partial sum, in any order)."""
    a = torch.relu(r.h)
    dlm = c.dlm if c.dlm is not None else torch.zeros_like(c.dlp)
    adl = torch.stack([c.dlp.abs(), dlm.abs()], 1)
    s = {
        "h": (c.f.abs() @ c.w1.abs().t() + c.b1.abs()).max(),
        "logit": torch.maximum(a[:, :C] @ c.w2[:C].abs() + abs(B2[0]), a[:, C:] @ c.w2[C:].abs() + abs(B2[1])).max(),
        "df": (r.dh[:, :C].abs() @ c.w1[:C].abs()
               + (c.gadd.abs().repeat_interleave(c.P, 0) if c.gadd is not None else 0)).max(),
        "dW1": (r.dh.abs().t() @ c.f.abs()).max(),
        "db1": r.dh.abs().sum(0).max(),
        "dw2": torch.maximum(a[:, :C].t() @ adl[:, 0], a[:, C:].t() @ adl[:, 1]).max(),
    }
    return {k: float(v) for k, v in s.items()}


def assert_exact_preconditions(c, r=None):
    """What the bitwise comparison rests on, and what makes errors visible; see the module text."""
    r = heads_ref(c) if r is None else r
    # the 16-bit operands survive the cast unchanged
    for name, t in (("f", c.f), ("w1", c.w1), ("dh", r.dh)):
        assert torch.equal(t.float().to(c.dtype).double(), t), f"{name} is not exact in {c.dtype}"
    for name, t in (("b1", c.b1), ("w2", c.w2), ("b2", c.b2), ("dlp", c.dlp), ("dlm", c.dlm), ("gadd", c.gadd)):
        assert t is None or torch.equal(t.float().double(), t), name
    # every partial sum is a multiple of the output's unit below 2^24 units
    for name, s in abs_term_sums(c, r).items():
        assert s < 2.0 ** 24 * UNITS[name], f"{name}: sum |terms| {s} >= 2^24 x {UNITS[name]} (M {c.M})"
    for name in ("h", "df_exact", "dW1", "db1", "dw2", "lp", "lm"):
        t = getattr(r, name)
        assert torch.equal(t.float().double(), t), f"{name} is not exact in f32"
    # inputs on which a wrong row, boundary or tile shows
    act = r.h > 0
    for row in (c.M - 1, (c.M - 1) // TRB * TRB):
        assert float(c.dlp[row]) != 0 and bool(act[row, :C].any()), f"row {row}: policy head inactive"
        assert bool(act[row, C:].any()), f"row {row}: mine head inactive"
        assert c.dlm is None or float(c.dlm[row]) != 0, f"row {row}: dlm = 0"
    if c.gadd is not None and c.gadd.shape[0] > 1:
        assert bool((c.gadd[1:] != c.gadd[:-1]).all()), "adjacent gadd rows share a channel"
    tail = c.f[-(TRB + 1):]
    assert torch.unique(tail, dim=0).shape[0] == tail.shape[0], "two of the last 65 f rows are equal"
    if c.dtype == torch.bfloat16 and c.M >= TRB:  # the final rounding of df is exercised
        assert bool((round16(r.df_exact, c.dtype).double() != r.df_exact).any()), "df is exact in bf16 everywhere"
    share0 = float((r.h == 0).double().mean())
    assert c.M < 1000 or share0 > 0, "no hidden activation is exactly 0"


# ---------------------------------------------------------------------------------------------
# Shapes of the GPU test, from the CU count (= the backward's largest grid).

def geometry(M, cus):
    """(ntiles, G, smallest and largest nloc) of k_heads_bwd at M rows: G = min(ntiles, cus)
    workgroups, workgroup b runs the tiles b, b + G, ..."""
    ntiles = (M + TRB - 1) // TRB
    G = min(ntiles, cus)
    return ntiles, G, ntiles // G, (ntiles + G - 1) // G


def pick_P(M):
    """A sample length that divides M: the smallest divisor in 16 .. 512 (gadd by LDS-DMA), else
    the largest below 16 (plain loads)."""
    for p in range(16, 513):
        if M % p == 0:
            return p
    return max(p for p in range(1, 16) if M % p == 0)


def fwd_rows(cus):
    return [1, 31, 32, 33, 97, 127, 128, 129, 2 * cus * TR + 33]  # the last: a grid-stride second pass


def bwd_tile_shapes(cus):
    """Tile and reduce edges: single-tile M, then G = ntiles around HR_S and 4 HR_S with a last
    tile of LAST rows."""
    ms = [1, 5, 63, 64, 65, 127, 129] + [(nt - 1) * TRB + LAST for nt in (2, 3, 4, 5, 15, 16, 17, 33)]
    return [(m, pick_P(m)) for m in ms]


RING_KJ = ((1, 1), (3, 1), (4, 0), (4, 1), (5, 1), (6, 1), (3, -1), (4, -1))  # j = -1: cus - 1
RING_P = 17  # five samples per tile, unaligned: the LDS-DMA kernel, as on the production boards


def ring_rows(ntiles, P):
    """The smallest multiple of P whose last tile, tile ntiles - 1, is partial (P < 64)."""
    assert P < TRB - 1
    return -(-((ntiles - 1) * TRB + 1) // P) * P


def bwd_ring_shapes(cus):
    """ntiles = k cus + j: workgroups of one launch differ in nloc across the ring's cases."""
    return [(ring_rows(k * cus + (j if j >= 0 else cus - 1), RING_P), RING_P) for k, j in RING_KJ]


GADD_P = (1, 12, 15, 16, 17, 20, 81, 256, 480)


def bwd_gadd_shapes(cus):
    """Every gadd path at a small M (at least three samples and 150 rows) and past 4 cus tiles,
    then one sample with P >= 16 (the DMA window clamped to the buffer's end)."""
    out = []
    for P in GADD_P:
        out.append((max(3, -(-150 // P)) * P, P))
        out.append((-(-(4 * cus * TRB + 1) // P) * P, P))
    return out + [(100, 100), (4 * cus * TRB + LAST, 4 * cus * TRB + LAST)]


def bwd_optional_shapes(cus):
    return [(153, 17), (ring_rows(4 * cus + 1, RING_P), RING_P)]


def all_bwd_shapes(cus):
    return bwd_tile_shapes(cus) + bwd_ring_shapes(cus) + bwd_gadd_shapes(cus) + bwd_optional_shapes(cus)
