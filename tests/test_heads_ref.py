"""Pins tests/heads_ref.py (the f64 heads that the HIP kernels of csrc/msheads.hip are compared
with bit for bit) to PyTorch itself on the CPU: two nn.Sequential(Conv2d(96, 96, 1), ReLU,
Conv2d(96, 1, 1)) in f64, the mine head on f.detach(), and autograd. On the exact grid f64 sums
are exact in any order, so every comparison is torch.equal. Also checks, without a device, that
every shape tests/test_heads_gpu.py builds for 256 and 304 CUs meets the grid's preconditions."""
from __future__ import annotations

import pytest
import torch

import heads_ref as R


def _torch_heads(c):
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(96, 96, 1), torch.nn.ReLU(),  # noqa: E731
                                     torch.nn.Conv2d(96, 1, 1)).double()
    pol, mine = mk(), mk()
    with torch.no_grad():
        for i, h in enumerate((pol, mine)):
            sl = slice(i * 96, (i + 1) * 96)
            h[0].weight.copy_(c.w1[sl].reshape(96, 96, 1, 1))
            h[0].bias.copy_(c.b1[sl])
            h[2].weight.copy_(c.w2[sl].reshape(1, 96, 1, 1))
            h[2].bias.copy_(c.b2[i:i + 1])
    return pol, mine


@pytest.mark.parametrize("M,P", [(65 * 17, 17), (600, 12), (5, 1)])
@pytest.mark.parametrize("with_dlm", [True, False])
def test_heads_ref_is_torch_autograd(M, P, with_dlm):
    c = R.grid_case(M, P, torch.bfloat16, seed=M + P, dlm=with_dlm)
    r = R.heads_ref(c)
    n = M // P
    pol, mine = _torch_heads(c)
    f = c.f.clone().requires_grad_(True)
    x = f.view(n, P, 96).permute(0, 2, 1).unsqueeze(-1)  # NCHW [n, 96, P, 1]
    lp = pol(x).reshape(M)
    lm = mine(x.detach()).reshape(M)
    pooled = f.view(n, P, 96).mean(1)
    dpool = c.gadd * P
    loss = (lp * c.dlp).sum() + (pooled * dpool).sum()
    if with_dlm:
        loss = loss + (lm * c.dlm).sum()
    loss.backward()
    assert torch.equal(lp.detach(), r.lp) and torch.equal(lm.detach(), r.lm)
    assert torch.equal(f.grad, r.df_exact)
    assert torch.equal(r.df, r.df_exact.float().to(c.dtype))
    for i, h in enumerate((pol, mine)):
        sl = slice(i * 96, (i + 1) * 96)
        if i == 1 and not with_dlm:  # no gradient reaches the mine head: the reference's rows are 0
            assert all(p.grad is None for p in h.parameters())
            assert not r.dW1[sl].any() and not r.db1[sl].any() and not r.dw2[sl].any() and r.db2[1] == 0
            continue
        assert torch.equal(h[0].weight.grad.reshape(96, 96), r.dW1[sl]), i
        assert torch.equal(h[0].bias.grad, r.db1[sl]), i
        assert torch.equal(h[2].weight.grad.reshape(96), r.dw2[sl]), i
        assert torch.equal(h[2].bias.grad.reshape(()), r.db2[i]), i


def test_relu_edge_is_exercised():
    """Some hidden activations are exactly 0, where torch's ReLU gradient is 0: dh is 0 there."""
    c = R.grid_case(65 * 17, 17, torch.float16, seed=1)
    r = R.heads_ref(c)
    z = r.h == 0
    assert z.any() and not r.dh[z].any()


def test_preconditions_catch_a_grid_that_is_too_wide():
    c = R.grid_case(600, 12, torch.bfloat16, seed=2)
    c.f[3, 5] = 0.25 + 2.0 ** -10  # not a bf16 value
    with pytest.raises(AssertionError, match="f is not exact"):
        R.assert_exact_preconditions(c)
    c.dtype = torch.float16  # ... but an fp16 one
    R.assert_exact_preconditions(c)
    c = R.grid_case(600, 12, torch.bfloat16, seed=2)
    c.gadd[1] = c.gadd[0]
    with pytest.raises(AssertionError, match="adjacent gadd"):
        R.assert_exact_preconditions(c)


@pytest.mark.parametrize("cus", [256, 304])
def test_gpu_shapes_meet_the_preconditions(cus):
    """Every backward shape of the GPU test, in both element types, at the seed it uses there
    (grid_case asserts the preconditions); the forward rows are a subset of the same draws."""
    shapes = sorted(set(R.all_bwd_shapes(cus)) | {(m, 1) for m in R.fwd_rows(cus)})
    assert max(m for m, _ in shapes) <= (6 * cus + 1) * R.TRB
    for M, P in shapes:
        assert M % P == 0, (M, P)
        c = R.grid_case(M, P, torch.bfloat16, seed=M, check=False)
        r = R.heads_ref(c)
        for dt in (torch.bfloat16, torch.float16):
            c.dtype = dt
            R.assert_exact_preconditions(c, r)
    # the ring shapes reach every case of the counted waits: nloc below NS - 1, NS - 1, NS, above
    seen = set()
    for M, _ in R.bwd_ring_shapes(cus):
        _, _, lo, hi = R.geometry(M, cus)
        seen |= {lo, hi}
    assert {1, 2, 3, 4, 5, 6, 7} <= seen
