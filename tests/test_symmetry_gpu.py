"""Board symmetries on the device (csrc/mssym.hip, ms_amd/symmetry.py) against the numpy
restatement of tests/symmetry_ref.py: ms_sym_gather bit for bit on every plane (NaN payloads,
-0.0 and denormals in the labels; repeats and NULL rows; each plane NULL in turn; guard rows), its
bad rows, ms_sym_expand and ms_sym_mean, SymmetricModel's equivariance on exact-arithmetic stubs
and its equality with a torch-op restatement on a real network, and the augmented imitation update."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import symmetry_ref as R

pytestmark = pytest.mark.gpu

PLANES = ("codes", "mask", "best", "labels", "kind")
DTYPES = dict(codes=np.uint8, mask=np.uint8, best=np.uint8, labels=np.uint32, kind=np.uint8)
SENTINEL = 0xA5
# f32 bit patterns that an arithmetic copy could change: quiet and signalling NaNs with payloads,
# -0.0, the smallest and the largest denormal of either sign, infinities
SPECIAL = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0xFF9ABCDE, 0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF,
                    0x7F800000, 0xFF800000, 0x3F800000], dtype=np.uint32)
B_SRC = 257


def _sources(H, W, seed):
    """Random source planes of B_SRC rows as numpy arrays (labels as uint32 bit patterns)."""
    rng = np.random.default_rng(seed)
    A = H * W
    labels = rng.integers(0, 1 << 32, size=(B_SRC, A), dtype=np.uint64).astype(np.uint32)
    special = rng.random((B_SRC, A)) < 0.3
    labels[special] = SPECIAL[rng.integers(0, len(SPECIAL), size=int(special.sum()))]
    return dict(codes=rng.integers(0, 256, size=(B_SRC, A), dtype=np.uint8),
                mask=rng.integers(0, 2, size=(B_SRC, A), dtype=np.uint8),
                best=rng.integers(0, 2, size=(B_SRC, A), dtype=np.uint8), labels=labels,
                kind=rng.integers(0, 3, size=(B_SRC,), dtype=np.uint8))


def _to_device(src, gpu, H, W, rows=slice(None)):
    """The tensors ExpertBuffer holds: codes [B, H, W], a bool mask, f32 labels."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v[rows])).to(gpu) for k, v in src.items() if k != "labels"}
    t["labels"] = torch.from_numpy(np.ascontiguousarray(src["labels"][rows]).view(np.int32)).to(gpu).view(torch.float32)
    t["codes"] = t["codes"].view(-1, H, W)
    t["mask"] = t["mask"].view(torch.bool)
    return t


def _guarded(like, n, gpu):
    """{plane: (whole, inner)}: n rows between two guard rows, every byte SENTINEL."""
    out = {}
    for k, t in like.items():
        whole = torch.full((n + 2,) + tuple(t.shape[1:]), SENTINEL, dtype=torch.uint8, device=gpu)
        if t.dtype == torch.float32:
            whole = torch.full((n + 2,) + tuple(t.shape[1:]) + (4,), SENTINEL, dtype=torch.uint8,
                               device=gpu).view(torch.float32).squeeze(-1)
        elif t.dtype == torch.bool:
            whole = whole.view(torch.bool)
        out[k] = (whole, whole[1:n + 1])
    return out


def _bits(t):
    """A device plane as numpy bytes / uint32 bit patterns, rows flattened."""
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32).reshape(t.shape[0], -1)
    return t.view(torch.uint8).cpu().numpy().reshape(t.shape[0], -1) if t.dim() > 1 else t.cpu().numpy()


def _want(src, rows, g, H, W):
    return {k: (src[k][rows] if k == "kind" else R.rows_transform(src[k][rows], g, H, W)) for k in PLANES}


def _untouched(whole):
    b = _bits(whole)
    return bool((b[0] == (SENTINEL if b.dtype == np.uint8 else 0xA5A5A5A5)).all()
                and (b[-1] == (SENTINEL if b.dtype == np.uint8 else 0xA5A5A5A5)).all())


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gather_equals_numpy_bit_for_bit(gpu, shape):
    from ms_amd.symmetry import group_size, sym_gather
    H, W = shape
    G = group_size(H, W)
    src = _sources(H, W, seed=H * 64 + W)
    dev = _to_device(src, gpu, H, W)
    for n in (1, 3, 5, 257):  # workgroups of four rows: tails of 1, 3 and 1 rows
        g = ((np.arange(n) + n) % G).astype(np.uint8)  # every valid value in turn
        rows = (np.arange(n, dtype=np.int64) * 5 + 3) % B_SRC  # not in order
        rows[n // 2] = rows[0]  # a repeat
        if n == 257:
            rows[-1] = rows[-2] = B_SRC - 1
        want = _want(src, rows, g, H, W)
        guard = _guarded(dev, n, gpu)
        got = sym_gather(torch.from_numpy(rows).to(gpu), torch.from_numpy(g).to(gpu), H, W, **dev, status=True,
                         out={k: inner for k, (_, inner) in guard.items()})
        for k in PLANES:
            assert got[k].data_ptr() == guard[k][1].data_ptr() and got[k].dtype == dev[k].dtype
            assert np.array_equal(_bits(got[k]), want[k]), (n, k)
            assert _untouched(guard[k][0]), (n, k)
        assert not got["status"].any()
        # rows = NULL: the identity over a source of exactly n rows; outputs allocated by the call
        part = _to_device(src, gpu, H, W, slice(0, n))
        got = sym_gather(None, torch.from_numpy(g).to(gpu), H, W, **part)
        want = _want(src, np.arange(n), g, H, W)
        for k in PLANES:
            assert got[k].shape == part[k].shape and got[k].dtype == part[k].dtype
            assert np.array_equal(_bits(got[k]), want[k]), (n, k, "identity rows")


@pytest.mark.parametrize("shape", ((5, 7), (16, 16)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_gather_skips_a_plane_whose_input_or_output_is_null(gpu, shape):
    from ms_amd.symmetry import group_size, sym_gather
    H, W = shape
    n, G = 5, group_size(H, W)
    src = _sources(H, W, seed=7)
    dev = _to_device(src, gpu, H, W)
    g = (np.arange(n) % G).astype(np.uint8)
    rows = np.array([4, 0, 256, 4, 9], dtype=np.int64)
    want = _want(src, rows, g, H, W)
    tr, tg = torch.from_numpy(rows).to(gpu), torch.from_numpy(g).to(gpu)
    for skipped in PLANES:
        for null_side in ("input", "output"):
            guard = _guarded(dev, n, gpu)
            ins = {k: v for k, v in dev.items() if not (null_side == "input" and k == skipped)}
            outs = {k: inner for k, (_, inner) in guard.items() if not (null_side == "output" and k == skipped)}
            got = sym_gather(tr, tg, H, W, **ins, out=outs)
            assert skipped not in got
            for k in PLANES:
                whole, inner = guard[k]
                assert _untouched(whole), (skipped, null_side, k)
                if k == skipped:
                    assert (_bits(inner).view(np.uint8) == SENTINEL).all(), (skipped, null_side)
                else:
                    assert np.array_equal(_bits(inner), want[k]), (skipped, null_side, k)


@pytest.mark.parametrize("shape", ((5, 7), (4, 4)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_gather_bad_rows_are_zero_and_flagged(gpu, shape):
    from ms_amd.symmetry import sym_gather
    H, W = shape
    src = _sources(H, W, seed=11)
    dev = _to_device(src, gpu, H, W)
    #                 ok  -1  ok  B_src ok  g=8 g=4  ok  2^40  -2^40  g=255 ok
    rows = np.array([0, -1, 1, B_SRC, 2, 3, 4, 5, 1 << 40, -(1 << 40), 6, 256], dtype=np.int64)
    g = np.array([1, 0, 2, 0, 3, 8, 4, 0, 1, 1, 255, 3], dtype=np.uint8)
    bad = np.array([0, 1, 0, 1, 0, 1, int(H != W), 0, 1, 1, 1, 0], dtype=bool)
    n = len(rows)
    guard = _guarded(dev, n, gpu)
    got = sym_gather(torch.from_numpy(rows).to(gpu), torch.from_numpy(g).to(gpu), H, W, **dev, status=True,
                     out={k: inner for k, (_, inner) in guard.items()})
    assert np.array_equal(got["status"].cpu().numpy(), bad.astype(np.uint8))
    good = ~bad
    want = _want(src, rows[good], g[good], H, W)
    for k in PLANES:
        b = _bits(got[k])
        assert not b[bad].any(), k  # every plane zero, kind 0: bc_update gives the row weight 0
        assert np.array_equal(b[good], want[k]), k  # the neighbours are what they would be alone
        assert _untouched(guard[k][0]), k


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_expand_and_mean_equal_numpy_bit_for_bit(gpu, shape):
    from ms_amd.symmetry import group_size, sym_expand, sym_mean
    H, W = shape
    A, Gmax = H * W, group_size(H, W)
    rng = np.random.default_rng(H * 64 + W + 1)
    for n in (1, 5, 257) if shape in ((16, 16), (5, 7)) else (5,):
        codes = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
        tc = torch.from_numpy(codes).to(gpu)
        for G in sorted({1, 4, Gmax}):
            imgs = sym_expand(tc, G)
            assert imgs.shape == (G, n, H, W) and imgs.dtype == torch.uint8
            assert np.array_equal(imgs.cpu().numpy(), R.expand(codes, G)), (n, G)
            x = (rng.standard_normal((G, n, A)) * 10.0 ** rng.integers(-3, 4, size=(G, n, A))).astype(np.float32)
            got = sym_mean(torch.from_numpy(x).to(gpu), H, W)
            assert got.shape == (n, A) and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy().view(np.uint32), R.mean(x, H, W).view(np.uint32)), (n, G)
            # G images of one plane average back to the plane exactly: u8 codes through the kernel,
            # and arbitrary f32 values (3 * f would round; the pairwise tree only doubles)
            back = sym_mean(imgs.float().reshape(G, n, A), H, W)
            assert torch.equal(back, tc.float().reshape(n, A)), (n, G)
            f = x[0].reshape(n, H, W)
            fx = torch.from_numpy(np.ascontiguousarray(R.expand(f, G))).to(gpu).reshape(G, n, A)
            assert np.array_equal(sym_mean(fx, H, W).cpu().numpy().view(np.uint32), f.reshape(n, A).view(np.uint32))
        assert torch.equal(sym_expand(tc), sym_expand(tc, Gmax))
    # the per-board scalar case (the value): H = W = 1
    v = rng.standard_normal((Gmax, 7, 1)).astype(np.float32)
    assert np.array_equal(sym_mean(torch.from_numpy(v).to(gpu), 1, 1).cpu().numpy(), R.mean(v[:, :, :], 1, 1))


def test_group_of_eight_needs_a_square_board(gpu):
    from ms_amd.symmetry import sym_expand, sym_mean
    codes = torch.zeros((3, 5, 7), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError, match="square"):
        sym_expand(codes, 8)
    with pytest.raises(ValueError, match="square"):
        sym_mean(torch.zeros((8, 3, 35), device=gpu), 5, 7)
    with pytest.raises(ValueError):
        sym_expand(codes, 2)
    assert sym_expand(codes, 4).shape == (4, 3, 5, 7) and sym_expand(codes).shape[0] == 4


# ---- SymmetricModel ----

class ConvStub(nn.Module):
    """A policy whose outputs are exact in f32: one 3x3 convolution with small integer weights on
    the one-hot obs for the policy logits, another for the mine logits (both as a sum over
    unfolded taps), and a value that weighs the logits by the cell index. Every number is an
    integer far below 2^24, so any order of summation gives the same bits."""

    def __init__(self, w_policy, w_mine, value_by_cell: bool):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))
        self.register_buffer("wp", torch.as_tensor(w_policy, dtype=torch.float32).reshape(1, 90, 1))
        self.register_buffer("wm", torch.as_tensor(w_mine, dtype=torch.float32).reshape(1, 90, 1))
        self.value_by_cell = value_by_cell

    def forward(self, x, return_mine=False):
        from ms_amd.fused import codes_to_obs
        if x.dtype == torch.uint8:
            x = codes_to_obs(x)
        n, _, H, W = x.shape
        taps = F.unfold(x, 3, padding=1)  # [n, 10 * 9, A]
        logits = (taps * self.wp).sum(1)
        weight = torch.arange(H * W, dtype=torch.float32, device=x.device) if self.value_by_cell else 1.0
        value = (logits * weight).sum(1)
        if return_mine:
            return logits, value, (taps * self.wm).sum(1).view(n, 1, H, W)
        return logits, value


def _plain_weights(seed):
    """[10, 3, 3] integers in -4..4 with no symmetry."""
    return np.random.default_rng(seed).integers(-4, 5, size=(10, 3, 3)).astype(np.float32)


def _d4_weights(seed):
    """[10, 3, 3] integers, each channel's kernel invariant under all eight symmetries."""
    a = np.random.default_rng(seed).integers(-4, 5, size=(10, 3)).astype(np.float32)
    w = np.empty((10, 3, 3), dtype=np.float32)
    w[:, 1, 1] = a[:, 0]
    w[:, [0, 1, 1, 2], [1, 0, 2, 1]] = a[:, 1:2]
    w[:, [0, 0, 2, 2], [0, 2, 0, 2]] = a[:, 2:3]
    return w


def _t(x, h):
    """T_h on the last two axes of a device tensor, through the numpy restatement."""
    return torch.from_numpy(np.ascontiguousarray(R.transform(x.cpu().numpy(), h))).to(x.device)


@pytest.mark.parametrize("shape", ((4, 4), (5, 7)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_wrapped_stub_is_equivariant(gpu, shape):
    from ms_amd.symmetry import SymmetricModel, group_size
    H, W = shape
    n, G = 6, group_size(H, W)
    codes = torch.from_numpy(np.random.default_rng(5).integers(0, 10, size=(n, H, W), dtype=np.uint8)).to(gpu)
    stub = ConvStub(_plain_weights(1), _plain_weights(2), value_by_cell=True).to(gpu).eval()
    S = SymmetricModel(stub).eval()
    assert len(list(S.parameters())) == 1 and next(S.parameters()).device == codes.device
    lg, v, mine = S(codes, return_mine=True)
    assert lg.shape == (n, H * W) and v.shape == (n,) and mine.shape == (n, 1, H, W)
    assert lg.dtype == v.dtype == mine.dtype == torch.float32
    assert len(S(codes)) == 2 and torch.equal(S(codes)[0], lg)
    p, pv = stub(codes)
    plain_differs = 0
    for h in range(G):
        th = _t(codes, h)
        lg_h, v_h, mine_h = S(th, return_mine=True)
        assert torch.equal(lg_h.view(n, H, W), _t(lg.view(n, H, W), h)), h
        assert torch.equal(mine_h, _t(mine, h)), h
        assert torch.equal(v_h, v), h
        p_h, pv_h = stub(th)
        plain_differs += int(not torch.equal(p_h.view(n, H, W), _t(p.view(n, H, W), h))) + int(not torch.equal(pv_h, pv))
    assert plain_differs >= G  # the stub alone is not equivariant: the wrapper is what makes it so
    # a stub that is symmetric already is returned unchanged
    sym = ConvStub(_d4_weights(3), _d4_weights(4), value_by_cell=False).to(gpu).eval()
    a, b = SymmetricModel(sym)(codes, return_mine=True), sym(codes, return_mine=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y.reshape(x.shape))
    assert a[0].abs().sum() > 0


def _torch_ensemble(model, codes):
    """SymmetricModel restated with torch ops: the same [G * n] batch by flip / transpose, one
    forward, every image's outputs moved back, the same pairwise tree."""
    n, H, W = codes.shape
    G = 8 if H == W else 4

    def t(x, g):
        if g & 4:
            x = x.transpose(-1, -2)
        if g & 1:
            x = x.flip(-2)
        if g & 2:
            x = x.flip(-1)
        return x
    batch = torch.stack([t(codes, g) for g in range(G)]).reshape(G * n, H, W).contiguous()
    with torch.no_grad():
        lg, v, mine = model(batch, return_mine=True)

    def tree(y):
        if len(y) == 4:
            return ((y[0] + y[1]) + (y[2] + y[3])) * 0.25
        return (((y[0] + y[1]) + (y[2] + y[3])) + ((y[4] + y[5]) + (y[6] + y[7]))) * 0.125
    lg, mine, v = lg.float().view(G, n, H, W), mine.float().view(G, n, H, W), v.float().view(G, n)
    inv = [R.inverse(g) for g in range(G)]
    return (tree([t(lg[g], inv[g]) for g in range(G)]).reshape(n, H * W), tree([v[g] for g in range(G)]),
            tree([t(mine[g], inv[g]) for g in range(G)]).reshape(n, 1, H, W))


def test_wrapped_network_equals_the_torch_restatement(gpu):
    """A real residual network in fp32 at 9x9, n = 5: the same input batch and the same order of
    the sum, so the outputs are equal bit for bit; f32 obs and u8 codes give the same outputs."""
    from ms_amd.fused import codes_to_obs
    from ms_amd.models import build_model
    from ms_amd.symmetry import SymmetricModel
    torch.manual_seed(0)
    model = build_model("cnn_residual", obs_shape=(10, 9, 9),
                        model_cfg=dict(stem_channels=96, blocks=2, dropout=0.05, value_hidden=32)).to(gpu).eval()
    codes = torch.from_numpy(np.random.default_rng(9).integers(0, 10, size=(5, 9, 9), dtype=np.uint8)).to(gpu)
    S = SymmetricModel(model)
    got = S(codes, return_mine=True)
    want = _torch_ensemble(model, codes)
    for name, a, b in zip(("logits", "value", "mine"), got, want):
        assert a.shape == b.shape and a.dtype == torch.float32, name
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    from_obs = S(codes_to_obs(codes), return_mine=True)
    for a, b in zip(got, from_obs):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], model(codes)[0])  # the network alone is not symmetric
    assert not got[0].requires_grad
    S.train()  # the wrapped model is a submodule: train() and eval() reach it
    assert model.training
    S.eval()
    assert not model.training and not S.training


def test_evaluate_vec_takes_the_wrapped_model(gpu):
    from ms_amd import EnvConfig
    from ms_amd.eval import evaluate_vec
    from ms_amd.models import build_model
    from ms_amd.symmetry import SymmetricModel
    torch.manual_seed(0)
    model = build_model("cnn", obs_shape=(10, 8, 8), model_cfg={}).to(gpu)
    m = evaluate_vec(SymmetricModel(model), EnvConfig(H=8, W=8, mine_count=10), episodes=16, seed=0, num_envs=16)
    print(m)
    for k in ("win_rate", "win_ci_low", "win_ci_high", "avg_steps", "avg_progress", "invalid_rate", "belief_auroc",
              "belief_ece"):
        assert np.isfinite(m[k]), k
    assert m["invalid_rate"] == 0.0 and m["episodes"] == 16.0 and m["avg_steps"] >= 1.0


# ---- augmented imitation update: 8x8x10, 32 envs x 8 steps ----

AH = AW = 8
AN, AT = 32, 8


@pytest.fixture(scope="module")
def small_buffer(gpu):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd.imitate import collect_expert
    vec = VecMinesweeper(AN, EnvConfig(H=AH, W=AW, mine_count=10), seed=0, device=gpu)
    return collect_expert(vec, AT, budget=1 << 12, method="grouped", explore=0.0, seed=3)


def test_buffer_gather_with_a_symmetry(gpu, small_buffer):
    b = small_buffer
    B = len(b)
    gen = torch.Generator(device=gpu).manual_seed(1)
    rows = torch.randperm(B, device=gpu, generator=gen)[:100]
    g = torch.randint(0, 8, (100,), dtype=torch.uint8, device=gpu, generator=gen)
    d = b.gather(rows, g)
    plain = b.gather(rows)
    assert set(d) == set(plain) == set(b.FIELDS) | {"rows"} and d["rows"] is rows
    for k in b.FIELDS:
        assert d[k].shape == plain[k].shape and d[k].dtype == plain[k].dtype, k
        assert torch.equal(plain[k], getattr(b, k)[rows]), k  # g = None is still the five index ops
    assert (plain["kind"] != 0).any() and plain["best"].any()
    assert not (d["best"].bool() & ~d["mask"]).any()
    assert torch.equal(d["best"].sum(1), plain["best"].sum(1)) and torch.equal(d["kind"], plain["kind"])
    assert torch.equal(d["mask"].sum(1), plain["mask"].sum(1))
    assert torch.equal(d["codes"].reshape(100, -1) == 0, d["mask"])  # hidden cells are the legal ones
    gn = g.cpu().numpy()
    for k in ("codes", "mask", "best", "labels"):
        want = R.rows_transform(_bits(plain[k]), gn, AH, AW)
        assert np.array_equal(_bits(d[k]), want), k
    ident = b.gather(rows, torch.zeros(100, dtype=torch.uint8, device=gpu))
    for k in b.FIELDS:
        assert torch.equal(ident[k], plain[k]), k


def _augmented_run(gpu, buffer, augment, monkeypatch):
    from ms_amd.imitate import BCConfig, ExpertBuffer, bc_update
    from ms_amd.train import PPOTrainConfig, Trainer
    cfg = PPOTrainConfig(H=AH, W=AW, mine_count=10, num_envs=AN, steps_per_env=AT, aux_mine_weight=0.05,
                         aux_mine_calib_weight=0.01)
    model_d = {"name": "cnn_residual", "stem_channels": 96, "blocks": 1, "dropout": 0.05, "value_hidden": 32}
    tr = Trainer(cfg, {}, model_d, {}, seed=0, amp="fp16", device=gpu)
    seen = []
    gather = ExpertBuffer.gather

    def recording(self, rows, g=None):
        seen.append((rows.clone(), None if g is None else g.clone()))
        return gather(self, rows, g)
    monkeypatch.setattr(ExpertBuffer, "gather", recording)
    bc = BCConfig(mini_batches=4, epochs=2, aux_mine_weight=0.05, aux_mine_calib_weight=0.01, seed=5, augment=augment)
    st = bc_update(tr.model, buffer, tr.opt, bc, tr.amp_dtype, tr.scaler, counter=2)
    monkeypatch.setattr(ExpertBuffer, "gather", gather)
    return st, {k: v.detach().clone() for k, v in tr.model.state_dict().items()}, seen


def test_augmented_update(gpu, small_buffer, monkeypatch):
    st1, p1, seen1 = _augmented_run(gpu, small_buffer, True, monkeypatch)
    st2, p2, seen2 = _augmented_run(gpu, small_buffer, True, monkeypatch)
    st0, p0, seen0 = _augmented_run(gpu, small_buffer, False, monkeypatch)
    print(st1, st0)
    assert st1["bad_rows"] == 0.0 and all(np.isfinite(v) for v in st1.values())
    assert st1 == st2  # the same seeds: the same update, to the last bit
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k
    assert len(seen1) == len(seen0) == 8  # 2 epochs x 4 minibatches
    for (r1, g1), (r0, g0) in zip(seen1, seen0):
        assert torch.equal(r1, r0) and g0 is None  # the permutation does not depend on augment
        assert g1.dtype == torch.uint8 and g1.shape == r1.shape and int(g1.max()) < 8
    gs = torch.cat([g for _, g in seen1])
    assert len(torch.unique(gs)) == 8  # 512 draws: every element of the group
    # a fresh orientation per epoch: the two epochs give the rows different symmetries
    e0 = torch.empty(len(small_buffer), dtype=torch.uint8, device=gpu)
    e1 = e0.clone()
    for i, (r, g) in enumerate(seen1):
        (e0 if i < 4 else e1)[r] = g
    assert not torch.equal(e0, e1)
    assert any(not torch.equal(p1[k], p0[k]) for k in p1)  # and the update is not the plain one
