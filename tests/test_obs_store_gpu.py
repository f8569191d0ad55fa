"""The obs plane stores (csrc/msenv_board.h store_plane4 / store_plane1, whatever form
MS_OBS_STORE selects): every byte of obs and mask written, nothing outside them, ordered
inside a launch, and visible to every kind of reader that follows a step."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as O
from test_env_gpu import _vec

pytestmark = pytest.mark.gpu

_NAN_BITS = 0x7FC5A5A5  # a quiet NaN no kernel writes (obs is 0.0 / 1.0)
_MASK_FILL = 0xA5       # not a bool byte
_OBS_GUARD = 2048       # floats (8 KiB: more than one plane of every board below)
_MASK_GUARD = 4096      # bytes


class _Guarded:
    """obs [N,10,H,W] f32 and mask [N,A] bool as views into larger device buffers, with a
    guard zone on both sides; fill() before a launch, check() after it."""

    def __init__(self, N, H, W, obs_shift=0):
        self.n_obs, self.n_mask = N * 10 * H * W, N * H * W
        self.obs_buf = torch.empty(2 * _OBS_GUARD + self.n_obs + obs_shift, dtype=torch.float32, device="cuda")
        self.mask_buf = torch.empty(2 * _MASK_GUARD + self.n_mask, dtype=torch.uint8, device="cuda")
        self.o0 = _OBS_GUARD + obs_shift
        self.obs = self.obs_buf[self.o0:self.o0 + self.n_obs].view(N, 10, H, W)
        self.mask = self.mask_buf[_MASK_GUARD:_MASK_GUARD + self.n_mask].view(torch.bool).view(N, H * W)

    def fill(self):
        self.obs_buf.view(torch.int32).fill_(_NAN_BITS)
        self.mask_buf.fill_(_MASK_FILL)

    def check(self, ref_obs, ref_mask, what):
        ob = self.obs_buf.cpu().numpy().view(np.int32)
        mb = self.mask_buf.cpu().numpy()
        lo, hi = self.o0, self.o0 + self.n_obs
        assert (ob[:lo] == _NAN_BITS).all() and (ob[hi:] == _NAN_BITS).all(), f"obs guard touched: {what}"
        assert (mb[:_MASK_GUARD] == _MASK_FILL).all() and (mb[_MASK_GUARD + self.n_mask:] == _MASK_FILL).all(), \
            f"mask guard touched: {what}"
        inner, minner = ob[lo:hi], mb[_MASK_GUARD:_MASK_GUARD + self.n_mask]
        assert not (inner == _NAN_BITS).any(), f"obs bytes left unwritten: {what}"
        assert not (minner == _MASK_FILL).any(), f"mask bytes left unwritten: {what}"
        assert np.array_equal(inner, np.ascontiguousarray(ref_obs).view(np.int32).ravel()), f"obs: {what}"
        assert np.array_equal(minner, ref_mask.astype(np.uint8).ravel()), f"mask: {what}"


def _out(g, N):
    return dict(obs=g.obs, action_mask=g.mask, rewards=torch.empty(N, device="cuda"),
                dones=torch.empty(N, dtype=torch.bool, device="cuda"))


# (H, W, K, N, debug flag): the emit paths at the smallest sizes that leave a partial last
# workgroup or wave
_EMIT_CASES = [
    (16, 16, 40, 5, None),                            # k_step, partial workgroup of 4
    (16, 16, 40, 203, "MS_DBG_FORCE_PACKED"),         # pk_emit16, partial wave
    (9, 9, 10, 33, None),                             # packed byte image, partial wave
    (9, 9, 10, 6, "MS_DBG_ONE_BOARD_PER_WAVE"),       # scalar stores, A % 4 != 0
    (30, 16, 99, 3, None),
    (5, 7, 8, 4, None),                               # generic template
]


@pytest.mark.parametrize("H,W,K,N,flag", _EMIT_CASES)
@pytest.mark.parametrize("mode", [0, 1])
def test_every_byte_written_once_and_only_inside(gpu, H, W, K, N, flag, mode):
    """Each of 12 tape steps writes all of obs and mask (no sentinel left), nothing outside
    them (guards intact), and the oracle's bytes."""
    from ms_amd import _lib as L
    v = _vec(H, W, K, N, seed=5)
    if flag:
        v.set_debug_flags(getattr(L, flag))
    o = O.OracleVec(H, W, K, N, seed=5)
    v.reset()
    o.reset()
    g = _Guarded(N, H, W)
    out = _out(g, N)
    for t in range(12):
        a = v.tape_actions(t, mode)
        g.fill()
        v.step(a, out=out)
        ref = o.step(a.cpu().numpy())
        g.check(ref["obs"], ref["mask"], f"step {t}")
        assert np.array_equal(out["rewards"].cpu().numpy(), ref["reward"]), t


def test_misaligned_obs_base_16x16(gpu):
    """A 16x16 obs base that is 4-B but not 16-B aligned (a view one float into its buffer)
    gives the obs of an aligned twin env, and stays inside its view."""
    N = 40
    a, b = _vec(16, 16, 40, N, seed=3), _vec(16, 16, 40, N, seed=3)
    a.reset()
    b.reset()
    g = _Guarded(N, 16, 16, obs_shift=1)
    assert g.obs.data_ptr() % 16 == 4
    out = _out(g, N)
    for t in range(10):
        act = a.tape_actions(t, 1)
        g.fill()
        a.step(act, out=out)
        bb, rb, db, _ = b.step(act)
        g.check(bb["obs"].cpu().numpy(), bb["action_mask"].cpu().numpy(), f"step {t}")
        assert torch.equal(out["rewards"], rb) and torch.equal(out["dones"], db), t


@pytest.mark.parametrize("H,W,K,N", [(16, 16, 40, 130), (9, 9, 10, 203)])
@pytest.mark.parametrize("mode", [0, 1])
def test_run_tape_overwrite_keeps_last_step(gpu, H, W, K, N, mode):
    """ms_run_tape with slots = 0 writes 7 steps into one obs buffer in one launch; what stays
    is the last step's (same-address stores of one launch land in program order)."""
    T = 7
    a, b = _vec(H, W, K, N, seed=17), _vec(H, W, K, N, seed=17)
    a.reset()
    b.reset()
    for t in range(T):
        act = a.tape_actions(2 + t, mode)
        batch, r, d, _ = a.step(act)
    last = b.run_tape(2, T, mode, slots=False)
    assert torch.equal(last["obs"], batch["obs"])
    assert torch.equal(last["action_mask"], batch["action_mask"])
    assert torch.equal(last["actions"], act) and torch.equal(last["rewards"], r) and torch.equal(last["dones"], d)


def test_consumers_see_the_obs(gpu):
    """After step on stream s: a reduction on s, one on a second stream behind an event of s,
    and a host copy all see the oracle's obs; and a captured graph of 3 (tape, step) pairs
    into distinct slots replays to what a twin env computes eagerly."""
    H, W, K, N = 16, 16, 40, 130
    v = _vec(H, W, K, N, seed=11)
    o = O.OracleVec(H, W, K, N, seed=11)
    v.reset()
    o.reset()
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for t in range(3):
        with torch.cuda.stream(s):
            a = v.tape_actions(t, 1)
            batch, _, _, _ = v.step(a)
            obs = batch["obs"]
            red = obs.sum(dim=(2, 3))
            ev = torch.cuda.Event()
            ev.record(s)
        s2.wait_event(ev)
        with torch.cuda.stream(s2):
            red2 = obs.sum(dim=(2, 3))
        with torch.cuda.stream(s):
            host = obs.cpu().numpy()
        s2.synchronize()
        s.synchronize()
        ref = o.step(a.cpu().numpy())["obs"]
        want = ref.sum(axis=(2, 3))  # counts of 0/1 cells: exact in f32
        assert np.array_equal(host, ref), t
        assert np.array_equal(red.cpu().numpy(), want), t
        assert np.array_equal(red2.cpu().numpy(), want), t

    a_env, b_env = _vec(H, W, K, N, seed=23), _vec(H, W, K, N, seed=23)
    a_env.reset()
    b_env.reset()
    acts = torch.empty(3, N, dtype=torch.int64, device="cuda")
    outs = [dict(obs=torch.zeros(N, 10, H, W, device="cuda"),
                 action_mask=torch.zeros(N, H * W, dtype=torch.bool, device="cuda"),
                 rewards=torch.zeros(N, device="cuda"), dones=torch.zeros(N, dtype=torch.bool, device="cuda"))
            for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(3):
            a_env.tape_actions(i, 1, out=acts[i])
            a_env.step(acts[i], out=outs[i])
    graph.replay()
    torch.cuda.synchronize()
    for i in range(3):
        act = b_env.tape_actions(i, 1)
        bb, rb, db, _ = b_env.step(act)
        assert torch.equal(acts[i], act), i
        assert torch.equal(outs[i]["obs"], bb["obs"]), i
        assert torch.equal(outs[i]["action_mask"], bb["action_mask"]), i
        assert torch.equal(outs[i]["rewards"], rb) and torch.equal(outs[i]["dones"], db), i


@pytest.mark.parametrize("H,W,K,N", [(16, 16, 40, 5), (9, 9, 10, 6), (9, 9, 10, 3)])
def test_reset_obs(gpu, H, W, K, N):
    """reset writes the oracle's reset obs and mask (float4 form, and the scalar form when
    the float count is no multiple of 4: 9x9 N=3), every byte and only inside."""
    v = _vec(H, W, K, N, seed=2)
    o = O.OracleVec(H, W, K, N, seed=2)
    g = _Guarded(N, H, W)
    g.fill()
    v.reset(out=dict(obs=g.obs, action_mask=g.mask))
    ref_obs, ref_mask = o.reset()
    g.check(ref_obs, ref_mask, "reset")
