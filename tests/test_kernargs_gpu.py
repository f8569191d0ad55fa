"""Kernel-argument order of the env kernels (k_tape, k_step, k_step_packed, k_run, k_run_packed):
every value a launch site hands over must arrive in the parameter it was meant for. The tape is
checked against the pinned CPU oracle for every instantiation, both modes and env counts around
the wave size; the moved values (both halves of t, env_begin, the actions pointer) one by one;
the step kernels with optional outputs absent and the run kernels against a twin handle that
takes the full ms_tape_actions / ms_step calls (itself checked against the oracle)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

TAPE_BOARDS = [(16, 16, 40), (9, 9, 10), (30, 16, 99), (16, 30, 99), (7, 11, 12)]
# (H, W, K, n, packed16): a partial k_step workgroup of 4, a partial packed wave of 16 (9x9: four
# boards per wave, four waves), and 16x16 forced onto the packed kernels
STEP_CASES = [(16, 16, 40, 5, False), (9, 9, 10, 17, False), (16, 16, 40, 17, True)]
AUX_KEYS = ("step", "last_new_reveals", "revealed_frac", "outcome")


def _vec(H, W, K, N, seed=0, packed16=False, **kw):
    from ms_amd import EnvConfig, VecMinesweeper
    from ms_amd import _lib as L
    v = VecMinesweeper(N, EnvConfig(H=H, W=W, mine_count=K), seed=seed, **kw)
    if packed16:
        v.set_debug_flags(L.MS_DBG_FORCE_PACKED)
    return v


def _same_state(a, b):
    assert np.array_equal(a.rng_state(), b.rng_state())
    sa, sb = a.snapshot_tensors(), b.snapshot_tensors()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("H,W,K", TAPE_BOARDS)
@pytest.mark.parametrize("mode", [0, 1])
def test_tape_every_instantiation_vs_oracle(gpu, H, W, K, mode):
    """A lone env, a partial wave, an exact wave, one lane into the second workgroup, two full
    waves and two lanes; 8 steps, so fresh, first-click, part-revealed and reset boards occur."""
    for n in (1, 63, 64, 65, 130):
        v = _vec(H, W, K, n, seed=3)
        o = O.OracleVec(H, W, K, n, seed=3)
        v.reset()
        o.reset()
        for t in range(8):
            a = v.tape_actions(t, mode)
            a_np = a.cpu().numpy()
            assert np.array_equal(a_np, o.tape(t, mode)), (n, t)
            _, r, dn, _ = v.step(a)
            ref = o.step(a_np, want_obs=False)
            assert np.array_equal(r.cpu().numpy(), ref["reward"]), (n, t)
            assert np.array_equal(dn.cpu().numpy(), ref["done"]), (n, t)
        assert np.array_equal(v.rng_state(), o.rng_state()), n


@pytest.mark.parametrize("H,W,K", [(16, 16, 40), (7, 11, 12)])
@pytest.mark.parametrize("mode", [0, 1])
def test_tape_moved_values(gpu, H, W, K, mode):
    """Both halves of t, env_begin != 0 (shard 1 of 3 of 96 envs) and an actions pointer that is
    8-byte but not 16-byte aligned, on part-revealed boards."""
    total, rank, world = 96, 1, 3
    begin, n = total * rank // world, total // world
    v = _vec(H, W, K, total, seed=6, shard=(rank, world))
    assert v.env_begin == begin and v.num_envs == n
    o = O.OracleVec(H, W, K, total, seed=6, env_begin=begin, env_count=n)
    v.reset()
    o.reset()
    sentinel = -0x0123456789ABCDEF
    buf = torch.full((n + 1,), sentinel, dtype=torch.int64, device=v.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:]
    for t in (0, 1, 2**32 + 5, 2**63 + 1, 2**32 + 6, 2**63 + 2**32 + 9):
        a = v.tape_actions(t, mode, out=out)
        assert a.data_ptr() == buf.data_ptr() + 8
        a_np = a.cpu().numpy()
        assert np.array_equal(a_np, o.tape(t, mode)), t
        assert int(buf[0]) == sentinel, t
        v.step(a.clone())
        o.step(a_np, want_obs=False)
    # the two halves of t are told apart: neither half alone gives these actions
    hi = o.tape(2**32 + 5, mode)
    assert not np.array_equal(hi, o.tape(5, mode)) and not np.array_equal(hi, o.tape(2**32, mode))
    assert np.array_equal(v.tape_actions(2**32 + 5, mode).cpu().numpy(), hi)


def _step_outputs(v, n):
    dev = v.device
    return dict(rewards=torch.empty(n, dtype=torch.float32, device=dev), dones=torch.empty(n, dtype=torch.bool, device=dev),
                step=torch.empty(n, dtype=torch.int32, device=dev), last_new=torch.empty(n, dtype=torch.int32, device=dev),
                frac=torch.empty(n, dtype=torch.float64, device=dev), outcome=torch.empty(n, dtype=torch.int8, device=dev))


@pytest.mark.parametrize("H,W,K,n,packed16", STEP_CASES)
@pytest.mark.parametrize("form", ["no_obs_no_mask", "codes", "i32"])
def test_step_optional_outputs_absent(gpu, H, W, K, n, packed16, form):
    """ms_step with obs and mask null, ms_step_codes and ms_step_i32 report and leave behind
    what the full ms_step call does on a twin handle (which equals the oracle)."""
    from ms_amd import _lib as L
    from ms_amd.fused import obs_encode
    full, v = _vec(H, W, K, n, seed=8, packed16=packed16), _vec(H, W, K, n, seed=8, packed16=packed16)
    o = O.OracleVec(H, W, K, n, seed=8)
    full.reset()
    v.reset()
    o.reset()
    lib = L.load()
    for t in range(6):
        a = full.tape_actions(t, 1)
        assert torch.equal(v.tape_actions(t, 1), a), t
        batch, r, dn, info = full.step(a)
        ref = o.step(a.cpu().numpy())
        assert np.array_equal(batch["obs"].cpu().numpy(), ref["obs"]), t
        assert np.array_equal(r.cpu().numpy(), ref["reward"]), t
        want = dict(rewards=r, dones=dn, **{k: info.tensors[k] for k in AUX_KEYS})
        if form == "no_obs_no_mask":
            out = _step_outputs(v, n)
            with torch.cuda.device(v.device):
                L.check(lib.ms_step(v._h, L.ptr(a), None, None, L.ptr(out["rewards"]), L.ptr(out["dones"]),
                                    L.ptr(out["step"]), L.ptr(out["last_new"]), L.ptr(out["frac"]),
                                    L.ptr(out["outcome"]), v._stream()))
            v._version += 1
            got = dict(rewards=out["rewards"], dones=out["dones"], step=out["step"], last_new_reveals=out["last_new"],
                       revealed_frac=out["frac"], outcome=out["outcome"])
        elif form == "codes":
            bufs = dict(codes=torch.full((n, H * W), 255, dtype=torch.uint8, device=v.device),
                        action_mask=torch.empty((n, H * W), dtype=torch.bool, device=v.device),
                        rewards=torch.empty(n, dtype=torch.float32, device=v.device),
                        dones=torch.empty(n, dtype=torch.bool, device=v.device))
            b2, r2, d2, info2 = v.step(a, out=bufs)
            enc = torch.empty((n, H, W), dtype=torch.uint8, device=v.device)
            obs_encode(batch["obs"].contiguous(), enc)
            assert torch.equal(b2["codes"].reshape(n, H, W), enc), t
            assert torch.equal(b2["action_mask"], batch["action_mask"]), t
            got = dict(rewards=r2, dones=d2, **{k: info2.tensors[k] for k in AUX_KEYS})
        else:
            b2, r2, d2, info2 = v.step(a.to(torch.int32))
            assert torch.equal(b2["obs"], batch["obs"]) and torch.equal(b2["action_mask"], batch["action_mask"]), t
            got = dict(rewards=r2, dones=d2, **{k: info2.tensors[k] for k in AUX_KEYS})
        for k in want:
            assert torch.equal(got[k], want[k]), (k, t)
    _same_state(full, v)
    assert np.array_equal(full.rng_state(), o.rng_state())


@pytest.mark.parametrize("H,W,K,n,packed16", STEP_CASES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("slots", [False, True])
def test_run_tape_moved_values(gpu, H, W, K, n, packed16, mode, slots):
    """ms_run_tape with T = 3 and t0 = 2**32 + 7 equals three (tape_actions, step) pairs on a
    twin handle, the returned actions included; the twin's tape equals the oracle's."""
    T, t0 = 3, 2**32 + 7
    a, b = _vec(H, W, K, n, seed=12, packed16=packed16), _vec(H, W, K, n, seed=12, packed16=packed16)
    o = O.OracleVec(H, W, K, n, seed=12)
    for x in (a, b, o):
        x.reset()
    keys = type(a)._RUN_KEYS
    ref = {k: [] for k in keys}
    for t in range(T):
        act = a.tape_actions(t0 + t, mode)
        assert np.array_equal(act.cpu().numpy(), o.tape(t0 + t, mode)), t
        batch, r, d, info = a.step(act)
        oref = o.step(act.cpu().numpy())
        assert np.array_equal(batch["obs"].cpu().numpy(), oref["obs"]), t
        vals = dict(actions=act, obs=batch["obs"], action_mask=batch["action_mask"], rewards=r, dones=d,
                    **{k: info.tensors[k] for k in AUX_KEYS})
        for k in keys:
            ref[k].append(vals[k].clone())
    out = b.run_tape(t0, T, mode, slots=slots)
    for k in keys:
        want = torch.stack(ref[k]) if slots else ref[k][-1]
        assert torch.equal(out[k], want), k
    _same_state(a, b)
    assert np.array_equal(b.rng_state(), o.rng_state())
