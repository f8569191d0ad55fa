"""ms_dagger_act on the device (include/msdagger.h, csrc/msdagger.hip) against the numpy restatement
tests/dagger_ref.py. Every comparison is exact. The uniform action and mode 1's learner action are
Gumbel-max draws whose logf numpy does not reproduce bit for bit: the reference takes them from
ms_sample_masked on the device, which the kernel must equal cell for cell.

Rows 1, 3, 5, 130: a partial last workgroup (four rows each) and more than one workgroup. Cells
1, 63, 64, 65, 81, 256, 480, 3968: one cell, the lane-count boundaries, 1 to 8 cells per lane and
the bound (62 per lane)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import dagger_ref as R

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 5, 130)
CELLS = (1, 63, 64, 65, 81, 256, 480, 3968)
SEED, COUNTER = 0x1234567890ABCDEF, 11
OUT = ("action", "source", "learner_action", "agree")


def _case(n, A, seed=0):
    """Logits with ties, a few +-inf and no NaN (k_sample, the reference of mode 1, has no defined
    answer for a row of NaN keys; the edge-row test covers NaN); a half-legal mask with one row of
    no legal cell and one of a single legal cell; random teacher targets."""
    g = torch.Generator(device="cpu").manual_seed(1000 * A + n + seed)
    logits = (torch.randn(n, A, generator=g) * 3).round()  # whole numbers: many equal maxima
    r = torch.rand(n, A, generator=g)
    logits[r < 0.03] = float("-inf")
    logits[r > 0.98] = float("inf")
    mask = torch.rand(n, A, generator=g) < 0.5
    mask[n // 2] = False
    if n > 2:
        mask[n - 1] = False
        mask[n - 1, A // 3] = True
    kind = torch.randint(0, 3, (n,), generator=g, dtype=torch.uint8)
    best = (torch.rand(n, A, generator=g) < 0.3).to(torch.uint8)
    action = torch.where(kind != 0, torch.randint(0, A, (n,), generator=g), torch.full((n,), -1))
    return logits, mask, {"best": best, "action": action, "kind": kind}


def _dev(gpu, logits, mask, tg):
    return logits.to(gpu), mask.to(gpu), {k: v.to(gpu) for k, v in tg.items()}


def _draws(logits, mask, row_begin):
    """(u, sampled l) as numpy: ms_sample_masked on zeros with the seed, and on the logits with the
    learner's stream seed."""
    from ms_amd.rollout import sample_masked
    u, _ = sample_masked(torch.zeros_like(logits), mask, SEED, COUNTER, row_begin=row_begin)
    s, _ = sample_masked(logits, mask, R.stream_seed(SEED, R.C_LEARNER), COUNTER, row_begin=row_begin)
    return u.cpu().numpy(), R.sampled(s.cpu().numpy(), mask.cpu().numpy())


def _check_legal(actions, mask_np, A):
    a = np.asarray(actions)
    assert ((a >= 0) & (a < A)).all()
    assert R.legal(mask_np)[np.arange(len(a)), a].all()


@pytest.mark.parametrize("A", CELLS)
def test_matches_the_reference(gpu, A):
    from ms_amd.dagger import dagger_act
    seen = set()
    for n in ROWS:
        logits, mask, tg = _case(n, A)
        lg_np, m_np = logits.numpy(), mask.numpy()
        tg_np = {k: v.numpy() for k, v in tg.items()}
        dl, dm, dt = _dev(gpu, logits, mask, tg)
        for row_begin in (0, 7):
            u, ls = _draws(dl, dm, row_begin)
            _check_legal(u, m_np, A)
            learner = {"greedy": R.greedy(lg_np, m_np), "sample": ls}
            for mode in ("greedy", "sample"):
                _check_legal(learner[mode], m_np, A)
                for beta in (0.0, 0.3, 1.0):
                    for explore in (0.0, 0.4, 1.0):
                        got = dagger_act(dl, dm, dt, seed=SEED, counter=COUNTER, beta=beta, explore=explore,
                                         mode=mode, row_begin=row_begin)
                        want = R.act(u, learner[mode], tg_np["action"], tg_np["kind"], tg_np["best"], seed=SEED,
                                     counter=COUNTER, beta=beta, explore=explore, row_begin=row_begin)
                        for k in OUT:
                            w = torch.from_numpy(want[k])
                            assert got[k].dtype == w.dtype and torch.equal(got[k].cpu(), w), \
                                (k, n, A, row_begin, mode, beta, explore)
                        seen |= set(want["source"].tolist())
    assert seen == {0, 1, 2}


def test_a_shard_equals_its_rows_of_the_whole_call(gpu):
    from ms_amd.dagger import dagger_act
    n, A, a, b = 130, 81, 37, 102
    dl, dm, dt = _dev(gpu, *_case(n, A))
    for mode in ("greedy", "sample"):
        kw = dict(seed=SEED, counter=COUNTER, beta=0.3, explore=0.4, mode=mode)
        whole = dagger_act(dl, dm, dt, row_begin=5, **kw)
        part = dagger_act(dl[a:b], dm[a:b], {k: v[a:b] for k, v in dt.items()}, row_begin=5 + a, **kw)
        for k in OUT:
            assert torch.equal(part[k], whole[k][a:b]), (k, mode)
        assert len(set(whole["source"].tolist())) == 3
        other = dagger_act(dl[a:b], dm[a:b], {k: v[a:b] for k, v in dt.items()}, row_begin=0, **kw)
        assert not torch.equal(other["source"], part["source"])  # the coins are keyed by the global row


def test_greedy_edge_rows_and_legal_actions_in_both_modes(gpu):
    from ms_amd.dagger import dagger_act
    A = 130  # three cells on lanes 0 and 1, two on the others
    inf, nan = float("inf"), float("nan")
    base = torch.linspace(-2.0, 2.0, A)
    rows, masks, want = [], [], []

    def add(lg, m, w):
        rows.append(lg)
        masks.append(m)
        want.append(w)

    ones = torch.ones(A, dtype=torch.bool)
    lg = base.clone()
    lg[[5, 70, 100]] = 7.0
    add(lg, ones, 5)  # duplicated maxima across lanes and slices: the lowest index
    lg = base.clone()
    lg[[69, 5]] = 7.0
    m = ones.clone()
    m[5] = False
    add(lg, m, 69)  # the lower of the two maxima is masked
    lg = base.clone()
    lg[64] = 50.0
    m = ones.clone()
    m[64] = False
    add(lg, m, A - 1)  # the maximum at a masked cell is ignored
    lg = base.clone()
    lg[77] = 9.0
    add(lg, torch.zeros(A, dtype=torch.bool), 77)  # no legal cell: all legal
    m = torch.zeros(A, dtype=torch.bool)
    m[[66, 3, 129]] = True
    add(torch.full((A,), -inf), m, 3)  # every legal logit -inf: the lowest legal cell
    lg = base.clone()
    lg[A - 1] = nan
    add(lg, ones, A - 2)  # NaN where the arg-max would be
    lg = base.clone()
    m = torch.zeros(A, dtype=torch.bool)
    m[[70, 8, 100]] = True
    lg[[70, 8, 100]] = nan
    add(lg, m, 8)  # every legal logit NaN (the others are masked): the lowest legal cell
    add(torch.full((A,), nan), torch.zeros(A, dtype=torch.bool), 0)  # all NaN, nothing legal
    lg = torch.full((A,), nan)
    lg[[4, 90]] = -inf
    m = ones.clone()
    m[0] = False
    add(lg, m, 1)  # NaN and -inf only: no logit above -inf, so the lowest legal cell
    lg = base.clone()
    lg[[3, 67]] = inf
    add(lg, ones, 3)  # +inf twice
    logits, mask = torch.stack(rows), torch.stack(masks)
    n = logits.shape[0]
    assert R.greedy(logits.numpy(), mask.numpy()).tolist() == want  # the reference agrees with the list
    kind = torch.ones(n, dtype=torch.uint8)
    best = torch.zeros((n, A), dtype=torch.uint8)
    best[torch.arange(n), torch.tensor(want)] = 1
    best[0] = 0
    tg = {"best": best, "action": torch.tensor(want), "kind": kind}  # a legal move for the teacher, too
    dl, dm, dt = _dev(gpu, logits, mask, tg)
    got = dagger_act(dl, dm, dt, seed=SEED, counter=COUNTER, beta=0.0, explore=0.0, mode="greedy")
    assert got["action"].tolist() == want and got["learner_action"].tolist() == want
    assert got["source"].tolist() == [2] * n and got["agree"].tolist() == [0] + [1] * (n - 1)
    for c in range(8):
        s = dagger_act(dl, dm, dt, seed=SEED, counter=c, beta=0.0, explore=0.0, mode="sample")
        _check_legal(s["action"].cpu().numpy(), mask.numpy(), A)
        assert torch.equal(s["action"], s["learner_action"])
        # where only one answer is possible: the rows whose legal keys are all NaN, and +inf's lowest
        assert s["action"][6].item() == 8 and s["action"][7].item() == 0 and s["action"][9].item() == 3
        assert s["action"][8].item() in (4, 90)  # the two -inf cells tie at -inf; NaN keys never lead
        assert s["action"][4].item() == 3  # keys all -inf: the lowest legal cell, as in k_sample
        half = dagger_act(dl, dm, dt, seed=SEED, counter=c, beta=0.5, explore=0.5, mode="sample")
        _check_legal(half["action"].cpu().numpy(), mask.numpy(), A)
        _check_legal(half["learner_action"].cpu().numpy(), mask.numpy(), A)


def test_beta_one_reads_no_logits(gpu):
    from ms_amd.dagger import dagger_act
    from ms_amd.rollout import sample_masked
    n, A = 130, 81
    dl, dm, dt = _dev(gpu, *_case(n, A))
    got = dagger_act(None, dm, dt, seed=SEED, counter=COUNTER, beta=1.0, explore=0.0, row_begin=7)
    u, _ = sample_masked(torch.zeros_like(dl), dm, SEED, COUNTER, row_begin=7)
    assert torch.equal(got["action"], torch.where(dt["kind"] != 0, dt["action"], u))
    assert torch.equal(got["source"], (dt["kind"] != 0).to(torch.uint8))
    assert (got["learner_action"] == -1).all() and not got["agree"].any()
    # with logits the same moves are played; the learner's move and the agreement are reported
    wl = dagger_act(dl, dm, dt, seed=SEED, counter=COUNTER, beta=1.0, explore=0.0, row_begin=7)
    assert torch.equal(wl["action"], got["action"]) and torch.equal(wl["source"], got["source"])
    assert (wl["learner_action"] >= 0).all() and wl["agree"].any()
    # explore alone, still without logits
    ex = dagger_act(None, dm, dt, seed=SEED, counter=COUNTER, beta=1.0, explore=1.0, row_begin=7)
    assert torch.equal(ex["action"], u) and not ex["source"].any()


def _raw(lib, L, dl, dm, dt, n, A, beta, explore, mode, outs):
    return lib.ms_dagger_act(L.ptr(dl), L.ptr(dm.view(torch.uint8)), L.ptr(dt["best"]), L.ptr(dt["action"]),
                             L.ptr(dt["kind"]), n, A, 0, SEED, COUNTER, beta, explore, mode,
                             *(L.ptr(o) for o in outs), L.stream_ptr(dm.device))


def test_null_outputs_and_refused_calls(gpu):
    from ms_amd import _lib as L
    from ms_amd.dagger import dagger_act
    lib = L.load()
    n, A = 5, 65
    dl, dm, dt = _dev(gpu, *_case(n, A))
    full = dagger_act(dl, dm, dt, seed=SEED, counter=COUNTER, beta=0.3, explore=0.4, mode="sample")

    def fresh():
        return [torch.full((n,), -7, dtype=torch.int64, device=gpu), torch.full((n,), 249, dtype=torch.uint8, device=gpu),
                torch.full((n,), -7, dtype=torch.int64, device=gpu), torch.full((n,), 249, dtype=torch.uint8, device=gpu)]

    for keep in ((0,), (0, 1), (0, 2), (0, 3), (0, 1, 2, 3)):
        outs = fresh()
        passed = [o if i in keep else None for i, o in enumerate(outs)]
        assert _raw(lib, L, dl, dm, dt, n, A, 0.3, 0.4, 1, passed) == 0
        for i, k in enumerate(OUT):
            if i in keep:
                assert torch.equal(outs[i], full[k]), (keep, k)
    # each refused call returns MS_EINVAL and launches nothing: the outputs keep their fill
    outs = fresh()
    for beta, explore, mode, lg, cells in ((1.5, 0.0, 0, dl, A), (float("nan"), 0.0, 0, dl, A), (0.5, 0.0, 2, dl, A),
                                           (0.5, 0.0, 0, None, A), (0.5, 0.0, 0, dl, 0), (0.5, float("nan"), 0, dl, A)):
        assert _raw(lib, L, lg, dm, dt, n, cells, beta, explore, mode, outs) == 1
        assert b"ms_dagger_act" in lib.ms_last_error()
    torch.cuda.synchronize()
    for o, fill in zip(outs, (-7, 249, -7, 249)):
        assert (o == fill).all()
    with pytest.raises(L.MsEnvError, match="3968"):  # the wrapper raises what the library reports
        L.check(_raw(lib, L, dl, dm, dt, n, 3969, 0.5, 0.0, 0, outs))


def test_two_calls_are_bitwise_equal(gpu):
    from ms_amd.dagger import dagger_act
    dl, dm, dt = _dev(gpu, *_case(130, 256))
    for mode in ("greedy", "sample"):
        kw = dict(seed=SEED, counter=COUNTER, beta=0.3, explore=0.4, mode=mode, row_begin=3)
        a, b = dagger_act(dl, dm, dt, **kw), dagger_act(dl, dm, dt, **kw)
        for k in OUT:
            assert torch.equal(a[k], b[k]), (k, mode)
        c = dagger_act(dl, dm, dt, **dict(kw, counter=COUNTER + 1))
        assert not torch.equal(a["source"], c["source"])
