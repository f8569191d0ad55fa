"""Host restatement of the masked sampler's random stream (csrc/msrollout.hip uniform01 and
k_sample, csrc/msenv_pcg.h splitmix64) with numpy uint64: the Gumbel keys l - log(-log u) in f64."""
from __future__ import annotations

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    with np.errstate(over="ignore"):
        z = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(seed, counter, rows, cols):
    """u(seed, counter, row, col) in (0, 1) from 24 hash bits, f64 [len(rows), len(cols)]."""
    with np.errstate(over="ignore"):
        rc = np.asarray(rows, dtype=np.uint64)[:, None] * np.uint64(0x100000001B3) + \
            np.asarray(cols, dtype=np.uint64)[None, :]
        h = splitmix64(np.uint64(seed) ^ splitmix64(np.uint64(counter) ^ splitmix64(rc)))
    return ((h >> np.uint64(40)).astype(np.float64) + 0.5) / 16777216.0


def gumbel_keys(logits, mask, seed, counter, row_begin=0):
    """f64 [N, A] keys of k_sample: logit - log(-log u) at legal cells, -inf elsewhere; a row with
    no legal cell counts as all legal."""
    lg = np.asarray(logits, dtype=np.float64)
    m = np.asarray(mask, dtype=bool).copy()
    m[~m.any(1)] = True
    n, a = lg.shape
    u = uniform01(seed, counter, np.arange(row_begin, row_begin + n), np.arange(a))
    return np.where(m, lg - np.log(-np.log(u)), -np.inf)


def sampler_case(N=64, A=81, seed=21):
    """The fixed logits / mask of the arg-max test (built on the CPU, so the CPU test counts the
    same near-tie rows that the GPU test leaves out)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(N, A, generator=g) * 3
    mask = torch.rand(N, A, generator=g) < 0.5
    return logits, mask


def near_tie_rows(keys, gap=1e-3):
    """Rows whose runner-up key is within ``gap`` of the maximum."""
    s = np.sort(keys, axis=1)
    return (s[:, -1] - s[:, -2]) <= gap
