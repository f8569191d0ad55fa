"""A plain ``bench.py`` run (no ``--full``): it times exactly ``--steps`` steps, prints one JSON
line holding only the headline figure, and ``--dump-outputs`` writes what the last timed step
returned. The dumped arrays are checked against the CPU oracle stepped through the same tape
indices, so they are the same from run to run and from build to build.

One process, small sizes: 64 envs, 1003 steps = the 500-step graph replayed twice plus a
3-step graph (every replay path of the timed region).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, STEPS, WARMUP, GRAPH_STEPS = 64, 1003, 2, 500


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    import oracle as O
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", str(N), "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["timed_steps"] == STEPS and line["warmup"] == WARMUP
    assert line["unit"] == "env_steps/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for moved in ("roofline", "multistep", "north_star_points", "ppo", "cpu_baseline"):
        assert moved not in line, moved

    # the tape indices bench.py ran: warm-up 0..W-1, each of the two graphs once untimed, then
    # timed the 500-step graph twice and the 3-step graph
    import bench
    assert bench.GRAPH_STEPS == GRAPH_STEPS
    reps, rem = divmod(STEPS, GRAPH_STEPS)
    g_chunk, g_rem = list(range(WARMUP, WARMUP + GRAPH_STEPS)), list(range(WARMUP, WARMUP + rem))
    ts = list(range(WARMUP)) + g_chunk + g_rem + g_chunk * reps + g_rem
    ref = O.OracleVec(16, 16, 40, N, seed=0)
    ref.reset()
    for t in ts[:-1]:
        ref.step(ref.tape(t), want_obs=False)
    a = ref.tape(ts[-1])
    o = ref.step(a)
    want = {"action": a, "obs": o["obs"], "action_mask": o["mask"], "reward": o["reward"], "done": o["done"],
            "step": o["step"], "last_new": o["last_new"], "frac": o["frac"], "outcome": o["outcome"]}
    got = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert set(got) == set(want)
    assert sum(v.nbytes for v in got.values()) <= 64e6
    for k, w in want.items():
        assert got[k].dtype == (np.float64 if w.dtype == np.float64 else np.float32), k
        assert got[k].shape == w.shape, k
        assert np.array_equal(got[k], w.astype(got[k].dtype)), k
