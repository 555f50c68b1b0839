"""What the motion statistics cost the C2 step (12x12, 32 agents, 65,536 envs, Neumann) when they are
on, next to the exit flow measured in the same run: the flow kernel reads the same two position
rows and writes one, the motion kernel adds the origin row (read and written) and one more table.

    python tools/motion_stats_cost.py [--envs 65536] [--steps 496] [--rounds 5] [--variants NAME,NAME,...]

One engine, burnt in for 1,000 steps; then, round by round (interleaved), the features are set to
each variant in turn and `--steps` steps of one step(n) call are timed:
  off             both features off (bench.py's workload)
  motion          the motion statistics: one class, curve_bins = 128   (the default form and grid)
  motion5         five classes (e % 5), 128 bins
  global          `motion` with FFM_MOTION_STATS_FORM=global
  bN              `motion` with FFM_MOTION_STATS_BLOCKS = N
  flow            the exit flow alone: one class, one door, 128 bins (tools/exit_flow_cost.py's flow)
  both            `motion` and `flow` together (the motion kernel first, the flow kernel carries the snapshot)
One line per run: variant, round, us per step; then the medians and motion's cost over flow's.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (motion classes or 0, flow classes or 0, switches)
VARIANTS = {
    "off": (0, 0, {}),
    "motion": (1, 0, {}),
    "motion5": (5, 0, {}),
    "global": (1, 0, {"FFM_MOTION_STATS_FORM": "global"}),
    "b256": (1, 0, {"FFM_MOTION_STATS_BLOCKS": "256"}),
    "b4096": (1, 0, {"FFM_MOTION_STATS_BLOCKS": "4096"}),
    "flow": (0, 1, {}),
    "both": (1, 1, {}),
}
SWITCHES = ("FFM_MOTION_STATS_FORM", "FFM_MOTION_STATS_BLOCKS")
BINS = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=496)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="off,motion,flow,both,motion5,global")
    a = ap.parse_args()
    import torch
    from ffm_amd.data import l1_sff, make_room
    from ffm_amd.engine import Engine
    m = make_room(12, 12)
    s = l1_sff(m)
    p = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}
    E = a.envs
    names = [n for n in a.variants.split(",") if n]
    # one engine for every variant, as tools/exit_flow_cost.py: a difference between two lines is the feature's
    eng = Engine(m, s, n_envs=E, n_agents=32, params=p, rng="philox", seed=42, auto_reset=True)
    eng.reset()
    eng.step(1000)
    cls5 = np.arange(E) % 5

    def configure(name):
        mo, xf, sw = VARIANTS[name]
        for k in SWITCHES:                  # read when the feature is set
            os.environ.pop(k, None)
        os.environ.update(sw)
        eng.set_motion_stats(classes=cls5 % mo if mo > 1 else None, n_classes=mo, curve_bins=BINS)
        eng.set_exit_flow(classes=cls5 % xf if xf > 1 else None, n_classes=xf, curve_bins=BINS)
        for k in SWITCHES:
            os.environ.pop(k, None)

    for name in names:
        configure(name)
        print(f"# {name}: motion_stats {eng.motion_stats_info()} exit_flow {eng.launch_info()['exit_flow']}", flush=True)
    runs = {name: [] for name in names}
    for r in range(1, a.rounds + 1):
        for name in names:
            configure(name)
            eng.step(16)                    # the region starts with the variant's kernels loaded
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.step(a.steps)
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / a.steps * 1e6
            runs[name].append(us)
            print(f"{name} round{r} {us:.2f} us_per_step", flush=True)
    eng.close()
    med = {name: statistics.median(v) for name, v in runs.items()}
    for name in names:
        print(f"median {name} {med[name]:.2f} us_per_step (min {min(runs[name]):.2f}, max {max(runs[name]):.2f})")
    if all(k in med for k in ("off", "motion", "flow")) and med["flow"] > med["off"]:
        print(f"ratio (motion - off) / (flow - off) = {(med['motion'] - med['off']) / (med['flow'] - med['off']):.2f}")


if __name__ == "__main__":
    main()
