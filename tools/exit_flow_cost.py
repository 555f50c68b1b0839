"""What the exit flow costs the C2 step (12x12, 32 agents, 65,536 envs, Neumann) when it is on, next to
the field statistics' observer measured in the same run, and what the host route it replaces costs.

    python tools/exit_flow_cost.py [--envs 65536] [--steps 496] [--rounds 5] [--host-steps 24]
                                   [--variants NAME,NAME,...]

One engine, burnt in for 1,000 steps; then, round by round (interleaved), the features are set to
each variant in turn and `--steps` steps of one step(n) call are timed:
  off             both features off (bench.py's workload)
  flow            the exit flow: one class, one door, curve_bins = 128   (the default form and grid)
  flow5           five classes (e % 5), 128 bins
  global          `flow` with FFM_EXIT_FLOW_FORM=global
  bN              `flow` with FFM_EXIT_FLOW_BLOCKS = N
  fields          the field statistics alone: five classes, 128 bins (tools/field_stats_cost.py's 5c+128)
  both            `flow5` and `fields` together
  host            the route the flow replaces: get_state() before and after every step(1) and the set
                  rule in NumPy, `--host-steps` steps per round
One line per run: variant, round, us per step.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (flow classes or 0, field-statistics classes or 0, switches)
VARIANTS = {
    "off": (0, 0, {}),
    "flow": (1, 0, {}),
    "flow5": (5, 0, {}),
    "global": (1, 0, {"FFM_EXIT_FLOW_FORM": "global"}),
    "b256": (1, 0, {"FFM_EXIT_FLOW_BLOCKS": "256"}),
    "b512": (1, 0, {"FFM_EXIT_FLOW_BLOCKS": "512"}),
    "b1024": (1, 0, {"FFM_EXIT_FLOW_BLOCKS": "1024"}),
    "b4096": (1, 0, {"FFM_EXIT_FLOW_BLOCKS": "4096"}),
    "fields": (0, 5, {}),
    "both": (5, 5, {}),
    "host": (0, 0, {}),
}
SWITCHES = ("FFM_EXIT_FLOW_FORM", "FFM_EXIT_FLOW_BLOCKS")
BINS = 128


def host_flow(door_from, before, after, exited):
    """The set rule on the host: exited[door] += 1 for every agent of `before` whose cell has a door
    and is not among `after` (an env that was re-placed or emptied: every agent)."""
    (p0, c0, k0), (p1, c1, k1) = before, after
    A = p0.shape[1]
    live0 = np.arange(A)[None, :] < c0[:, None]
    live1 = np.arange(A)[None, :] < c1[:, None]
    door = np.where(live0, door_from[np.minimum(p0, door_from.size - 1)], -1)
    occ = np.zeros((p0.shape[0], door_from.size), bool)
    e, j = np.nonzero(live1)
    occ[e, p1[e, j]] = True
    emptied = (k1 != k0) | (c1 == 0)
    stayed = np.take_along_axis(occ, np.minimum(p0, door_from.size - 1).astype(np.int64), axis=1) & ~emptied[:, None]
    left = (door >= 0) & ~stayed
    exited += np.bincount(door[left], minlength=exited.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=496)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=24)
    ap.add_argument("--variants", default="off,flow,flow5,global,fields,both,host")
    a = ap.parse_args()
    import torch
    from ffm_amd.data import l1_sff, make_room
    from ffm_amd.engine import Engine, _DevArray
    m = make_room(12, 12)
    s = l1_sff(m)
    p = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}
    E = a.envs
    names = [n for n in a.variants.split(",") if n]
    # one engine for every variant, as tools/field_stats_cost.py: a difference between two lines is the feature's
    eng = Engine(m, s, n_envs=E, n_agents=32, params=p, rng="philox", seed=42, auto_reset=True)
    eng.reset()
    eng.step(1000)
    cls5 = np.arange(E) % 5
    door_from = np.full(144, -1, np.int64)
    door_from[1 * 12 + 6] = 0                  # the cell below the exit at (0, 6): the one Neumann neighbour
    eps = torch.as_tensor(_DevArray(eng.device_buffers()["episodes"], E, "<i4"), device=f"cuda:{eng.device}")

    def configure(name):
        xf, fs, sw = VARIANTS[name]
        for k in SWITCHES:                  # read when the feature is set
            os.environ.pop(k, None)
        os.environ.update(sw)
        eng.set_exit_flow(classes=cls5 % xf if xf > 1 else None, n_classes=xf, curve_bins=BINS)
        eng.set_field_stats(cls5 % fs if fs > 1 else None, fs, BINS)
        for k in SWITCHES:
            os.environ.pop(k, None)

    for name in names:
        configure(name)
        li = eng.launch_info()
        print(f"# {name}: exit_flow {li['exit_flow']} field_stats {li['field_stats']}", flush=True)
    for r in range(1, a.rounds + 1):
        for name in names:
            configure(name)
            eng.step(16)                    # the region starts with the variant's kernels loaded
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "host":
                exited = np.zeros(1, np.int64)
                pos, cnt, _ = eng.get_state()
                before = (pos, cnt, eps.cpu().numpy())
                for _ in range(a.host_steps):
                    eng.step(1)
                    pos, cnt, _ = eng.get_state()
                    after = (pos, cnt, eps.cpu().numpy())
                    host_flow(door_from, before, after, exited)
                    before = after
                done = a.host_steps
            else:
                eng.step(a.steps)
                done = a.steps
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{name} round{r} {dt / done * 1e6:.2f} us_per_step", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
