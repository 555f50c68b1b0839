"""What the field statistics cost the C2 step (12x12, 32 agents, 65,536 envs, Neumann) when they are on,
and what the host route they replace costs.

    python tools/field_stats_cost.py [--envs 65536] [--steps 496] [--rounds 5] [--host-steps 48]
                                     [--variants NAME,NAME,...]

One engine, burnt in for 1,000 steps; then, round by round (interleaved), the feature is set to
each variant in turn and `--steps` steps of one step(n) call are timed:
  off             the feature off (bench.py's workload)
  1c              one class, no curve                    (the default form, slots and grid)
  5c+128          five classes (e % 5), curve_bins = 128
  lds / global    5c+128 with FFM_FIELD_STATS_FORM forced
  s1 s4 s64       5c+128, the LDS form with FFM_FIELD_STATS_SLOTS = 1, 4, 64   (default: kernels.h)
  rNbM            5c+128 with FFM_FIELD_STATS_RUN = N envs per run and FFM_FIELD_STATS_BLOCKS = M
                  (a shard of 32,768 envs is 32,768 / N runs)
  host            the route the feature replaces: step(1), get_state() and np.bincount of the cells
                  of the occupied envs per class, `--host-steps` steps per round
One line per run: variant, round, us per step.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (classes, bins, switches)
VARIANTS = {
    "off": None,
    "1c": (1, 0, {}),
    "5c+128": (5, 128, {}),
    "lds": (5, 128, {"FFM_FIELD_STATS_FORM": "lds"}),
    "global": (5, 128, {"FFM_FIELD_STATS_FORM": "global"}),
    "s1": (5, 128, {"FFM_FIELD_STATS_FORM": "lds", "FFM_FIELD_STATS_SLOTS": "1"}),
    "s4": (5, 128, {"FFM_FIELD_STATS_FORM": "lds", "FFM_FIELD_STATS_SLOTS": "4"}),
    "s64": (5, 128, {"FFM_FIELD_STATS_FORM": "lds", "FFM_FIELD_STATS_SLOTS": "64"}),
    "r1024b32": (5, 128, {"FFM_FIELD_STATS_RUN": "1024", "FFM_FIELD_STATS_BLOCKS": "32"}),
    "r512b64": (5, 128, {"FFM_FIELD_STATS_RUN": "512", "FFM_FIELD_STATS_BLOCKS": "64"}),
    "r256b128": (5, 128, {"FFM_FIELD_STATS_RUN": "256", "FFM_FIELD_STATS_BLOCKS": "128"}),
    "r128b256": (5, 128, {"FFM_FIELD_STATS_RUN": "128", "FFM_FIELD_STATS_BLOCKS": "256"}),
    "r64b256": (5, 128, {"FFM_FIELD_STATS_RUN": "64", "FFM_FIELD_STATS_BLOCKS": "256"}),
    "r64b512": (5, 128, {"FFM_FIELD_STATS_RUN": "64", "FFM_FIELD_STATS_BLOCKS": "512"}),
    "r32b512": (5, 128, {"FFM_FIELD_STATS_RUN": "32", "FFM_FIELD_STATS_BLOCKS": "512"}),
    "r32b1024": (5, 128, {"FFM_FIELD_STATS_RUN": "32", "FFM_FIELD_STATS_BLOCKS": "1024"}),
    "r16b2048": (5, 128, {"FFM_FIELD_STATS_RUN": "16", "FFM_FIELD_STATS_BLOCKS": "2048"}),
    "host": None,
}
SWITCHES = ("FFM_FIELD_STATS_FORM", "FFM_FIELD_STATS_SLOTS", "FFM_FIELD_STATS_BLOCKS", "FFM_FIELD_STATS_RUN")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=496)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=48)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    a = ap.parse_args()
    import torch
    from ffm_amd.data import l1_sff, make_room
    from ffm_amd.engine import Engine
    m = make_room(12, 12)
    s = l1_sff(m)
    p = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}
    E = a.envs
    names = [n for n in a.variants.split(",") if n]
    # One engine for every variant: the same buffers, the same shard streams and hardware queues,
    # so a difference between two lines is the feature's.  (With one engine per variant in one
    # process, every fourth engine created stepped 15 - 40 us slower whatever its variant was:
    # presumably its shard stream shares a hardware queue with the caller's stream.)
    eng = Engine(m, s, n_envs=E, n_agents=32, params=p, rng="philox", seed=42, auto_reset=True)
    eng.reset()
    eng.step(1000)
    cls5 = np.arange(E) % 5

    def configure(name):
        fs = VARIANTS[name]
        for k in SWITCHES:                  # read when the feature is set
            os.environ.pop(k, None)
        if not fs:
            eng.set_field_stats(n_classes=0)
            return
        os.environ.update(fs[2])
        eng.set_field_stats(cls5 % fs[0] if fs[0] > 1 else None, fs[0], fs[1])
        for k in SWITCHES:
            os.environ.pop(k, None)

    for name in names:
        configure(name)
        print(f"# {name}: {eng.launch_info()['field_stats']}", flush=True)
    for r in range(1, a.rounds + 1):
        for name in names:
            configure(name)
            eng.step(16)                    # the region starts with the variant's kernels loaded
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "host":
                occ = np.zeros((5, 144), np.int64)
                for _ in range(a.host_steps):
                    eng.step(1)
                    pos, cnt, _ = eng.get_state()
                    live = np.arange(pos.shape[1])[None, :] < cnt[:, None]
                    key = cls5[:, None] * 144 + pos.astype(np.int64)
                    occ += np.bincount(key[live], minlength=5 * 144).reshape(5, 144)
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
