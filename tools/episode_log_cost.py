"""What the episode log costs the C2 step (12x12, 32 agents, 65,536 envs, Neumann) when it is on.

    python tools/episode_log_cost.py [--envs 65536] [--steps 496] [--rounds 6] [--bins 256]

Four engines of the same seed, each burnt in for 1,000 steps, then timed round by round
(interleaved) over `--steps` steps:
  off            the feature off (bench.py's workload)
  stats          histogram + summary only
  log+stats      records + histogram, one step(n) call, the log large enough for the region
  log+stats/16   the same, stepped 16 steps per call with a drain after each (the 16 E default
                 capacity; the drains' copies and synchronisations are inside the timed region)
One line per run: variant, round, us per step, records logged.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=496)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--bins", type=int, default=256)
    a = ap.parse_args()
    import torch
    from ffm_amd.data import l1_sff, make_room
    from ffm_amd.engine import Engine
    m = make_room(12, 12)
    s = l1_sff(m)
    p = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}
    E = a.envs
    variants = {"off": None, "stats": (0, a.bins), "log+stats": (max(4096, a.steps * E // 16), a.bins),
                "log+stats/16": (16 * E, a.bins)}
    engines = {}
    for name, log in variants.items():
        eng = Engine(m, s, n_envs=E, n_agents=32, params=p, rng="philox", seed=42, auto_reset=True)
        if log:
            eng.set_episode_log(*log)
        eng.reset()
        eng.step(1000)
        if log and log[0]:
            eng.drain_episodes()
        engines[name] = eng
    torch.cuda.synchronize()
    for r in range(1, a.rounds + 1):
        for name, eng in engines.items():
            n_rec = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name.endswith("/16"):
                for _ in range(a.steps // 16):
                    eng.step(16)
                    n_rec += len(eng.drain_episodes())
            else:
                eng.step(a.steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if name == "log+stats":
                n_rec = len(eng.drain_episodes())
            done = a.steps // 16 * 16 if name.endswith("/16") else a.steps
            print(f"{name} round{r} {dt / done * 1e6:.2f} us_per_step {n_rec} records", flush=True)
    st = engines["stats"].episode_stats()
    print(f"stats: count {st['count']} mean {st['mean']:.2f} std {st['std']:.2f} min {st['min']} max {st['max']}")
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
