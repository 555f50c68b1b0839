"""Step time of a 12x12 engine with per-env rooms on the group kernel's room form against the lane
kernel's, timed like bench.py's plain line (reset, burn-in + warmup, one region of K back-to-back
step launches between device syncs).

    python tools/env_rooms_group_time.py --variant {lane4,group4,pepg1,roomg1,four16k} [--envs 65536] [--steps 500]

lane4:    the four rooms of tests/test_gpu_env_rooms.py, env e in room e % 4, on the lane kernel's room form
          (set_env_rooms(rooms), the default)
group4:   the same rooms and mapping on the group kernel's room form (set_env_rooms(rooms, kernel="group"))
pepg1:    the default engine with one parameter set equal to the create-time parameters, on the group
          kernel's per-env form (set_env_params([{}], kernel="group")): what the room form is built on
roomg1:   one room (the create-time room) on the group kernel's room form: the cost of the room form itself
four16k:  what the feature replaces: four homogeneous engines of envs / 4 envs, one per room, each on
          its own kernel, stepped one after another; the time is that of all of them together
Prints one JSON line: variant, kernel, grid, ms_per_step, agent-steps/s.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def four_rooms():
    from ffm_amd.data import make_room, l1_sff
    r0 = make_room(12, 12)
    r1 = make_room(12, 12)
    r1[0, 5] = 3
    r2 = make_room(12, 12, exit_pos=(6, 0))
    r2[1:3, 9:11] = 2
    r2[9:11, 9:11] = 2
    r3 = make_room(12, 12)
    r3[11, 3] = 3
    r3[1:3, 1:3] = 2
    return [(m, l1_sff(m)) for m in (r0, r1, r2, r3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("lane4", "group4", "pepg1", "roomg1", "four16k"), required=True)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--neighborhood", default="neumann")
    a = ap.parse_args()
    import torch
    from ffm_amd.engine import Engine
    torch.cuda.set_device(0)
    rooms = four_rooms()
    params = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": a.neighborhood}

    def engine(room, n_envs, env_base=0):
        return Engine(*room, n_envs=n_envs, n_agents=32, params=params, rng="philox", seed=42, auto_reset=True,
                      env_base=env_base)

    if a.variant == "four16k":
        n = a.envs // 4
        engs = [engine(rooms[r], n, r * n) for r in range(4)]
    else:
        engs = [engine(rooms[0], a.envs)]
        if a.variant == "pepg1":
            engs[0].set_env_params([{}], kernel="group")
        elif a.variant == "roomg1":
            engs[0].set_env_rooms(rooms[:1], kernel="group")
        elif a.variant == "group4":
            engs[0].set_env_rooms(rooms, kernel="group")
        else:
            engs[0].set_env_rooms(rooms, kernel="lane")
    stream = torch.cuda.current_stream()
    for eng in engs:
        eng.reset(stream)
        eng.step(a.burn_in + a.warmup, stream)
    c0 = sum(eng.counters(stream)["agent_steps"] for eng in engs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for eng in engs:
        eng.step(a.steps, stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    c1 = sum(eng.counters(stream)["agent_steps"] for eng in engs)
    info = engs[0].launch_info()
    occ = engs[0].group_occupancy(True) if info["kernel"] == "group" else 0
    for eng in engs:
        eng.close()
    print(json.dumps({"variant": a.variant, "kernel": info["kernel"], "group_g": info["group_g"],
                      "group_one": info["group_one"], "blocks": info["blocks"], "step_shards": info["step_shards"],
                      "shard_blocks": info["shard_blocks"], "blocks_per_cu": occ, "env_rooms": info["env_rooms"],
                      "engines": len(engs), "envs": a.envs, "steps": a.steps, "ms_per_step": el / a.steps * 1e3,
                      "value": (c1 - c0) / el, "unit": "agent-steps/s"}))


if __name__ == "__main__":
    main()
