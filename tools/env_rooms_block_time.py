"""Step time of a 64x64 engine (config 3's shape: A = N = 512, Neumann) with per-env rooms on the block
kernel, timed like bench.py's plain line (reset, burn-in + warmup, one region of back-to-back step
launches between device syncs).

    python tools/env_rooms_block_time.py --variant {pep1,room1,room32,eng32,room4,eng4} [--envs 8192] [--steps 300]

pep1:    the default engine with one parameter set equal to the create-time parameters: the block kernel's
         per-env (PEP) form, what the room form is built on
room1:   per-env rooms, kernel="block", with one room (the create-time room): the room form on the same work
room32:  32 rooms (16 exit positions along the top wall x exit widths 1 and 2), env e in room e % 32
eng32:   what that replaces: 32 homogeneous engines of envs / 32 envs, one per room, stepped one after
         another on one stream; the time is that of all of them together
room4:   the first 4 of the rooms, env e in room e % 4
eng4:    four homogeneous engines of envs / 4 envs
Prints one JSON line: variant, kernel, grid, ms_per_step, agent-steps/s.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ("pep1", "room1", "room32", "eng32", "room4", "eng4")


def sweep_rooms(H, W, n):
    """n rooms: exit positions spread along the top wall, widths 1 and 2 alternating; room 0 is the
    default room (make_room(H, W))."""
    from ffm_amd.data import geodesic_sff, make_room
    rooms = [make_room(H, W)]
    for r in range(1, n):
        y = 2 + (r // 2) * max(1, (W - 6) // max(1, (n + 1) // 2))
        rooms.append(make_room(H, W, exit_pos=(0, min(y, W - 4)), exit_width=1 + r % 2))
    return [(m, geodesic_sff(m)) for m in rooms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS, required=True)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--burn-in", type=int, default=500)
    ap.add_argument("--neighborhood", default="neumann")
    a = ap.parse_args()
    import torch
    from ffm_amd.engine import Engine
    torch.cuda.set_device(0)
    n_rooms = {"pep1": 1, "room1": 1, "room32": 32, "eng32": 32, "room4": 4, "eng4": 4}[a.variant]
    rooms = sweep_rooms(a.size, a.size, n_rooms)
    params = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": a.neighborhood}

    def engine(room, n_envs, env_base=0):
        return Engine(*room, n_envs=n_envs, n_agents=a.agents, params=params, rng="philox", seed=42,
                      auto_reset=True, env_base=env_base)

    if a.variant.startswith("eng"):
        n = a.envs // n_rooms
        engs = [engine(rooms[r], n, r * n) for r in range(n_rooms)]
    else:
        engs = [engine(rooms[0], a.envs)]
        if a.variant == "pep1":
            engs[0].set_env_params([{}])
        else:
            engs[0].set_env_rooms(rooms, kernel="block")
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
    for eng in engs:
        eng.close()
    print(json.dumps({"variant": a.variant, "kernel": info["kernel"], "blocks": info["blocks"], "K": info["K"],
                      "block_size": info["block_size"], "env_rooms": info["env_rooms"], "engines": len(engs),
                      "envs": a.envs, "steps": a.steps, "ms_per_step": el / a.steps * 1e3,
                      "value": (c1 - c0) / el, "unit": "agent-steps/s"}))


if __name__ == "__main__":
    main()
