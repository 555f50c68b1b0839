"""Step time of a 12x12 engine with per-env parameters on, timed like bench.py's plain line
(reset, burn-in + warmup, one region of K back-to-back step launches between device syncs).

    python tools/env_params_time.py --variant {lane,same5,diff5} [--kernel {lane,group}] [--envs 65536] [--steps 500]

lane:   a homogeneous engine on the lane kernel (envs_per_block = -2), the feature off
same5:  the default engine with five identical sets (the create-time parameters): the lane
        kernel's per-env form on the same work as `lane`
diff5:  the five different sets of tests/test_gpu_env_params.py (k_S, k_D, diffuse, decay, N)
--kernel: the kernel that steps same5 / diff5 (Engine.set_env_params(kernel=...)): the lane kernel's
per-env form (the default) or the group kernel's own.
Prints one JSON line: variant, kernel, grid, shards, ms_per_step, agent-steps/s.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIFF5 = [dict(zip(("k_S", "k_D", "diffuse", "decay", "n_agents"), s)) for s in
         ((3, 1, 0.2, 0.2, 32), (0.5, 0, 0.2, 0.2, 5), (10, 2.5, 0.05, 0.6, 17), (1.5, 1, 0.5, 0.1, 1),
          (1, 4, 0.3, 0.3, 24))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("lane", "same5", "diff5"), required=True)
    ap.add_argument("--kernel", choices=("lane", "group"), default=None)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--neighborhood", default="neumann")
    a = ap.parse_args()
    import torch
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    torch.cuda.set_device(0)
    m = make_room(12, 12)
    params = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": a.neighborhood}
    eng = Engine(m, l1_sff(m), n_envs=a.envs, n_agents=32, params=params, rng="philox", seed=42, auto_reset=True,
                 envs_per_block=-2 if a.variant == "lane" else 0)
    if a.variant == "same5":
        eng.set_env_params([{}] * 5, kernel=a.kernel)
    elif a.variant == "diff5":
        eng.set_env_params(DIFF5, kernel=a.kernel)
    stream = torch.cuda.current_stream()
    eng.reset(stream)
    eng.step(a.burn_in + a.warmup, stream)
    c0 = eng.counters(stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.step(a.steps, stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    c1 = eng.counters(stream)
    info = eng.launch_info()
    eng.close()
    print(json.dumps({"variant": a.variant, "kernel": info["kernel"], "blocks": info["blocks"], "group_g": info["group_g"],
                      "step_shards": info["step_shards"], "shard_blocks": info["shard_blocks"],
                      "group_one": info["group_one"], "envs": a.envs,
                      "steps": a.steps, "ms_per_step": el / a.steps * 1e3,
                      "value": (c1["agent_steps"] - c0["agent_steps"]) / el, "unit": "agent-steps/s"}))


if __name__ == "__main__":
    main()
