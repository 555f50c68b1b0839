"""Evacuation times of E replicas of one room: the batched ``main.py``.

The reference's ``main.py:44-56`` steps one ``FloorFieldModel`` until the room is empty and
prints ``Simulation finished in {step} steps`` (``model/ffm_core.py:119-133`` ``run()`` does
the same).  This driver runs ``--envs`` independent replicas of that loop on one GPU,
``--episodes`` evacuations each, with the engine's on-device episode log
(``Engine.run_episodes``), and writes

* ``steps_per_episode.csv``: ``episode_num,env,N,steps`` -- the columns ``episode_num``, ``N``
  and ``steps`` are those the reference's ``analyze_steps_by_n.py`` reads;
* ``summary.txt``: count, mean, std, min, max of the evacuation times and the steps per second.

    python -m ffm_amd.evac --room 12 12 --N 32 --envs 4096 --episodes 4 --out runs/evac
    python -m ffm_amd.evac --map map.npy --sff sff.npy --N 50 --envs 1024 --out runs/evac
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np


def steps_csv(records: np.ndarray, episodes: int, N: int) -> str:
    """The text of steps_per_episode.csv from episode records [n, 4] int32 {env, episode
    index k, steps, t_end} (Engine.drain_episodes): one row per record in (env, k) order,
    episode_num = env * episodes + k + 1."""
    rec = np.asarray(records, dtype=np.int64).reshape(-1, 4)
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    lines = ["episode_num,env,N,steps"]
    for env, k, steps, _ in rec.tolist():
        lines.append(f"{env * episodes + k + 1},{env},{N},{steps}")
    return "\n".join(lines) + "\n"


def records_from_steps(steps: np.ndarray, env_base: int = 0) -> np.ndarray:
    """Engine.run_episodes' [E, per_env] lengths as records {env, k, steps, 0}."""
    steps = np.asarray(steps)
    E, K = steps.shape
    env = np.repeat(np.arange(E, dtype=np.int64) + env_base, K)
    k = np.tile(np.arange(K, dtype=np.int64), E)
    return np.stack([env, k, steps.reshape(-1).astype(np.int64), np.zeros(E * K, np.int64)], axis=1)


def summary_text(steps: np.ndarray, total_steps: int, seconds: float) -> str:
    s = np.asarray(steps, dtype=np.float64).reshape(-1)
    rate = total_steps / seconds if seconds > 0 else float("nan")
    return (f"count {s.size}\nmean {s.mean():.6f}\nstd {s.std():.6f}\nmin {int(s.min())}\nmax {int(s.max())}\n"
            f"steps_per_second {rate:.1f}\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--map", help=".npy map (0 free, 2 wall, 3 exit)")
    ap.add_argument("--sff", help=".npy static floor field of the map")
    ap.add_argument("--room", nargs=2, type=int, metavar=("H", "W"), help="a walled H x W room with one exit")
    ap.add_argument("--N", type=int, default=32, help="agents per env")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=1, help="evacuations per env")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--k_S", type=float, default=3)
    ap.add_argument("--k_D", type=float, default=1)
    ap.add_argument("--diffuse", type=float, default=0.2)
    ap.add_argument("--decay", type=float, default=0.2)
    ap.add_argument("--neighborhood", choices=("neumann", "moore"), default="moore")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--out", required=True, metavar="DIR")
    a = ap.parse_args(argv)
    if bool(a.map) != bool(a.sff) or bool(a.map) == bool(a.room):
        ap.error("give either --map and --sff, or --room H W")

    from .data import l1_sff, make_room
    from .engine import Engine
    if a.room:
        m = make_room(*a.room)
        sff = l1_sff(m)
    else:
        m, sff = np.load(a.map), np.load(a.sff)
    params = {"k_S": a.k_S, "k_D": a.k_D, "diffuse": a.diffuse, "decay": a.decay, "neighborhood": a.neighborhood}
    eng = Engine(m, sff, n_envs=a.envs, n_agents=a.N, params=params, rng="philox", seed=a.seed,
                 auto_reset=a.episodes > 1)
    eng.set_episode_log(hist_bins=0)
    eng.reset()
    t0 = time.perf_counter()
    steps = eng.run_episodes(per_env=a.episodes, max_steps=a.max_steps)
    dt = time.perf_counter() - t0
    taken = eng.counters()["steps"]
    eng.close()

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "steps_per_episode.csv"), "w") as f:
        f.write(steps_csv(records_from_steps(steps), a.episodes, a.N))
    text = summary_text(steps, taken * a.envs, dt)
    with open(os.path.join(a.out, "summary.txt"), "w") as f:
        f.write(text)
    print(text, end="")
    print(f"Simulation finished: {a.envs} envs x {a.episodes} episodes in {taken} steps")


if __name__ == "__main__":
    main()
