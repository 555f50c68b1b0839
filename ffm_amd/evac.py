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

A sweep runs in the same engine (``Engine.set_env_params``): ``--sweep NAME=v1,v2,...``
(repeatable; NAME one of k_S k_D diffuse decay N) makes the Cartesian product of the lists, in
argument order, the parameter sets; env e runs set e % P, so every wave mixes long and short
episodes.  ``steps_per_episode.csv`` then carries each env's own N and gains the columns
``k_S,k_D,diffuse,decay`` (``analyze_steps_by_n.py`` reads an N sweep directly), and
``sweep_summary.csv`` has one row per set: parameters, count, mean, std, min, max.

    python -m ffm_amd.evac --room 12 12 --sweep N=5,10,20,32 --sweep k_D=0,1,4 --envs 4096 --out runs/sweep

Rooms sweep in the same engine too (``Engine.set_env_rooms``): ``--rooms MAP.npy:SFF.npy ...`` gives
several rooms of one shape, and ``--sweep exit_width=1,2,4`` (with ``--room H W``) makes one room per
width, the exit starting at the default position.  The room axis joins the Cartesian product as its
slowest-varying axis (env e still runs combination e % P); both CSVs gain a ``room`` column (the room's
index) and, when ``exit_width`` is swept, an ``exit_width`` column.  A room sweep needs no parameter sweep.

    python -m ffm_amd.evac --room 12 12 --sweep exit_width=1,2,4 --sweep N=5,20,32 --envs 4096 --out runs/rooms

``--sweep-kernel {lane,group}`` picks the kernel that steps a sweep in a 12x12 engine (one born on
the group kernel): the lane kernel's per-env form or the group kernel's own.  The outputs are
the same bits either way; the default (SWEEP_KERNEL_DEFAULT) is the one that measured faster.

Rooms beyond the lane kernel's shapes (an engine whose kernel is ``wave`` or ``block``, such as the
reference's 50x50 room) sweep with the block kernel's room form, which the driver picks by itself
(``room_sweep_kernel``).  ``--room-kernel {lane,group,block}`` names the room form instead
(``Engine.set_env_rooms``'s ``kernel``): ``group`` is the group kernel's own room form for 12x12
engines, opt-in, same outputs as the lane form.  ``--sff geodesic`` gives rooms made by ``--room`` the obstacle-aware static
floor field (``data.geodesic_sff``) instead of the L1 distance; on rooms without obstacles the two
are the same bits.

    python -m ffm_amd.evac --room 50 50 --N 100 --sweep exit_width=1,2,4 --envs 1024 --out runs/rooms50

``--fields`` adds what the reference reads off its per-step position log (``main.py:44-54``,
``visualize_trajectory.py``): where the crowd stands and how the room empties, summed on the device
(``Engine.set_field_stats``) with one class per sweep combination (one class without a sweep).  It
writes ``occupancy.npy`` ([P, H, W] uint64 visits of every cell), ``occupancy.csv``
(``set,row,col,occupancy``, the cells ever occupied), ``observed.csv`` (``set,observed``: divide a
set's map by it for the mean density) and, with ``--curve-bins B``, ``remaining.csv``
(``set,tau,remaining,alive``: agents inside and envs still evacuating tau steps after placement).
With ``--episodes`` > 1 an env that finishes early keeps evacuating until the slowest is done, and
those episodes are observed too: normalise by ``observed`` and ``alive``, not by ``--episodes``.

    python -m ffm_amd.evac --room 12 12 --sweep exit_width=1,2,4 --fields --curve-bins 128 --envs 4096 --out runs/fields

``--flow`` adds which exit the agents leave through and when (``model/ffm_core.py:66-72, 100-102``
decides the door), counted on the device (``Engine.set_exit_flow``) with one class per sweep
combination: every exit cell of every room is a door, numbered in row-major order within its room.
It writes ``exit_usage.csv`` (``set,door,exited``), ``doors.csv`` (``room,door,row,col``: where each
door is) and, with ``--curve-bins B``, ``outflow.csv`` (``set,door,tau,exited``: the agents that left
through the door tau steps after placement; the last tau holds every later step too).

    python -m ffm_amd.evac --room 12 12 --sweep exit_width=1,2,4 --flow --curve-bins 128 --envs 4096 --out runs/flow

``--motion`` adds how the crowd moves (what ``visualize_trajectory.py`` and ``inspect_trajectory.py``
show from the position log), summed on the device (``Engine.set_motion_stats``) with one class per
sweep combination.  It writes ``flux.npy`` ([P, H, W, NB + 1] uint64: agents that stepped out of a
cell in each direction of the reference's neighbour order, the last entry those that stood still),
``flux.csv`` (``set,row,col,direction,count``, the non-zero entries), ``egress_by_origin.csv``
(``set,row,col,count,steps_sum``: the agents placed on a cell that have left and the sum of their
egress times, for the cells with any) and, with ``--curve-bins B``, ``speed.csv``
(``set,tau,present,moved``: moved / present is the mean speed tau steps after placement).

    python -m ffm_amd.evac --room 12 12 --sweep exit_width=1,2,4 --motion --curve-bins 128 --envs 4096 --out runs/motion
"""
from __future__ import annotations

import argparse
import itertools
import os
import time

import numpy as np


SWEEP_NAMES = ("k_S", "k_D", "diffuse", "decay", "N")
ROOM_SWEEP_NAMES = ("exit_width",)   # swept through the room axis (--room H W), not a parameter set
# The kernel of a sweep in an engine born on the group kernel when --sweep-kernel is not given
# (every other engine has the one choice): the group kernel's own per-env form, which measured
# faster than the lane kernel's in every run at 4,096, 32,768 and 65,536 envs (1.36, 1.64 and 1.66
# times; profiles/env_params_group/ab.txt).
SWEEP_KERNEL_DEFAULT = "group"


SFF_KINDS = ("l1", "geodesic")          # --sff for rooms made by --room


def parse_sff(text, made_room: bool):
    """The value of ``--sff``: (kind, path).  ``l1`` / ``geodesic`` name the field of a room made by
    ``--room`` (kind, None); anything else is the .npy file that goes with ``--map`` (None, path).
    None -> ("l1", None) with ``--room``, else (None, None)."""
    if text is None:
        return ("l1", None) if made_room else (None, None)
    if text in SFF_KINDS:
        if not made_room:
            raise ValueError(f"--sff {text} wants --room H W (with --map, --sff is the field's .npy file)")
        return text, None
    if made_room:
        raise ValueError(f"--sff with --room is one of {' '.join(SFF_KINDS)}, got {text!r}")
    return None, text


def room_sff(kind: str, m: np.ndarray, neighborhood: str) -> np.ndarray:
    """The static floor field of a made room: ``l1`` or ``geodesic`` (the engine's moves)."""
    from .data import geodesic_sff, l1_sff
    return l1_sff(m) if kind == "l1" else geodesic_sff(m, neighborhood=neighborhood)


def room_sweep_kernel(launch_info: dict):
    """The ``kernel`` argument of ``Engine.set_env_rooms`` for an engine with this ``launch_info()``:
    "block" where the create-time kernel is ``wave`` or ``block`` (the block kernel's room form),
    None elsewhere (lane and group engines have the lane form; a ``block_scratch`` engine has none
    and keeps the refusal of a plain call)."""
    return "block" if launch_info.get("kernel") in ("wave", "block") else None


def parse_sweep(text: str):
    """``NAME=v1,v2,...`` -> (NAME, [values]); N and exit_width values are ints, the others floats."""
    name, sep, vals = text.partition("=")
    name = name.strip()
    if not sep or name not in SWEEP_NAMES + ROOM_SWEEP_NAMES:
        raise ValueError("--sweep wants NAME=v1,v2,... with NAME one of "
                         f"{' '.join(SWEEP_NAMES + ROOM_SWEEP_NAMES)}: {text!r}")
    items = [v for v in vals.split(",") if v.strip()]
    if not items:
        raise ValueError(f"--sweep {name}: no values")
    return name, [int(v) if name in ("N",) + ROOM_SWEEP_NAMES else float(v) for v in items]


def sweep_grid(sweeps, base: dict, n_rooms: int = 0, exit_widths=None) -> list:
    """The parameter sets of a sweep: the Cartesian product of the (name, values) lists in
    argument order (the first name varies slowest), every other parameter from `base`.  Each
    set is a dict with the keys k_S, k_D, diffuse, decay, N.

    With `n_rooms` > 0 the room is one more axis, the slowest of all: the combinations of room 0
    come first, and every set also has "room" (the room's index) and, with `exit_widths` (one per
    room), "exit_width"."""
    names = [n for n, _ in sweeps]
    if len(set(names)) != len(names):
        raise ValueError("--sweep: a name is given twice")
    if exit_widths is not None and len(exit_widths) != n_rooms:
        raise ValueError("one exit width per room")
    sets = []
    for room in range(max(1, n_rooms)):
        for combo in itertools.product(*[v for _, v in sweeps]):
            st = {k: base[k] for k in SWEEP_NAMES}
            st.update(zip(names, combo))
            if n_rooms > 0:
                st["room"] = room
                if exit_widths is not None:
                    st["exit_width"] = exit_widths[room]
            sets.append(st)
    return sets


def _room_cols(sets) -> tuple:
    """The room columns the sets carry: (), ("room",) or ("room", "exit_width")."""
    return tuple(c for c in ("room",) + ROOM_SWEEP_NAMES if sets and c in sets[0])


def env_assignment(n_envs: int, n_sets: int) -> np.ndarray:
    """Env e runs set e % P."""
    if n_envs < n_sets:
        raise ValueError(f"--envs must be at least the number of sets ({n_sets})")
    return (np.arange(n_envs) % n_sets).astype(np.int32)


def _num(v) -> str:
    return f"{v:g}" if isinstance(v, float) else str(v)


def steps_csv(records: np.ndarray, episodes: int, N: int, sets=None, set_of_env=None, env_base: int = 0) -> str:
    """The text of steps_per_episode.csv from episode records [n, 4] int32 {env, episode
    index k, steps, t_end} (Engine.drain_episodes): one row per record in (env, k) order,
    episode_num = env * episodes + k + 1.  With `sets` (sweep_grid) and `set_of_env` the N
    column carries the env's own N and the columns k_S, k_D, diffuse, decay follow."""
    rec = np.asarray(records, dtype=np.int64).reshape(-1, 4)
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    if sets is None:
        lines = ["episode_num,env,N,steps"]
        for env, k, steps, _ in rec.tolist():
            lines.append(f"{env * episodes + k + 1},{env},{N},{steps}")
        return "\n".join(lines) + "\n"
    cols = ("k_S", "k_D", "diffuse", "decay") + _room_cols(sets)   # a room sweep: room[, exit_width] follow
    lines = ["episode_num,env,N,steps," + ",".join(cols)]
    for env, k, steps, _ in rec.tolist():
        st = sets[int(set_of_env[env - env_base])]
        lines.append(f"{env * episodes + k + 1},{env},{st['N']},{steps}," + ",".join(_num(st[c]) for c in cols))
    return "\n".join(lines) + "\n"


def sweep_summary_csv(steps: np.ndarray, sets, set_of_env) -> str:
    """The text of sweep_summary.csv: one row per set with its parameters and the count, mean,
    std, min, max of the evacuation times [E, per_env] of its envs."""
    steps = np.asarray(steps)
    soe = np.asarray(set_of_env)
    cols = ("k_S", "k_D", "diffuse", "decay", "N") + _room_cols(sets)   # a room sweep: room[, exit_width] follow N
    lines = ["set," + ",".join(cols) + ",count,mean,std,min,max"]
    for p, st in enumerate(sets):
        s = steps[soe == p].astype(np.float64).reshape(-1)
        head = f"{p}," + ",".join(_num(st[c]) for c in cols)
        if s.size == 0:
            lines.append(head + ",0,nan,nan,0,0")
        else:
            lines.append(head + f",{s.size},{s.mean():.6f},{s.std():.6f},{int(s.min())},{int(s.max())}")
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


def observed_csv(observed) -> str:
    """The text of observed.csv from Engine.field_stats()["observed"] [P]: ``set,observed``, the
    env states each set's occupancy map sums (occupancy / observed is a cell's mean density)."""
    obs = np.asarray(observed).reshape(-1)
    return "\n".join(["set,observed"] + [f"{p},{int(v)}" for p, v in enumerate(obs.tolist())]) + "\n"


def occupancy_csv(occupancy) -> str:
    """The text of occupancy.csv from Engine.field_stats()["occupancy"] [P, H, W]:
    ``set,row,col,occupancy``, one row per cell that was ever occupied, in (set, row, col) order
    (occupancy.npy holds the whole array)."""
    occ = np.asarray(occupancy)
    lines = ["set,row,col,occupancy"]
    for p, x, y in np.argwhere(occ != 0).tolist():
        lines.append(f"{p},{x},{y},{int(occ[p, x, y])}")
    return "\n".join(lines) + "\n"


def remaining_csv(remaining, alive) -> str:
    """The text of remaining.csv from Engine.field_stats()' curves [P, bins]:
    ``set,tau,remaining,alive`` for every set and every tau = 0 .. bins - 1 (tau: steps since the
    placement; the last holds every later step too; tau = 0, the placement, is never observed).
    remaining / episodes is the mean number inside at tau, its slope the outflow."""
    rem, al = np.asarray(remaining), np.asarray(alive)
    if rem.shape != al.shape or rem.ndim != 2:
        raise ValueError("remaining and alive are [sets, bins] arrays of one shape")
    lines = ["set,tau,remaining,alive"]
    for p in range(rem.shape[0]):
        for tau in range(rem.shape[1]):
            lines.append(f"{p},{tau},{int(rem[p, tau])},{int(al[p, tau])}")
    return "\n".join(lines) + "\n"


def exit_usage_csv(exited) -> str:
    """The text of exit_usage.csv from Engine.exit_flow()["exited"] [P, D]: ``set,door,exited`` for
    every set and door, in that order (a door the set's room does not have reads 0)."""
    ex = np.asarray(exited)
    if ex.ndim != 2:
        raise ValueError("exited is a [sets, doors] array")
    lines = ["set,door,exited"]
    for p in range(ex.shape[0]):
        for d in range(ex.shape[1]):
            lines.append(f"{p},{d},{int(ex[p, d])}")
    return "\n".join(lines) + "\n"


def doors_csv(door_of_cell) -> str:
    """The text of doors.csv from Engine.exit_flow()["door_of_cell"] [R, H, W] (-1 off the exits):
    ``room,door,row,col``, one row per exit cell in (room, row, col) order."""
    doc = np.asarray(door_of_cell)
    if doc.ndim != 3:
        raise ValueError("door_of_cell is a [rooms, H, W] array")
    lines = ["room,door,row,col"]
    for r, x, y in np.argwhere(doc >= 0).tolist():
        lines.append(f"{r},{int(doc[r, x, y])},{x},{y}")
    return "\n".join(lines) + "\n"


def outflow_csv(outflow) -> str:
    """The text of outflow.csv from Engine.exit_flow()["outflow"] [P, D, bins]:
    ``set,door,tau,exited`` for every set, door and tau = 0 .. bins - 1 (tau: steps since the
    placement; the last holds every later step too; nobody leaves at tau = 0)."""
    out = np.asarray(outflow)
    if out.ndim != 3:
        raise ValueError("outflow is a [sets, doors, bins] array")
    lines = ["set,door,tau,exited"]
    for p in range(out.shape[0]):
        for d in range(out.shape[1]):
            for tau in range(out.shape[2]):
                lines.append(f"{p},{d},{tau},{int(out[p, d, tau])}")
    return "\n".join(lines) + "\n"


def flux_csv(flux) -> str:
    """The text of flux.csv from Engine.motion_stats()["flux"] [P, H, W, NB + 1]:
    ``set,row,col,direction,count``, one row per non-zero entry in (set, row, col, direction) order
    (direction: the index into motion_stats()["directions"], the last one a stay; flux.npy holds
    the whole array)."""
    fx = np.asarray(flux)
    if fx.ndim != 4:
        raise ValueError("flux is a [sets, H, W, directions] array")
    lines = ["set,row,col,direction,count"]
    for p, x, y, d in np.argwhere(fx != 0).tolist():
        lines.append(f"{p},{x},{y},{d},{int(fx[p, x, y, d])}")
    return "\n".join(lines) + "\n"


def speed_csv(present, moved) -> str:
    """The text of speed.csv from Engine.motion_stats()' curves [P, bins]: ``set,tau,present,moved``
    for every set and every tau = 0 .. bins - 1 (tau: steps since the placement; the last holds
    every later step too; nothing is counted at tau = 0).  moved / present is the mean speed."""
    pr, mv = np.asarray(present), np.asarray(moved)
    if pr.shape != mv.shape or pr.ndim != 2:
        raise ValueError("present and moved are [sets, bins] arrays of one shape")
    lines = ["set,tau,present,moved"]
    for p in range(pr.shape[0]):
        for tau in range(pr.shape[1]):
            lines.append(f"{p},{tau},{int(pr[p, tau])},{int(mv[p, tau])}")
    return "\n".join(lines) + "\n"


def egress_by_origin_csv(egress_count, egress_steps) -> str:
    """The text of egress_by_origin.csv from Engine.motion_stats()' egress tables [P, H, W]:
    ``set,row,col,count,steps_sum``, one row per cell that agents who left were placed on, in (set,
    row, col) order.  steps_sum / count is the mean egress time from the cell."""
    ct, st = np.asarray(egress_count), np.asarray(egress_steps)
    if ct.shape != st.shape or ct.ndim != 3:
        raise ValueError("egress_count and egress_steps are [sets, H, W] arrays of one shape")
    lines = ["set,row,col,count,steps_sum"]
    for p, x, y in np.argwhere(ct != 0).tolist():
        lines.append(f"{p},{x},{y},{int(ct[p, x, y])},{int(st[p, x, y])}")
    return "\n".join(lines) + "\n"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--map", help=".npy map (0 free, 2 wall, 3 exit)")
    ap.add_argument("--sff", help=".npy static floor field of the map; with --room: l1 (default) or geodesic "
                                  "(obstacle-aware, data.geodesic_sff)")
    ap.add_argument("--room", nargs=2, type=int, metavar=("H", "W"), help="a walled H x W room with one exit")
    ap.add_argument("--rooms", nargs="+", metavar="MAP.npy:SFF.npy",
                    help="several rooms of one shape in one engine (the room axis of the sweep)")
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
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME=v1,v2,...",
                    help="sweep k_S, k_D, diffuse, decay, N or (with --room) exit_width in one engine "
                         "(repeatable: Cartesian product)")
    ap.add_argument("--sweep-kernel", choices=("lane", "group"), default=None,
                    help="the kernel that steps a sweep in an engine born on the group kernel (12x12): the lane "
                         f"kernel's per-env form or the group kernel's own (default: {SWEEP_KERNEL_DEFAULT}; "
                         "same outputs either way)")
    ap.add_argument("--room-kernel", choices=("lane", "group", "block"), default=None,
                    help="the kernel that steps a room sweep (Engine.set_env_rooms' kernel): lane, the group kernel's "
                         "own room form (12x12 engines, opt-in) or block (default: the driver's pick, "
                         "room_sweep_kernel; same outputs whichever runs)")
    ap.add_argument("--fields", action="store_true",
                    help="also write the on-device field statistics (Engine.set_field_stats), one class per sweep "
                         "combination: occupancy.npy, occupancy.csv, observed.csv")
    ap.add_argument("--flow", action="store_true",
                    help="also write the on-device exit flow (Engine.set_exit_flow), one class per sweep "
                         "combination: exit_usage.csv, doors.csv")
    ap.add_argument("--motion", action="store_true",
                    help="also write the on-device motion statistics (Engine.set_motion_stats), one class per sweep "
                         "combination: flux.npy, flux.csv, egress_by_origin.csv")
    ap.add_argument("--curve-bins", type=int, default=0, metavar="B",
                    help="with --fields, --flow or --motion: the curves over tau = 0 .. B - 1 steps since placement "
                         "(remaining.csv, outflow.csv, speed.csv)")
    ap.add_argument("--out", required=True, metavar="DIR")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.curve_bins < 0 or (a.curve_bins and not (a.fields or a.flow or a.motion)):
        ap.error("--curve-bins B wants B >= 0 and --fields, --flow or --motion")
    if sum(map(bool, (a.map, a.room, a.rooms))) != 1 or (a.rooms and a.sff):
        ap.error("give either --map and --sff, or --room H W, or --rooms MAP.npy:SFF.npy ...")
    try:
        sff_kind, sff_path = parse_sff(a.sff, bool(a.room))
    except ValueError as err:
        ap.error(str(err))
    if bool(a.map) != bool(sff_path):
        ap.error("give either --map and --sff, or --room H W, or --rooms MAP.npy:SFF.npy ...")

    from .data import make_room
    from .engine import Engine
    params = {"k_S": a.k_S, "k_D": a.k_D, "diffuse": a.diffuse, "decay": a.decay, "neighborhood": a.neighborhood}
    rooms = widths = None      # the room axis: (map, sff) pairs, and the exit widths that made them
    sets = soe = None
    n_max = a.N
    try:
        sweeps = [parse_sweep(t) for t in a.sweep]
        room_sweeps = [sw for sw in sweeps if sw[0] in ROOM_SWEEP_NAMES]
        sweeps = [sw for sw in sweeps if sw[0] not in ROOM_SWEEP_NAMES]
        if len(room_sweeps) > 1:
            raise ValueError("--sweep: a name is given twice")
        if room_sweeps and not a.room:
            raise ValueError("--sweep exit_width wants --room H W")
        if room_sweeps:
            widths = room_sweeps[0][1]
            maps = [make_room(*a.room, exit_pos=(0, a.room[1] // 2), exit_width=w) for w in widths]
            rooms = [(mp, room_sff(sff_kind, mp, a.neighborhood)) for mp in maps]
        elif a.rooms:
            rooms = []
            for text in a.rooms:
                mp, sep, sf = text.partition(":")
                if not sep:
                    raise ValueError(f"--rooms wants MAP.npy:SFF.npy, got {text!r}")
                rooms.append((np.load(mp), np.load(sf).astype(np.float32)))
        if rooms:
            m, sff = rooms[0]
        elif a.room:
            m = make_room(*a.room)
            sff = room_sff(sff_kind, m, a.neighborhood)
        else:
            m, sff = np.load(a.map), np.load(sff_path)
        if sweeps or rooms:
            sets = sweep_grid(sweeps, {**params, "N": a.N}, len(rooms) if rooms else 0, widths)
            soe = env_assignment(a.envs, len(sets))
            n_max = max(st["N"] for st in sets)   # the agent capacity
    except ValueError as err:
        ap.error(str(err))
    eng = Engine(m, sff, n_envs=a.envs, n_agents=n_max, params=params, rng="philox", seed=a.seed,
                 auto_reset=a.episodes > 1)
    try:   # before the reset: its placement takes each env's own room and N
        if rooms:
            eng.set_env_rooms(rooms, np.array([sets[p]["room"] for p in soe], np.int32),
                              kernel=a.room_kernel if a.room_kernel is not None
                              else room_sweep_kernel(eng.launch_info()))
        if sets and (sweeps or not rooms):
            # the room axis is the slowest: combination c has the parameters of combination c % Pp
            n_par = len(sets) // max(1, len(rooms) if rooms else 1)
            kernel = a.sweep_kernel
            if kernel is None and eng.launch_info()["kernel"] == "group":
                kernel = SWEEP_KERNEL_DEFAULT
            eng.set_env_params([{"k_S": st["k_S"], "k_D": st["k_D"], "diffuse": st["diffuse"], "decay": st["decay"],
                                 "n_agents": st["N"]} for st in sets[:n_par]], soe % n_par, kernel=kernel)
    except (NotImplementedError, ValueError) as err:   # e.g. --sweep-kernel group on an engine of another kernel
        eng.close()
        ap.error(str(err))
    eng.set_episode_log(hist_bins=0)
    if a.fields:   # the class is the sweep's combination index
        eng.set_field_stats(classes=soe if sets else None, n_classes=len(sets) if sets else 1,
                            curve_bins=a.curve_bins)
    if a.flow:     # after the rooms: the doors are those of the rooms in effect
        eng.set_exit_flow(classes=soe if sets else None, n_classes=len(sets) if sets else 1, curve_bins=a.curve_bins)
    if a.motion:   # after the rooms too: the direction table is that of the rooms in effect
        eng.set_motion_stats(classes=soe if sets else None, n_classes=len(sets) if sets else 1, curve_bins=a.curve_bins)
    eng.reset()
    t0 = time.perf_counter()
    steps = eng.run_episodes(per_env=a.episodes, max_steps=a.max_steps)
    dt = time.perf_counter() - t0
    taken = eng.counters()["steps"]
    fields = eng.field_stats() if a.fields else None
    flow = eng.exit_flow() if a.flow else None
    motion = eng.motion_stats() if a.motion else None
    eng.close()

    os.makedirs(a.out, exist_ok=True)
    if fields is not None:
        np.save(os.path.join(a.out, "occupancy.npy"), fields["occupancy"])
        texts = {"occupancy.csv": occupancy_csv(fields["occupancy"]), "observed.csv": observed_csv(fields["observed"])}
        if a.curve_bins > 0:
            texts["remaining.csv"] = remaining_csv(fields["remaining"], fields["alive"])
        for name, body in texts.items():
            with open(os.path.join(a.out, name), "w") as f:
                f.write(body)
    if flow is not None:
        texts = {"exit_usage.csv": exit_usage_csv(flow["exited"]), "doors.csv": doors_csv(flow["door_of_cell"])}
        if a.curve_bins > 0:
            texts["outflow.csv"] = outflow_csv(flow["outflow"])
        for name, body in texts.items():
            with open(os.path.join(a.out, name), "w") as f:
                f.write(body)
    if motion is not None:
        np.save(os.path.join(a.out, "flux.npy"), motion["flux"])
        texts = {"flux.csv": flux_csv(motion["flux"]),
                 "egress_by_origin.csv": egress_by_origin_csv(motion["egress_count"], motion["egress_steps"])}
        if a.curve_bins > 0:
            texts["speed.csv"] = speed_csv(motion["present"], motion["moved"])
        for name, body in texts.items():
            with open(os.path.join(a.out, name), "w") as f:
                f.write(body)
    with open(os.path.join(a.out, "steps_per_episode.csv"), "w") as f:
        f.write(steps_csv(records_from_steps(steps), a.episodes, a.N, sets, soe))
    if sets:
        with open(os.path.join(a.out, "sweep_summary.csv"), "w") as f:
            f.write(sweep_summary_csv(steps, sets, soe))
    text = summary_text(steps, taken * a.envs, dt)
    with open(os.path.join(a.out, "summary.txt"), "w") as f:
        f.write(text)
    print(text, end="")
    print(f"Simulation finished: {a.envs} envs x {a.episodes} episodes in {taken} steps")


if __name__ == "__main__":
    main()
