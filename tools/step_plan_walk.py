"""Walks tiny engines through the feature states that select their step plan (engine.cpp, plan())
and records what every state launches and computes.

    python tools/step_plan_walk.py                      # print the walks' result as JSON
    python tools/step_plan_walk.py --record FILE        # ... and write it to FILE
    python tools/step_plan_walk.py --check FILE         # compare with FILE, exit 1 on a difference

tests/test_gpu_step_plan.py replays the walks against tests/golden/step_plan_walk.json.  That file
is recorded from the library of the commit BEFORE a change to the engine's host side (FFM_LIB_PATH
selects the library), never from the change itself: `--commit` names it in the file.

The engines (seed, sets and rooms of the per-env sweep tests): a 12x12 group engine of 135 envs,
created with the switches unset, with FFM_STEP_SHARDS=2 and with FFM_GROUP_ONE=0 (set around the
create call only: the plans computed later then differ from the create plan, which has to come
back untouched); a 16x16 lane engine of 9 envs; a 12x12 wave engine (capacity 40) of 5 envs; a
20x20 block engine of 13 envs.  Every state records launch_info(), group_occupancy() of both
forms, the counter slots, the set and room counts and, after reset() and step(3) (n > 1: the
sharded path where the plan has shards), a sha256 over the state, the episodes and the counters.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 42
KEYS = ("k_S", "k_D", "diffuse", "decay", "n_agents")
SETS5 = ((3, 1, 0.2, 0.2, 32), (0.5, 0, 0.2, 0.2, 5), (10, 2.5, 0.05, 0.6, 17), (1.5, 1, 0.5, 0.1, 1),
         (1, 4, 0.3, 0.3, 24))
SWITCHES = ("FFM_STEP_SHARDS", "FFM_WAVE_BLOCKS", "FFM_GROUP_ENVS", "FFM_GROUP_ONE", "FFM_RESET_CANDIDATES")


def rooms12():
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


def rooms16():
    from ffm_amd.data import make_room, l1_sff
    return [(m, l1_sff(m)) for m in (make_room(16, 16), make_room(16, 16, exit_pos=(0, 4), exit_width=2))]


def rooms20():
    from ffm_amd.data import geodesic_sff, make_room, l1_sff
    p20b = make_room(20, 20)
    p20b[4, 5:16] = 2                       # a barrier in front of the exit: a trap under l1_sff
    return [(m, l1_sff(m)) for m in (make_room(20, 20), make_room(20, 20, exit_pos=(0, 8), exit_width=4))] + \
           [(p20b, geodesic_sff(p20b))]


# name: rooms, agent capacity, create-time n_agents, envs, the switch set around the create call
ENGINES = {
    "group": (rooms12, 32, 32, 135, {}),
    "group_shards2": (rooms12, 32, 32, 135, {"FFM_STEP_SHARDS": "2"}),
    "group_loop": (rooms12, 32, 32, 135, {"FFM_GROUP_ONE": "0"}),
    "lane": (rooms16, 32, 32, 9, {}),
    "wave": (rooms12, 40, 32, 5, {}),
    "block": (rooms20, 32, 12, 13, {}),
}
# (state, parameter sets: on / off / None = untouched, its kernel, rooms: on / off / None, their kernel)
GROUP_WALK = (
    ("params on", True, None, None, None),
    ("params kernel=group", True, "group", None, None),
    ("rooms on with params on", None, None, True, None),
    ("rooms off", None, None, False, None),
    ("params off", False, None, None, None),
    ("rooms on kernel=group", None, None, True, "group"),
    ("params on kernel=group with rooms on", True, "group", None, None),
    ("rooms off again", None, None, False, None),
    ("params kernel=lane", True, "lane", None, None),
    ("params off again", False, None, None, None),
)


def other_walk(room_kernel):
    return (("params on", True, None, None, None), ("params off", False, None, None, None),
            ("rooms on", None, None, True, room_kernel), ("rooms off", None, None, False, None))


WALKS = {"group": GROUP_WALK, "group_shards2": GROUP_WALK, "group_loop": GROUP_WALK, "lane": other_walk(None),
         "wave": other_walk("block"), "block": other_walk("block")}


@contextlib.contextmanager
def switches(**on):
    """The engine's environment switches: all unset but those given, restored on exit."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(on)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class _Dev:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i4", "data": (int(ptr), False),
                                         "version": 3, "strides": None}


def _state(eng):
    import torch
    info = eng.launch_info()
    info.pop("field_stats", None)    # the observer's settings are no part of a step plan (off throughout the walk)
    info.pop("exit_flow", None)      # nor are the exit flow's
    rec = {"launch_info": info, "occupancy_one": eng.group_occupancy(True), "occupancy_loop": eng.group_occupancy(False),
           "counter_slots": int(eng.device_buffers()["counter_slots"]), "sets": len(eng.env_params()[0]),
           "rooms": info["env_rooms"]}
    eng.reset()
    eng.step(3)
    pos, cnt, dff = eng.get_state()
    torch.cuda.synchronize()
    eps = torch.as_tensor(_Dev(eng.device_buffers()["episodes"], eng.n_envs), device=f"cuda:{eng.device}").cpu().numpy()
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(cnt, np.int32).tobytes())
    for e in range(eng.n_envs):                          # the live positions only
        h.update(np.ascontiguousarray(pos[e, :cnt[e]], np.uint16).tobytes())
    h.update(np.ascontiguousarray(dff, np.float32).tobytes())
    h.update(np.ascontiguousarray(eps, np.int32).tobytes())
    h.update(json.dumps(eng.counters(), sort_keys=True).encode())
    rec["sha256"] = h.hexdigest()
    return rec


def walk(name):
    """The recorded states of one engine's walk: [(state, record)], "created" first."""
    import torch
    from ffm_amd.engine import Engine
    torch.cuda.init()                                    # before the library opens the device, as the tests do
    make_rooms, A, N, E, at_create = ENGINES[name]
    rooms = make_rooms()
    sets = [dict(zip(KEYS, s[:4] + (min(s[4], A),))) for s in SETS5]
    params = {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}
    with switches(**at_create):
        eng = Engine(rooms[0][0], rooms[0][1], n_envs=E, n_agents=N, agent_capacity=A, params=params, seed=SEED,
                     auto_reset=True)
    out = []
    try:
        with switches():
            out.append(["created", _state(eng)])
            for state, pep, pep_kernel, room, room_kernel in WALKS[name]:
                if pep is not None:
                    eng.set_env_params(sets if pep else None, kernel=pep_kernel)
                if room is not None:
                    eng.set_env_rooms(rooms if room else None, kernel=room_kernel)
                out.append([state, _state(eng)])
    finally:
        eng.close()
    return out


def run():
    return {name: walk(name) for name in ENGINES}


def differences(got, want):
    """Readable differences between two results of run() (lists after a JSON round trip)."""
    diffs = []
    for name in want:
        for (state, w), (_, g) in zip(want[name], got[name]):
            for k in w:
                if g[k] != w[k]:
                    diffs.append(f"{name} / {state} / {k}: {g[k]} != {w[k]}")
        if len(got[name]) != len(want[name]):
            diffs.append(f"{name}: {len(got[name])} states != {len(want[name])}")
    return diffs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", metavar="FILE")
    ap.add_argument("--check", metavar="FILE")
    ap.add_argument("--commit", default="", help="the commit the library was built from (noted in the file)")
    a = ap.parse_args()
    got = json.loads(json.dumps(run()))
    if a.check:
        with open(a.check) as f:
            diffs = differences(got, json.load(f)["walks"])
        print("\n".join(diffs) if diffs else "step plan walk: equal")
        sys.exit(1 if diffs else 0)
    doc = {"recorded_from": a.commit, "walks": got}
    text = json.dumps(doc, indent=1, sort_keys=True)
    if a.record:
        with open(a.record, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
