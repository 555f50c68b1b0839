"""Helpers of the per-env sweep tests (test_gpu_env_rooms*.py; the textually equal ones also serve
test_gpu_env_params.py): named rooms, the oracle mirror of an engine with per-env rooms and
parameter sets, engine construction, snapshots and the comparisons.  Every file keeps its own room
table, cases and tests, and binds its `_room` to the helpers that need one.
"""
import functools

import numpy as np

SEED = 42
CREATE = (3, 1, 0.2, 0.2, 3)          # the create-time parameters (k_S, k_D, diffuse, decay, N)
KEYS = ("k_S", "k_D", "diffuse", "decay", "n_agents")
# the sets of tests/test_gpu_env_params.py
SETS5 = ((3, 1, 0.2, 0.2, 32), (0.5, 0, 0.2, 0.2, 5), (10, 2.5, 0.05, 0.6, 17), (1.5, 1, 0.5, 0.1, 1),
         (1, 4, 0.3, 0.3, 24))


def rooms(build, geodesic=()):
    """`_room(name)` -> (map, float32 SFF), cached and read-only, over a file's table `build(name)`
    -> map: the L1 field, or for the names in `geodesic` (a room with an obstacle in the way) its
    geodesic_sff (the default, Neumann, field under both neighbourhoods)."""
    @functools.lru_cache(maxsize=None)
    def _room(name):
        from ffm_amd.data import geodesic_sff, l1_sff
        m = build(name)
        s = geodesic_sff(m) if name in geodesic else l1_sff(m)
        m.setflags(write=False)
        s.setflags(write=False)
        return m, s
    return _room


def _params(s, nbh):
    return {"k_S": s[0], "k_D": s[1], "diffuse": s[2], "decay": s[3], "neighborhood": nbh}


def _dicts(sets):
    return [dict(zip(KEYS, s)) for s in sets]


def _episodes(eng):
    import torch
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


# ---------------------------------------------------------------------------
# The oracle mirror: one Core per (room, set), one env per call.
# room: the file's _room; rooms: room names; roe / soe: per-env indices (tuples); sets: parameter
# sets, or None (`create`, the create-time parameters and N).
# ops: ("step", n) | ("snap",) | ("reset_envs", mask tuple) | ("drain",) | ("rooms", roe tuple)
# sel: envs whose trajectory rows are mirrored.  Returns the snapshots, the episode records and,
# per ("drain",), the rows {(env, k): (steps, [positions])} since the drain before.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(room, A, nbh, rooms, roe, sets, soe, ops, sel=(), create=CREATE):
    from oracle import oracle as O
    E = len(roe)
    H, W = room(rooms[0])[0].shape
    sets = sets or (create,)
    soe = soe or (0,) * E
    roe = list(roe)
    cores = {}

    def core(e):
        key = (rooms[roe[e]], sets[soe[e]][:4])
        if key not in cores:
            m, s = room(key[0])
            cores[key] = O.Core(np.array(m), np.array(s), _params(key[1], nbh))
        return cores[key]

    N = [sets[soe[e]][4] for e in range(E)]
    pos = np.full((E, A), 0xFFFF, np.uint16)
    cnt = np.zeros(E, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    for e in range(E):                                   # reset(): placement keyed t = 0
        pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, 0, e)
        cnt[e] = N[e]
    start = np.zeros(E, np.int64)
    insteps = {e: 0 for e in sel}
    rows, drains = {}, []
    agent_steps, t, snaps, recs = 0, 1, [], []
    for op in ops:
        if op[0] == "step":
            for _ in range(op[1]):
                agent_steps += int(cnt.sum())
                for e in range(E):
                    k0 = int(eps[e])
                    core(e).step_philox_batch(pos[e:e + 1], cnt[e:e + 1], dff[e:e + 1], eps[e:e + 1], SEED, t, True,
                                              N[e], e, 1)
                    ended = eps[e] != k0
                    if ended:
                        recs.append((e, k0, t - start[e], t))
                        start[e] = t
                    if e in insteps:                      # the row after this step (an ended episode: the empty row)
                        insteps[e] += 1
                        st, ps = rows.setdefault((e, k0), ([], []))
                        st.append(insteps[e])
                        cc = np.zeros(0, np.int32) if ended else pos[e, :cnt[e]].astype(np.int32)
                        ps.append(np.stack([cc // W, cc % W], axis=1))
                        if ended:
                            insteps[e] = 0
                t += 1
        elif op[0] == "snap":
            snaps.append({"pos": pos.copy(), "cnt": cnt.copy(), "dff": dff.copy(), "eps": eps.copy(),
                          "agent_steps": agent_steps, "resets": int(eps.sum())})
        elif op[0] == "reset_envs":                      # placed with index t, which advances
            for e in np.flatnonzero(np.asarray(op[1])):
                pos[e] = 0xFFFF
                pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, t, e)
                cnt[e] = N[e]
                dff[e] = 0.0
                start[e] = t
                if e in insteps:
                    insteps[e] = 0
            t += 1
        elif op[0] == "drain":
            drains.append(rows)
            rows = {}
        elif op[0] == "rooms":                           # a second set_env_rooms call: the mapping from here on
            roe = list(op[1])                            # (the caller re-places the changed envs next)
        else:
            raise ValueError(op)
    rec = np.asarray(recs, np.int64).reshape(-1, 4)
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))].astype(np.int32)
    for sn in snaps:
        for v in sn.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    rec.setflags(write=False)
    return tuple(snaps), rec, tuple(drains)


def _engine(pair, A, nbh, E, create=CREATE, epb=0, rng="philox", f64=False):
    """An engine created in the room `pair` = (map, sff) with the parameters and N of `create`."""
    from ffm_amd.engine import Engine
    m, s = pair
    return Engine(m, s.astype(np.float64) if f64 else s, n_envs=E, n_agents=create[4], agent_capacity=A,
                  params=_params(create, nbh), rng=rng, seed=SEED, auto_reset=True, envs_per_block=epb)


def _snapshot(eng):
    pos, cnt, dff = eng.get_state()
    c = eng.counters()
    return {"pos": pos, "cnt": cnt, "dff": dff, "eps": _episodes(eng), "agent_steps": c["agent_steps"],
            "resets": c["resets"]}


def _assert_same(got, want, what="", counters=True):
    assert np.array_equal(got["cnt"], want["cnt"]), f"{what}: counts differ"
    assert np.array_equal(got["eps"], want["eps"]), f"{what}: episodes differ"
    for e in range(len(want["cnt"])):
        n = want["cnt"][e]
        assert np.array_equal(got["pos"][e, :n], want["pos"][e, :n]), f"{what}: positions differ (env {e})"
    assert np.array_equal(got["dff"].view(np.uint32), want["dff"].view(np.uint32)), f"{what}: DFF bits differ"
    if counters:
        assert got["agent_steps"] == want["agent_steps"], f"{what}: agent_steps"
        assert got["resets"] == want["resets"], f"{what}: resets"


def _assert_on(eng, n_rooms, g=None, shards=None, kernel="lane"):
    """Rooms are on, in the form of `kernel` (the group form: its single-group form); g / shards: the
    envs per group and the step shards expected, where the caller pins them."""
    info = eng.launch_info()
    assert info["kernel"] == kernel and info["env_rooms"] == n_rooms
    if kernel == "group":
        assert info["group_one"]
    if g is not None:
        assert info["group_g"] == g
    if shards is not None:
        assert info["step_shards"] == shards
    return info


def _assert_coverage(eps, roe, n_rooms):
    """Every room's own free list and F was placed from: an env of each ended an episode."""
    roe = np.asarray(roe)
    for r in range(n_rooms):
        assert (eps[roe == r] > 0).any(), f"oracle: no env of room {r} ended an episode"
