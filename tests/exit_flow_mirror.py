"""The oracle mirror of the exit flow (ffm_engine_set_exit_flow): what tests/test_gpu_exit_flow.py
compares the device's arrays against, and what tests/test_exit_flow_mirror.py pins without a GPU.

The oracle.Cores are stepped env by env from reset_philox(N, seed, t0, e) with start[e] = t0, as
the field statistics' mirror does: start[e] is set again at every placement (the auto-reset, seen
by `eps`; reset_envs, which consumes a step index), ("on",) sets start to t - 1.  The positions
before every step are kept, and the leavers of an env-step are found by a method that is not the
kernel's set rule, the sequential order-preserving walk over P (n0 agents, before) and P' (n
agents, after):
  agent i with a door stayed iff j < n and P'[j] == P[i] (then j += 1), else it left;
  an agent without a door is matched to P'[j], which must lie within one neighbourhood move;
  at the end j == n and the leavers number n0 - n.
An emptied or re-placed env: all leave, and each must have a door.  door_from is NumPy over the map.
An event adds exited[c][door] and outflow[c][door][min(tau, bins - 1)] with tau = t - start[e]
before the step (mod 2^32).
"""
import functools

import numpy as np

import env_sweep_util as U
from env_sweep_util import SEED

BINS = 16
PAR = (3, 1, 0.2, 0.2)
M32 = 0xFFFFFFFF
NEIGHBOURS = {      # the reference's neighbour order (model/ffm_core.py:28-34), (d row, d col)
    "neumann": ((-1, 0), (1, 0), (0, -1), (0, 1)),
    "moore": ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)),
}


def three(H, W):
    """make_room(H, W) plus exits at (H - 1, 3) and (5, 0): three doors."""
    from ffm_amd.data import make_room
    m = make_room(H, W)
    m[H - 1, 3] = 3
    m[5, 0] = 3
    return m


def _map(name):
    from ffm_amd.data import make_room
    if name == "T12":
        return three(12, 12)
    if name == "T14":
        return three(14, 14)
    if name in ("X1", "X2", "X3", "X4"):          # 12x12, 1 .. 4 exit cells (X4: the 4-wide exit at (0, 4))
        return make_room(12, 12, exit_pos=(0, 4), exit_width=int(name[1]))
    if name in ("Y1", "Y2", "Y3", "Y4"):
        return make_room(14, 14, exit_pos=(0, 5), exit_width=int(name[1]))
    if name == "R64":
        return make_room(64, 64)
    raise KeyError(name)


room = U.rooms(_map)


def cls3(E):
    return tuple(e % 3 for e in range(E))


def default_doors(m):
    """[H, W] int32: a room's exit cells numbered in row-major order, -1 elsewhere."""
    ex = (np.asarray(m) == 3)
    return np.where(ex, np.cumsum(ex.reshape(-1)).reshape(ex.shape) - 1, -1).astype(np.int32)


def door_from(m, doors, nbh):
    """[H, W] int32: for a free cell the door of the first exit cell among its neighbours in
    neighbour order, -1 for none (and for every cell that is not free)."""
    m = np.asarray(m)
    H, W = m.shape
    lab = np.full((H + 2, W + 2), -1, np.int32)
    lab[1:-1, 1:-1] = np.where(m == 3, doors, -1)
    out = np.full((H, W), -1, np.int32)
    for dx, dy in NEIGHBOURS[nbh]:
        cand = lab[1 + dx:1 + dx + H, 1 + dy:1 + dy + W]
        out = np.where((out < 0) & (cand >= 0), cand, out)
    return np.where(m == 0, out, -1).astype(np.int32)


def _one_move(a, b, W, nbh):
    dx, dy = abs(int(a) // W - int(b) // W), abs(int(a) % W - int(b) % W)
    return dx + dy <= 1 if nbh == "neumann" else max(dx, dy) <= 1


def leavers(P, Pn, dfrom, W, nbh, emptied):
    """Indices into P of the agents that left, by the sequential walk."""
    if emptied:
        assert all(dfrom[c] >= 0 for c in P), "an emptied env held an agent without a door"
        return list(range(len(P)))
    out, j, n = [], 0, len(Pn)
    for i, c in enumerate(P):
        if dfrom[c] >= 0:
            if j < n and Pn[j] == c:
                j += 1
            else:
                out.append(i)
        else:
            assert j < n and _one_move(c, Pn[j], W, nbh), "an agent without a door has no successor"
            j += 1
    assert j == n and len(out) == len(P) - n
    return out


# ---------------------------------------------------------------------------
# rooms: names; roe / soe: per-env room / set indices; sets: (k_S, k_D, diffuse, decay, N) tuples;
# cls: per-env classes; labels: None (default doors) or one tuple of H * W labels per room.
# ops: ("step", n) | ("reset_envs", mask tuple) | ("set_state", cells per env) | ("on",) | ("mark",).
# Returns (windows, eps, doors): per window between marks a dict of exited [C, D], outflow
# [C, D, bins] and the counts the vacuity checks read; doors [R, H, W].
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow(rooms, roe, A, nbh, sets, soe, ops, cls, C, auto=True, t0=0, bins=BINS, labels=None):
    from oracle import oracle as O
    E = len(roe)
    H, W = room(rooms[0])[0].shape
    cores = {}

    def core(e):
        key = (rooms[roe[e]], sets[soe[e]][:4])
        if key not in cores:
            m, s = room(key[0])
            cores[key] = O.Core(np.array(m), np.array(s), U._params(key[1], nbh))
        return cores[key]

    doors = np.stack([default_doors(room(r)[0]) if labels is None else
                      np.where(room(r)[0] == 3, np.asarray(labels[k], np.int32).reshape(H, W), -1).astype(np.int32)
                      for k, r in enumerate(rooms)])
    D = max(1, int(doors.max()) + 1)
    dfrom = [door_from(room(r)[0], doors[k], nbh).reshape(-1) for k, r in enumerate(rooms)]

    N = [sets[soe[e]][4] for e in range(E)]
    pos = np.full((E, A), 0xFFFF, np.uint16)
    cnt = np.zeros(E, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    for e in range(E):
        pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, t0 & M32, e)
        cnt[e] = N[e]
    start = np.full(E, t0 & M32, np.int64)
    t = t0 + 1

    def fresh():
        return {"exited": np.zeros((C, D), np.uint64), "outflow": np.zeros((C, D, bins), np.uint64), "events": 0,
                "multi": 0, "in_replace": 0, "clamped": 0, "tau1": 0, "idx64": 0, "before_wrap": 0, "after_wrap": 0}

    windows, cur = [], fresh()
    for op in ops:
        if op[0] == "step":
            for _ in range(op[1]):
                for e in range(E):
                    k0, n0 = int(eps[e]), int(cnt[e])
                    P = pos[e, :n0].astype(np.int64)
                    core(e).step_philox_batch(pos[e:e + 1], cnt[e:e + 1], dff[e:e + 1], eps[e:e + 1], SEED, t & M32,
                                              auto, N[e], e, 1)
                    replaced = eps[e] != k0
                    n = int(cnt[e])
                    gone = leavers(P, pos[e, :n].astype(np.int64), dfrom[roe[e]], W, nbh,
                                   n0 > 0 and (replaced or n == 0))
                    tau = ((t & M32) - int(start[e])) & M32
                    for i in gone:
                        d = int(dfrom[roe[e]][P[i]])
                        cur["exited"][cls[e], d] += np.uint64(1)
                        if bins:
                            cur["outflow"][cls[e], d, min(tau, bins - 1)] += np.uint64(1)
                    k = len(gone)
                    cur["events"] += k
                    cur["multi"] += k >= 2
                    cur["in_replace"] += k if replaced else 0
                    cur["clamped"] += k if bins and tau > bins - 1 else 0
                    cur["tau1"] += k if tau == 1 else 0
                    cur["idx64"] += sum(i >= 64 for i in gone)
                    cur["before_wrap" if t <= M32 else "after_wrap"] += k
                    if replaced:
                        start[e] = t & M32
                t += 1
        elif op[0] == "reset_envs":
            for e in np.flatnonzero(np.asarray(op[1])):
                pos[e] = 0xFFFF
                pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, t & M32, e)
                cnt[e] = N[e]
                dff[e] = 0.0
                start[e] = t & M32
            t += 1
        elif op[0] == "set_state":                       # positions and counts of every env; ep_start stays
            for e in range(E):
                cells = op[1][e]
                pos[e] = 0xFFFF
                pos[e, :len(cells)] = cells
                cnt[e] = len(cells)
        elif op[0] == "on":
            start[:] = (t - 1) & M32
        elif op[0] == "mark":
            windows.append(cur)
            cur = fresh()
        else:
            raise ValueError(op)
    windows.append(cur)
    for w in windows:
        w["exited"].setflags(write=False)
        w["outflow"].setflags(write=False)
    eps.setflags(write=False)
    doors.setflags(write=False)
    return tuple(windows), eps, doors


# name: room, A, N, E, T, envs_per_block, the create-time kernel (the field statistics' engines, in three(H, W))
ENGINES = {
    "group": ("T12", 32, 32, 37, 300, 0, "group"),
    "lane": ("T12", 32, 32, 37, 300, -2, "lane"),
    "wave": ("T12", 40, 40, 13, 400, 0, "wave"),
    "wave_odd": ("T12", 35, 33, 13, 400, 0, "wave"),
    "block": ("T14", 16, 10, 19, 200, 0, "block"),
}


def plain(name, nbh, ops=None, auto=True, t0=0, E=None):
    """The mirror of an engine of ENGINES under ops (default: T steps); classes e % 3, BINS bins."""
    rm, A, N, E0, T, _, _ = ENGINES[name]
    E = E or E0
    ops = ops or (("step", T),)
    return flow((rm,), (0,) * E, A, nbh, (PAR + (N,),), (0,) * E, ops, cls3(E), 3, auto, t0)


def assert_not_vacuous(w, eps, auto=True):
    assert (w["exited"] > 0).all(), "mirror: a (class, door) without events"
    assert w["multi"] > 0, "mirror: no env-step with two or more leavers"
    assert w["clamped"] > 0, "mirror: nothing clamped into the last bin"
    if auto:
        assert w["in_replace"] > 0, "mirror: no event in a re-placing step"
        assert (eps >= 2).all(), "mirror: an env finished fewer than two episodes"


RING_EXIT = (0, 6)        # make_room(12, 12)'s exit, one of three(12, 12)'s


def ring_state(E, A):
    """A ring of agents around the exit at (0, 6) of three(12, 12) -- (1, 5), (1, 6), (1, 7) --
    and two more further in; env e holds the first 2 + e % 4 of them."""
    cells = [1 * 12 + 6, 1 * 12 + 5, 1 * 12 + 7, 2 * 12 + 6, 6 * 12 + 6]
    return tuple(tuple(cells[:2 + e % 4]) for e in range(E))
