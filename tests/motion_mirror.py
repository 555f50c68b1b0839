"""The oracle mirror of the motion statistics (ffm_engine_set_motion_stats): what
tests/test_gpu_motion_stats.py compares the device's arrays against, and what
tests/test_motion_mirror.py pins without a GPU.

The oracle.Cores are stepped env by env exactly as tests/exit_flow_mirror.py steps them (its rooms,
ENGINES, door_from, leavers and NEIGHBOURS are imported), with start[e] set at every placement and
the positions before every step kept.  The leavers of an env-step come from that mirror's
sequential walk, and the successor of a survivor from a walk of the same kind, not from the
kernel's rank rule: j advances over P' once per survivor of P, in order.  The origins are a Python
list per env, replaced at every placement (the first reset, reset_envs, the auto-reset) and at
("on",), and carried along the successors otherwise.  An env-step with n0 > 0 agents adds, with c
the env's class, tau = t - start[e] before the step (mod 2^32) and b = min(tau, bins - 1):
  flux[c][P[i]][d(i)] += 1, d(i) the neighbour index of the survivor's move (NB: a stay) or of the
  leaver's first exit cell;  present[c][b] += n0;  moved[c][b] += |{i : d(i) != NB}|;
  egress_count[c][origin(i)] += 1 and egress_steps[c][origin(i)] += tau for every leaver.
The exit flow's tables (default doors) are summed in the same pass, for the tests that run both.
"""
import functools

import numpy as np

import env_sweep_util as U
import exit_flow_mirror as X
from env_sweep_util import SEED
from exit_flow_mirror import BINS, ENGINES, M32, NEIGHBOURS, PAR, door_from, leavers, room

__all__ = ["BINS", "ENGINES", "M32", "NEIGHBOURS", "PAR", "dir_from", "motion", "plain", "assert_not_vacuous"]


def dir_from(m, nbh):
    """[H, W] int32: for a free cell the index, in neighbour order, of the first exit cell among its
    neighbours, -1 for none (and for every cell that is not free)."""
    m = np.asarray(m)
    H, W = m.shape
    ex = np.zeros((H + 2, W + 2), bool)
    ex[1:-1, 1:-1] = m == 3
    out = np.full((H, W), -1, np.int32)
    for k, (dx, dy) in enumerate(NEIGHBOURS[nbh]):
        cand = ex[1 + dx:1 + dx + H, 1 + dy:1 + dy + W]
        out = np.where((out < 0) & cand, k, out)
    return np.where(m == 0, out, -1).astype(np.int32)


def successors(n0, gone, n):
    """The index in P' of every agent of P (None for a leaver), by the sequential walk."""
    out, j, left = [], 0, set(gone)
    for i in range(n0):
        if i in left:
            out.append(None)
        else:
            out.append(j)
            j += 1
    assert j == n, "the survivors of P do not number the agents of P'"
    return out


# ---------------------------------------------------------------------------
# The arguments of exit_flow_mirror.flow (without labels).  ops: ("step", n) | ("reset_envs", mask
# tuple) | ("set_state", cells per env) | ("on",) (ep_start absent: start = t - 1; origins = the
# positions) | ("on", "keep") (ep_start was there: origins only) | ("mark",).
# Returns (windows, eps, doors): per window between marks a dict of the five tables, the exit
# flow's two, and the counts the vacuity checks read.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def motion(rooms, roe, A, nbh, sets, soe, ops, cls, C, auto=True, t0=0, bins=BINS):
    from oracle import oracle as O
    E = len(roe)
    H, W = room(rooms[0])[0].shape
    nb = NEIGHBOURS[nbh]
    NB = len(nb)
    code = {d: k for k, d in enumerate(nb)}
    code[(0, 0)] = NB
    cores = {}

    def core(e):
        key = (rooms[roe[e]], sets[soe[e]][:4])
        if key not in cores:
            m, s = room(key[0])
            cores[key] = O.Core(np.array(m), np.array(s), U._params(key[1], nbh))
        return cores[key]

    doors = np.stack([X.default_doors(room(r)[0]) for r in rooms])
    D = max(1, int(doors.max()) + 1)
    dfrom = [door_from(room(r)[0], doors[k], nbh).reshape(-1) for k, r in enumerate(rooms)]
    dirf = [dir_from(room(r)[0], nbh).reshape(-1) for r in rooms]

    N = [sets[soe[e]][4] for e in range(E)]
    pos = np.full((E, A), 0xFFFF, np.uint16)
    cnt = np.zeros(E, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    for e in range(E):
        pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, t0 & M32, e)
        cnt[e] = N[e]
    origin = [[int(c) for c in pos[e, :cnt[e]]] for e in range(E)]
    start = np.full(E, t0 & M32, np.int64)
    unseen = [True] * E                                  # placed, and not stepped since
    t = t0 + 1

    def fresh():
        return {"flux": np.zeros((C, H, W, NB + 1), np.uint64), "present": np.zeros((C, bins), np.uint64),
                "moved": np.zeros((C, bins), np.uint64), "egress_count": np.zeros((C, H, W), np.uint64),
                "egress_steps": np.zeros((C, H, W), np.uint64),
                "exited": np.zeros((C, D), np.uint64), "outflow": np.zeros((C, D, bins), np.uint64),
                "events": 0, "multi": 0, "in_replace": 0, "clamped": 0, "tau1": 0, "shifted": 0, "chunk_shift": 0,
                "late_first": 0, "before_wrap": 0, "after_wrap": 0}

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
                    if n0 == 0:
                        continue
                    emptied = replaced or n == 0
                    Pn = pos[e, :n].astype(np.int64)
                    gone = leavers(P, Pn, dfrom[roe[e]], W, nbh, emptied)
                    succ = successors(n0, gone, 0 if emptied else n)
                    tau = ((t & M32) - int(start[e])) & M32
                    c, b = cls[e], min(tau, bins - 1)
                    moved, carried = 0, [None] * (0 if emptied else n)
                    for i in range(n0):
                        x, y = divmod(int(P[i]), W)
                        if succ[i] is None:
                            d = int(dirf[roe[e]][P[i]])
                            assert 0 <= d < NB, "a leaver without an exit among its neighbours"
                            o = origin[e][i]
                            cur["egress_count"][c, o // W, o % W] += np.uint64(1)
                            cur["egress_steps"][c, o // W, o % W] += np.uint64(tau)
                            door = int(dfrom[roe[e]][P[i]])
                            cur["exited"][c, door] += np.uint64(1)
                            if bins:
                                cur["outflow"][c, door, b] += np.uint64(1)
                        else:
                            u, v = divmod(int(Pn[succ[i]]), W)
                            d = code[(u - x, v - y)]           # KeyError: no neighbour move
                            carried[succ[i]] = origin[e][i]
                            cur["shifted"] += succ[i] != i
                            cur["chunk_shift"] += i >= 64 and any(g < (i // 64) * 64 for g in gone)
                        cur["flux"][c, x, y, d] += np.uint64(1)
                        moved += d != NB
                    if bins:
                        cur["present"][c, b] += np.uint64(n0)
                        cur["moved"][c, b] += np.uint64(moved)
                    k = len(gone)
                    cur["events"] += k
                    cur["multi"] += k >= 2
                    cur["in_replace"] += k if replaced else 0
                    cur["clamped"] += n0 if bins and tau > bins - 1 else 0
                    cur["tau1"] += k if tau == 1 else 0
                    cur["late_first"] += k if unseen[e] and tau != 1 else 0     # (reset_envs consumed an index between)
                    unseen[e] = bool(replaced)
                    cur["before_wrap" if t <= M32 else "after_wrap"] += k
                    if replaced:
                        start[e] = t & M32
                        origin[e] = [int(x) for x in Pn]
                    else:
                        origin[e] = carried
                t += 1
        elif op[0] == "reset_envs":
            for e in np.flatnonzero(np.asarray(op[1])):
                pos[e] = 0xFFFF
                pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, t & M32, e)
                cnt[e] = N[e]
                dff[e] = 0.0
                start[e] = t & M32
                origin[e] = [int(x) for x in pos[e, :cnt[e]]]
                unseen[e] = True
            t += 1
        elif op[0] == "set_state":                       # positions and counts of every env; ep_start stays
            for e in range(E):                           # (the origins are undefined from here: the cells, say)
                cells = op[1][e]
                pos[e] = 0xFFFF
                pos[e, :len(cells)] = cells
                cnt[e] = len(cells)
                origin[e] = [int(x) for x in cells]
        elif op[0] == "on":
            if op[1:] != ("keep",):
                start[:] = (t - 1) & M32
            origin = [[int(x) for x in pos[e, :cnt[e]]] for e in range(E)]
        elif op[0] == "mark":
            windows.append(cur)
            cur = fresh()
        else:
            raise ValueError(op)
    windows.append(cur)
    for w in windows:
        for k in TABLES + ("exited", "outflow"):
            w[k].setflags(write=False)
    eps.setflags(write=False)
    doors.setflags(write=False)
    return tuple(windows), eps, doors


TABLES = ("flux", "present", "moved", "egress_count", "egress_steps")


def plain(name, nbh, ops=None, auto=True, t0=0, E=None):
    """The mirror of an engine of ENGINES under ops (default: T steps); classes e % 3, BINS bins."""
    rm, A, N, E0, T, _, _ = ENGINES[name]
    E = E or E0
    ops = ops or (("step", T),)
    return motion((rm,), (0,) * E, A, nbh, (PAR + (N,),), (0,) * E, ops, X.cls3(E), 3, auto, t0)


def free_cells(name):
    return int((np.asarray(room(name)[0]) == 0).sum())


def assert_identities(w):
    """What holds for the tables of any window."""
    NB = w["flux"].shape[-1] - 1
    if w["present"].shape[1]:
        assert int(w["flux"].sum()) == int(w["present"].sum())
        assert int(w["flux"][..., :NB].sum()) == int(w["moved"].sum())
        assert not w["present"][:, 0].any() and not w["moved"][:, 0].any()      # tau >= 1 always
    assert (w["egress_steps"] >= w["egress_count"]).all()
    assert ((w["egress_count"] == 0) <= (w["egress_steps"] == 0)).all()


def assert_not_vacuous(w, eps, rm, auto=True):
    NB = w["flux"].shape[-1] - 1
    assert (w["flux"].sum(axis=(1, 2)) > 0).all(), "mirror: a (class, direction) without counts"
    assert NB in (4, 8)
    assert w["multi"] > 0, "mirror: no env-step with two or more leavers"
    assert w["clamped"] > 0, "mirror: nothing clamped into the last bin"
    assert w["shifted"] > 0, "mirror: no survivor with a leaver below it"
    if auto:
        assert w["in_replace"] > 0, "mirror: no event in a re-placing step"
        assert (eps >= 2).all(), "mirror: an env finished fewer than two episodes"
        free = free_cells(rm)
        seen = (w["egress_count"] > 0).sum(axis=(1, 2))
        assert (10 * seen >= 9 * free).all(), ("mirror: egress from fewer than 90 % of the free cells", seen, free)
