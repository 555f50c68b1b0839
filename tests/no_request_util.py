"""Helpers of the no-request tests (test_no_request_fixtures.py on the CPU, test_gpu_no_request.py on
the GPU, tests/golden/gen_golden.py and gen_injected.py for the fixtures).

model/ffm_core.py:82 reads `if np.isfinite(probs_sum) and probs_sum != 0:`.  An agent that fails it
makes no request: it takes no draw, stays, and adds nothing to the DFF.  The sum is not finite
whenever a valid candidate's score is (see the three rooms below).  count_branches() counts, from a
state alone and in plain NumPy written like the reference's lines, the agents of a step that take
that branch and, separately, those that take :63 (no free neighbour at all).
"""
import functools

import numpy as np

_OFFSETS = {4: [(-1, 0), (1, 0), (0, -1), (0, 1)],
            8: [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]}
DFF_HUGE = np.float32(3e38)     # k_D = 8 times this overflows float32: +inf - (+inf)
HUGE_CELL = (6, 6)
# floors of no-request agent-steps that every fixture and every Philox case must reach
FLOORS = {"pocket": 1000, "overflow": 1000, "diag": 50}


# ---------------------------------------------------------------------------
# Rooms
# ---------------------------------------------------------------------------
def pocket_map():
    """A 12x12 room with rows 1-2, columns 1-3 walled off: six free cells that reach no exit."""
    from ffm_amd.data import make_room
    m = make_room(12, 12)
    m[3, 1:5] = 2
    m[1:3, 4] = 2
    return m


def diag_map():
    """(5, 5) free between four walls: reachable by diagonal moves only."""
    from ffm_amd.data import make_room
    m = make_room(12, 12)
    for x, y in ((4, 5), (6, 5), (5, 4), (5, 6)):
        m[x, y] = 2
    return m


@functools.lru_cache(maxsize=None)
def pocket_room(nbh="neumann", dtype="float32"):
    """-inf - (-inf): every candidate of an agent in the pocket has SFF inf (k_S = 0: 0 * inf)."""
    from ffm_amd.data import geodesic_sff
    m = pocket_map()
    s = geodesic_sff(m, nbh, np.dtype(dtype).type, unreachable="inf")
    assert np.isinf(s[1:3, 1:4]).all() and (m[1:3, 1:4] == 0).all()
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


@functools.lru_cache(maxsize=None)
def diag_room(dtype="float32"):
    """The Neumann geodesic field of diag_map (inf at (5, 5)) under Moore movement."""
    from ffm_amd.data import geodesic_sff
    m = diag_map()
    s = geodesic_sff(m, "neumann", np.dtype(dtype).type, unreachable="inf")
    assert np.isinf(s[5, 5]) and m[5, 5] == 0
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


def params(nbh, k_S=3, k_D=1):
    return {"k_S": k_S, "k_D": k_D, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


def huge_dff(m):
    d = np.zeros(m.shape, np.float32)
    d[HUGE_CELL] = DFF_HUGE
    return d


def overflow_state(m, nb, on_cell, seed, n=60):
    """(cells [n] u16 in agent order, dff [H, W]): one DFF cell at 3e38, whose product with k_D = 8
    is +inf in float32.  The agents on the cell's nb neighbours have it among their candidates
    (on_cell: one agent stands on it instead, and its own score is +inf): +inf - (+inf), and :82
    fails for them for as long as the cell stays above f32 max / 8.  The other agents stand on
    random free cells; the order is shuffled."""
    W = m.shape[1]
    hx, hy = HUGE_CELL
    first = [(hx, hy)] if on_cell else [(hx + dx, hy + dy) for dx, dy in _OFFSETS[nb]]
    taken = set(first) | {(hx, hy)}
    rest = [(int(x), int(y)) for x, y in np.argwhere(m == 0) if (int(x), int(y)) not in taken]
    rng = np.random.default_rng(seed)
    cells = np.array(first + [rest[i] for i in rng.permutation(len(rest))[:n - len(first)]])
    cells = cells[rng.permutation(len(cells))]
    return (cells[:, 0] * W + cells[:, 1]).astype(np.uint16), huge_dff(m)


# ---------------------------------------------------------------------------
# Who takes :82 and who takes :63, from a state
# ---------------------------------------------------------------------------
def count_branches(m, sff, p, pos, cnt, dff):
    """pos [E, A] cells (x * W + y), cnt [E], dff [E, H, W] float32, before a step.
    Returns (no_request [E], boxed_in [E], nonfinite [E]): per env, the agents that have a free
    unoccupied neighbour, no exit among their candidates and a sum of :81 that fails :82; the agents
    without any free unoccupied neighbour (:63); and the agents that reach :77 with a non-finite
    score among their candidates, whether the sum then fails :82 or not (a -inf beside a finite
    score is a candidate of probability exactly 0, and the sum stays finite)."""
    m = np.asarray(m)
    H, W = m.shape
    E, A = pos.shape
    nb = _OFFSETS[4 if p["neighborhood"] == "neumann" else 8]
    live = np.arange(A)[None, :] < np.asarray(cnt)[:, None]
    cell = np.where(live, pos, W + 1).astype(np.int64)
    x, y = cell // W, cell % W
    assert (x[live] > 0).all() and (x[live] < H - 1).all() and (y[live] > 0).all() and (y[live] < W - 1).all()
    env = np.arange(E)[:, None]
    occ = np.zeros((E, H * W), bool)
    occ[np.broadcast_to(env, cell.shape)[live], cell[live]] = True
    mf = m.reshape(-1)
    sf = np.asarray(sff).reshape(-1)
    df = dff.reshape(E, -1)
    cand = np.stack([cell + dx * W + dy for dx, dy in nb] + [cell], axis=-1)              # [E, A, NB + 1], stay last
    walk = (mf[cand] == 0) | (mf[cand] == 3)                                              # :52-54
    valid = walk & ~occ[env[:, :, None], cand]                                            # :57-60
    valid[..., -1] = True                                                                 # :64
    free = valid[..., :-1].any(-1)                                                        # :63
    to_exit = (valid & (mf[cand] == 3)).any(-1)                                           # :66-72
    with np.errstate(all="ignore"):
        score = -p["k_S"] * sf[cand] + p["k_D"] * df[env[:, :, None], cand]               # :77
        assert score.dtype == (np.float32 if sf.dtype == np.float32 else np.float64)
        mx = np.max(np.where(valid, score, -np.inf), axis=-1, keepdims=True)              # :78
        probs = np.where(valid, np.exp(score - mx), 0)                                    # :80
        tot = probs.sum(-1)                                                               # :81
    fails = ~(np.isfinite(tot) & (tot != 0))                                              # :82
    scored = live & free & ~to_exit
    return (scored & fails).sum(1), (live & ~free).sum(1), (scored & (valid & ~np.isfinite(score)).any(-1)).sum(1)


def count_mirror(mir, t0, T):
    """Step a rare_philox_util.Mirror T times from step index t0, counting before every step.
    Returns the three sums of count_branches over the whole run, in agent-steps."""
    groups = {}
    for e, c in enumerate(mir.cores):
        groups.setdefault(id(c), (c, []))[1].append(e)
    tot = np.zeros(3, np.int64)
    for k in range(T):
        for c, es in groups.values():
            tot += [int(x.sum()) for x in count_branches(c.map, c.sff32 if c.sff32 is not None else c.sff64,
                                                          c.params, mir.pos[es], mir.cnt[es], mir.dff[es])]
        mir.step(t0 + k, 1)
    return tuple(int(x) for x in tot)


def count_replay_mt(core, N, seeds, T, pos0=None, dff0=None):
    """The reference's MT episodes restated by the oracle (as tests/test_oracle.py replays them), counted:
    placement by seed (or pos0 / dff0 injected), at most T steps each."""
    from oracle import oracle as O
    sff = core.sff32 if core.sff32 is not None else core.sff64
    tot = np.zeros(3, np.int64)
    for seed in seeds:
        np_rng, py_rng = O.seeded_np(seed), O.seeded_py(seed)
        if pos0 is None:
            pos = core.init_agents_mt(N, np_rng)
            dff = np.zeros(core.map.shape, np.float32)
        else:
            pos, dff = np.asarray(pos0, np.int32), np.array(dff0, np.float32)
        for _ in range(T):
            if not len(pos):
                break
            tot += [int(x[0]) for x in count_branches(core.map, sff, core.params, pos[None], np.array([len(pos)]),
                                                      dff[None])]
            pos = core.step_mt(pos, dff, np_rng, py_rng)
    return tuple(int(x) for x in tot)
