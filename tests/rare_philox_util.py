"""Helpers of the rare-Philox tests (test_rare_philox_fixtures.py on the CPU, test_gpu_rare_philox.py
on the GPU): the fixtures of tests/golden/rare_philox.json (tools/find_rare_philox.py), the friction
scenario that makes a fixture's draw decide who moves, and an oracle mirror of an engine whose envs
may differ in room, parameters and N.
"""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rare_philox.json")
A = 32                      # agent capacity of every 12x12 case
TARGET = (5, 5)             # the contested interior cell of the friction scenario
PUR_DECIDE, PUR_FRICTION, PUR_RESET = 1, 2, 3
_OFFSETS = {4: [(-1, 0), (1, 0), (0, -1), (0, 1)],
            8: [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]}


@functools.lru_cache(maxsize=None)
def fixtures(kind=None):
    with open(GOLDEN) as f:
        fx = json.load(f)["fixtures"]
    return tuple(x for x in fx if kind is None or x["kind"] == kind)


def fixture(fid):
    (x,) = [x for x in fixtures() if x["id"] == fid]
    return x


def key_of(seed):
    return [seed & 0xFFFFFFFF, seed >> 32]


def placement_keys(fx, F=None):
    """The F placement keys of the fixture's (t, env), by the scalar Philox."""
    from oracle import oracle as O
    F = fx["F"] if F is None else F
    return np.array([int(O.philox([fx["t"], fx["env"], j, PUR_RESET << 28], key_of(fx["seed"]))[0]) for j in range(F)],
                    np.uint64)


# ---------------------------------------------------------------------------
# The friction scenario: a 12x12 room whose SFF is a well (40 everywhere, 0 at TARGET) with k_S = 3,
# k_D = 0: exp(-120) is 0 in float32, so an agent next to TARGET requests it with probability
# exactly 1.  The m requesters are the agents owner .. owner + m - 1, so the requester of rank k is
# agent owner + k; the owner - 1 agents below them stand packed in rows 8 .. 10, which touch neither
# a neighbour of TARGET nor the exit, and so nobody leaves in the first step and indices hold.
# ---------------------------------------------------------------------------
def nbh_of(fx):
    return "neumann" if fx["m"] <= 4 else "moore"


def friction_params(nbh):
    return {"k_S": 3, "k_D": 0, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


@functools.lru_cache(maxsize=None)
def well_room():
    from ffm_amd.data import make_room
    m = make_room(12, 12)
    s = np.full(m.shape, 40.0, np.float32)
    s[TARGET] = 0.0
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


def friction_state(fx):
    """(positions [A] u16, count) of the fixture's env: requesters on m of TARGET's neighbours in a
    shuffled order (so a slot's agent index is not its neighbour index), bystanders below."""
    m, owner = fx["m"], fx["owner"]
    W = 12
    offs = _OFFSETS[4 if m <= 4 else 8]
    order = np.random.default_rng(100 * m + owner).permutation(len(offs))[:m]
    pos = np.full(A, 0xFFFF, np.uint16)
    by = [(8 + i // 10) * W + 1 + i % 10 for i in range(owner)]
    assert owner + m <= A and owner <= 30
    pos[:owner] = by
    for k, o in enumerate(order):
        pos[owner + k] = (TARGET[0] + offs[o][0]) * W + TARGET[1] + offs[o][1]
    return pos, owner + m


def on_target(pos, cnt):
    """Agent indices standing on TARGET."""
    return np.flatnonzero(pos[:cnt] == TARGET[0] * 12 + TARGET[1]).tolist()


# ---------------------------------------------------------------------------
# Oracle mirror: env e steps in cores[e] with its own N[e]; global ids through env_base.
# ---------------------------------------------------------------------------
class Mirror:
    def __init__(self, cores, Ns, seed, env_base, cap=A, auto_reset=True):
        self.cores, self.Ns, self.seed, self.env_base, self.auto_reset = cores, list(Ns), seed, env_base, auto_reset
        E = len(cores)
        H, W = cores[0].H, cores[0].W
        self.pos = np.full((E, cap), 0xFFFF, np.uint16)
        self.cnt = np.zeros(E, np.int32)
        self.dff = np.zeros((E, H, W), np.float32)
        self.eps = np.zeros(E, np.int32)
        self.start = np.zeros(E, np.int64)       # step index (u32) of each env's last placement
        self.records = []                        # (global env, episode, steps, t_end) with u32 wrap
        self.agent_steps = 0
        self.steps = 0

    def reset(self, t):
        """Engine.reset() at step index t: every env placed with keys of t, episodes zeroed."""
        for e, c in enumerate(self.cores):
            self.pos[e] = 0xFFFF
            self.pos[e, :self.Ns[e]] = c.reset_philox(self.Ns[e], self.seed, t & 0xFFFFFFFF, self.env_base + e)
            self.cnt[e] = self.Ns[e]
        self.dff[:] = 0
        self.eps[:] = 0
        self.start[:] = t & 0xFFFFFFFF

    def set_env(self, e, pos, cnt, dff=None):
        self.pos[e] = 0xFFFF
        self.pos[e, :cnt] = pos[:cnt]
        self.cnt[e] = cnt
        self.dff[e] = 0 if dff is None else dff

    def step(self, t0, T):
        for k in range(T):
            t = (t0 + k) & 0xFFFFFFFF
            self.agent_steps += int(self.cnt.sum())
            for e, c in enumerate(self.cores):
                k0 = int(self.eps[e])
                c.step_philox_batch(self.pos[e:e + 1], self.cnt[e:e + 1], self.dff[e:e + 1], self.eps[e:e + 1],
                                    self.seed, t, self.auto_reset, self.Ns[e], self.env_base + e, 1)
                if self.eps[e] != k0:
                    self.records.append((self.env_base + e, k0, (t - self.start[e]) & 0xFFFFFFFF, t))
                    self.start[e] = t
            self.steps += 1


def assert_engine_equals(eng, mir, what=""):
    """Positions of the live agents, counts, DFF bits, episodes and counters, bit for bit."""
    from env_sweep_util import _episodes
    gpos, gcnt, gdff = eng.get_state()
    assert np.array_equal(gcnt, mir.cnt), f"{what}: counts differ in envs {np.flatnonzero(gcnt != mir.cnt).tolist()}"
    for e in range(len(mir.cnt)):
        n = mir.cnt[e]
        assert np.array_equal(gpos[e, :n], mir.pos[e, :n]), f"{what}: positions differ (env {e})"
    bad = np.argwhere(gdff.view(np.uint32) != mir.dff.view(np.uint32))
    assert not bad.size, f"{what}: DFF bits differ at (env, x, y) {bad[:8].tolist()}"
    assert np.array_equal(_episodes(eng), mir.eps), f"{what}: episodes differ"
    c = eng.counters()
    assert c["agent_steps"] == mir.agent_steps, f"{what}: agent_steps"
    assert c["resets"] == int(mir.eps.sum()), f"{what}: resets"
    assert c["steps"] == mir.steps, f"{what}: steps"
