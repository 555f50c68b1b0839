"""Per-env rooms on the block kernel (Engine.set_env_rooms(..., kernel="block") /
ffm_engine_set_env_rooms_kernel): geometry sweeps for rooms beyond the lane kernel's shapes.

The contract is that of tests/test_gpu_env_rooms.py: env e of an engine with
per-env rooms evolves bit for bit like the env with the same global id of a homogeneous engine
created with that room's map and SFF (and, with per-env parameters on as well, that env's set).
The expected state comes from the oracle, one env at a time (the helpers of tests/env_sweep_util.py,
with the create-time N a parameter).  Every case asserts the
create-time launch_info()["kernel"], then kernel == "block" and env_rooms == R while the form is on,
before it compares anything; every auto-reset case asserts from the oracle's result that every room
completed an episode, so every room's own F and free list was placed from inside the step kernel.

An LDS refusal caused by a room's F: no such shape exists.  F enters the block kernel's LDS only
through the placement keys (8 * min(F, 2A + 16 + 8 ceil(sqrt(2A + 16)) + 64) bytes), and the keys
share the bytes of the arrays that are dead by then (grid, positions, requests, draws:
K * (2 PHW + 14 A) bytes); the carve grows with F only where the keys outgrow those arrays, which
needs A + 32 sqrt(2A) > PHW - 320 at K = 1 and is impossible at K >= 2 beyond toy maps.  At K = 1
and an LDS near 64 KB (PHW >= 5,461) that takes A >= 2,800, whose arrays alone pass 64 KB: such an
engine is block_scratch and refused for that.  What can pass 64 KB is the K * 36 bytes of records
and room indices on an engine whose K was forced (envs_per_block) to fill the LDS: the "lds" case.
"""
import functools

import numpy as np
import pytest

import env_sweep_util as U
from env_sweep_util import SETS5, _assert_coverage, _assert_same, _dicts, _snapshot

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAR = (3, 1, 0.2, 0.2)                  # the create-time parameters (k_S, k_D, diffuse, decay)
NBHS = ("neumann", "moore")

# name: rooms, A, N, E, T, the create-time kernel, the first step by which every room has completed an
# episode and the episodes per room at T (the oracle's; Neumann, Moore)
CASES = {
    "wave12": dict(rooms=("R0", "R1", "R2", "R3"), A=40, N=40, E=13, T=400, kernel="wave",
                   first=(110, 67), eps=([12, 22, 9, 18], [20, 26, 16, 31])),
    "s14": dict(rooms=("P14", "P14W", "P14S"), A=16, N=10, E=19, T=200, kernel="block",
                first=(27, 15), eps=([48, 62, 41], [68, 75, 59])),
    "q20": dict(rooms=("P20", "P20W", "P20B"), A=32, N=12, E=13, T=300, kernel="block",
                first=(29, 22), eps=([40, 47, 29], [56, 59, 44])),
    "c64": dict(rooms=("P64", "P64B"), A=300, N=6, E=5, T=400, kernel="block",
                first=(106, 58), eps=([14, 7], [20, 12])),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _map(name):
    """The map of a named room."""
    from ffm_amd.data import make_room
    if name == "R0":
        m = make_room(12, 12)
    elif name == "R1":                       # a 2-wide exit
        m = make_room(12, 12)
        m[0, 5] = 3
    elif name == "R2":                       # a side exit and two pillars: F = 92
        m = make_room(12, 12, exit_pos=(6, 0))
        m[1:3, 9:11] = 2
        m[9:11, 9:11] = 2
    elif name == "R3":                       # a second exit and one pillar: F = 96
        m = make_room(12, 12)
        m[11, 3] = 3
        m[1:3, 1:3] = 2
    elif name == "TINY":                     # two free cells
        m = make_room(12, 12)
        m[1:11, 1:11] = 2
        m[1, 5:7] = 0
    elif name == "P14":
        m = make_room(14, 14)
    elif name == "P14W":
        m = make_room(14, 14, exit_pos=(0, 5), exit_width=2)
    elif name == "P14S":
        m = make_room(14, 14, exit_pos=(7, 0))
        m[2:4, 9:11] = 2
    elif name == "P20":
        m = make_room(20, 20)
    elif name == "P20W":
        m = make_room(20, 20, exit_pos=(0, 8), exit_width=4)
    elif name == "P20B":                     # a barrier in front of the exit: a trap under l1_sff
        m = make_room(20, 20)
        m[4, 5:16] = 2
    elif name == "P64":
        m = make_room(64, 64)
    elif name == "P64B":
        m = make_room(64, 64, exit_pos=(0, 10), exit_width=3)
        m[20:24, 8:14] = 2
    elif name == "P84":
        m = make_room(84, 84)
    elif name == "P84W":
        m = make_room(84, 84, exit_pos=(0, 20), exit_width=2)
        m[30:40, 30:40] = 2
    elif name == "P128":
        m = make_room(128, 128)
    else:
        raise KeyError(name)
    return m


# name -> (map, float32 SFF): the L1 field, or where the room has an obstacle in the way its geodesic_sff
_room = U.rooms(_map, geodesic=("P20B", "P64B"))
# the shared helpers (env_sweep_util.py) over this file's rooms; rooms on: the block kernel, one shard
_assert_on = functools.partial(U._assert_on, kernel="block", shards=1)


def test_room_free_cells():
    assert [int((_room(r)[0] == 0).sum()) for r in CASES["wave12"]["rooms"]] == [100, 100, 92, 96]
    assert int((_room("P84")[0] == 0).sum()) == 6724


def _oracle(A, N0, nbh, rooms, roe, sets, soe, ops, sel=()):
    """The oracle mirror with the create-time N a parameter (sets None: PAR + (N0,))."""
    return U._oracle(_room, A, nbh, rooms, roe, sets, soe, ops, sel, PAR + (N0,))


def _engine(room, A, N, nbh, E, par=PAR, **kw):
    return U._engine(_room(room), A, nbh, E, create=par + (N,), **kw)


def _pairs(rooms, nbh):
    return [_room(r) for r in rooms]


def _room_eps(eps, roe, n_rooms):
    roe = np.asarray(roe)
    return [int(eps[roe == r].sum()) for r in range(n_rooms)]


def _roe(c):
    return tuple(e % len(c["rooms"]) for e in range(c["E"]))


# 1. the four shapes, both neighbourhoods: env e in room e % R
@pytest.mark.parametrize("nbh", NBHS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_rooms_match_oracle(case, nbh):
    c = CASES[case]
    R, roe, ni = len(c["rooms"]), _roe(c), NBHS.index(nbh)
    first, T = c["first"][ni], c["T"]
    at = (1, first - 1, first, T)
    ops, last = [], 0
    for s in at:
        ops += [("step", s - last), ("snap",)]
        last = s
    want, _, _ = _oracle(c["A"], c["N"], nbh, c["rooms"], roe, None, None, tuple(ops))
    # the oracle's own figures: the first step with every room covered, the episodes per room at T
    _assert_coverage(want[2]["eps"], roe, R)
    assert 0 in _room_eps(want[1]["eps"], roe, R)
    assert _room_eps(want[3]["eps"], roe, R) == c["eps"][ni]
    eng = _engine(c["rooms"][0], c["A"], c["N"], nbh, c["E"])
    try:
        created = eng.launch_info()
        assert created["kernel"] == c["kernel"] and created["env_rooms"] == 0
        eng.set_env_rooms(_pairs(c["rooms"], nbh), np.asarray(roe, np.int32), kernel="block")
        info = _assert_on(eng, R)
        assert info["K"] == created["K"] and info["blocks"] == -(-c["E"] // info["K"])   # the create-time K
        assert info["block_size"] == (512 if c["A"] > 256 else 256)
        maps, sffs, got_roe = eng.env_rooms()
        assert np.array_equal(got_roe, np.asarray(roe, np.int32))
        for r, (m, s) in enumerate(_pairs(c["rooms"], nbh)):
            assert np.array_equal(maps[r], m) and np.array_equal(sffs[r].view(np.uint32), s.view(np.uint32))
        eng.reset()
        last = 0
        for s, w in zip(at, want):
            eng.step(s - last)
            last = s
            _assert_same(_snapshot(eng), w, f"{case} {nbh} after {s} steps")
    finally:
        eng.close()


# 2. the large-map reset: F = 6,724 puts the placement on core_block_reset_kernel (10 F + 2 N bytes
#    of the wave reset's LDS pass 64 KB) while the step kernel keeps its state in LDS
def test_large_map_reset():
    rooms, A, N, E, nbh = ("P84", "P84W"), 32, 3, 3, "neumann"
    roe = (0, 1, 0)
    mask = (0, 1, 1)
    ops = (("snap",), ("reset_envs", mask), ("snap",), ("step", 20), ("snap",))
    want, _, _ = _oracle(A, N, nbh, rooms, roe, None, None, ops)
    eng = _engine(rooms[0], A, N, nbh, E)
    try:
        assert eng.launch_info()["kernel"] == "block"
        eng.set_env_rooms(_pairs(rooms, nbh), np.asarray(roe, np.int32), kernel="block")
        _assert_on(eng, 2)
        eng.reset()
        _assert_same(_snapshot(eng), want[0], "reset()")
        eng.reset_envs(np.asarray(mask, np.uint8))
        _assert_same(_snapshot(eng), want[1], "reset_envs")
        eng.step(20)
        _assert_same(_snapshot(eng), want[2], "20 steps")
    finally:
        eng.close()


# 3. crossed with per-env parameters, in either call order
def _capped_sets(c):
    fmin = min(int((_room(r)[0] == 0).sum()) for r in c["rooms"])
    return tuple(s[:4] + (min(s[4], c["A"], fmin),) for s in SETS5)


@pytest.mark.parametrize("order", ["rooms_params", "params_rooms"])
@pytest.mark.parametrize("case", ["wave12", "q20"])
def test_crossed_with_env_params(case, order):
    c = CASES[case]
    nbh, E, T, R = "neumann", 20, 60, len(c["rooms"])
    sets = _capped_sets(c)
    roe = tuple(e % R for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    (want,), _, _ = _oracle(c["A"], sets[0][4], nbh, c["rooms"], roe, sets, soe, (("step", T), ("snap",)))
    _assert_coverage(want["eps"], roe, R)
    eng = _engine(c["rooms"][0], c["A"], sets[0][4], nbh, E, par=sets[0][:4])
    try:
        created = eng.launch_info()
        assert created["kernel"] == c["kernel"]
        if order == "rooms_params":
            eng.set_env_rooms(_pairs(c["rooms"], nbh), np.asarray(roe, np.int32), kernel="block")
            eng.set_env_params(_dicts(sets), np.asarray(soe, np.int32))
        else:
            eng.set_env_params(_dicts(sets), np.asarray(soe, np.int32))
            assert eng.launch_info()["kernel"] == "block"
            eng.set_env_rooms(_pairs(c["rooms"], nbh), np.asarray(roe, np.int32), kernel="block")
        _assert_on(eng, R)
        eng.reset()
        eng.step(T)
        _assert_same(_snapshot(eng), want, f"{case} {order}")
        eng.set_env_rooms(None)
        info = eng.launch_info()
        assert info["env_rooms"] == 0 and eng.env_rooms() is None and info["kernel"] == "block"   # the sets stay on
        assert [s["n_agents"] for s in eng.env_params()[0]] == [s[4] for s in sets]
        eng.set_env_params(None)
        assert eng.launch_info() == created
    finally:
        eng.close()


# 4. masked reset_envs over the envs of one room + the episode log and statistics + trajectory
#    capture of two envs in different rooms
@pytest.mark.parametrize("case", ["wave12", "q20"])
def test_reset_envs_log_and_capture(case):
    c = CASES[case]
    nbh, E, R = "moore", 11, len(c["rooms"])
    roe = tuple(e % R for e in range(E))
    sel = (1, 2)
    n1, n2 = 30, 60
    mask = tuple(1 if roe[e] == 1 else 0 for e in range(E))      # the envs of room 1
    ops = (("step", n1), ("snap",), ("drain",), ("reset_envs", mask), ("step", n2), ("snap",), ("drain",))
    want, rec, drains = _oracle(c["A"], c["N"], nbh, c["rooms"], roe, None, None, ops, sel)
    _assert_coverage(want[-1]["eps"], roe, R)
    eng = _engine(c["rooms"][0], c["A"], c["N"], nbh, E)
    try:
        eng.set_env_rooms(_pairs(c["rooms"], nbh), kernel="block")     # the default mapping: e % R
        _assert_on(eng, R)
        eng.set_episode_log(capacity=E * 64, hist_bins=8)
        eng.reset()
        eng.set_trajectory_capture(np.asarray(sel, np.int32))
        got_rec = []
        for i, (n, m) in enumerate(((n1, mask), (n2, None))):
            rows = {}
            for done in range(0, n, 10):                           # rows drained every 10 steps
                eng.step(min(10, n - done))
                _merge(rows, eng.drain_trajectories())
            _assert_same(_snapshot(eng), want[i], f"segment {i}")
            got_rec.append(eng.drain_episodes())
            assert set(rows) == set(drains[i]), f"segment {i}: captured episodes"
            for key, (st, ps) in drains[i].items():
                assert list(rows[key][0]) == st, f"segment {i} {key}: steps"
                assert all(np.array_equal(a, b) for a, b in zip(rows[key][1], ps)), f"segment {i} {key}: positions"
            if m is not None:
                eng.reset_envs(np.asarray(m, np.uint8))
        got = np.concatenate(got_rec)
        got = got[np.lexsort((got[:, 1], got[:, 0]))]
        assert np.array_equal(got, rec)
        st = eng.episode_stats()
        steps = rec[:, 2].astype(np.int64)
        assert (st["count"], st["sum"], st["min"], st["max"]) == (len(steps), int(steps.sum()), int(steps.min()),
                                                                  int(steps.max()))
        assert np.array_equal(np.asarray(st["hist"], np.int64), np.bincount(np.minimum(steps, 7), minlength=8))
    finally:
        eng.close()


def _merge(rows, more):
    for key, (st, ps) in more.items():
        if key in rows:
            rows[key] = (list(rows[key][0]) + list(st), list(rows[key][1]) + list(ps))
        else:
            rows[key] = (list(st), list(ps))
    return rows


# 5. a room change followed by reset_envs over the changed envs
@pytest.mark.parametrize("case", ["wave12", "q20"])
def test_room_change_then_reset_envs(case):
    c = CASES[case]
    nbh, E, R = "neumann", 9, len(c["rooms"])
    roe = tuple(e % R for e in range(E))
    roe2 = tuple((r + 1) % R if e % 2 == 0 else r for e, r in enumerate(roe))
    mask = tuple(1 if a != b else 0 for a, b in zip(roe, roe2))
    ops = (("step", 25), ("snap",), ("rooms", roe2), ("reset_envs", mask), ("step", 40), ("snap",))
    want, _, _ = _oracle(c["A"], c["N"], nbh, c["rooms"], roe, None, None, ops)
    eng = _engine(c["rooms"][0], c["A"], c["N"], nbh, E)
    try:
        eng.set_env_rooms(_pairs(c["rooms"], nbh), np.asarray(roe, np.int32), kernel="block")
        _assert_on(eng, R)
        eng.reset()
        eng.step(25)
        _assert_same(_snapshot(eng), want[0], "before the change")
        eng.set_env_rooms(_pairs(c["rooms"], nbh), np.asarray(roe2, np.int32))   # the setting is sticky
        _assert_on(eng, R)
        eng.reset_envs(np.asarray(mask, np.uint8))
        eng.step(40)
        _assert_same(_snapshot(eng), want[1], "after the change")
    finally:
        eng.close()


# 6. off again: the create-time kernel, grid and launch_info(); a reset + T steps equals a fresh engine
@pytest.mark.parametrize("case", ["wave12", "q20"])
def test_off_restores_the_created_engine(case):
    c = CASES[case]
    nbh, E, T = "neumann", 9, 30
    a, b = (_engine(c["rooms"][1], c["A"], c["N"], nbh, E) for _ in range(2))
    try:
        created = a.launch_info()
        assert created["kernel"] == c["kernel"]
        a.set_env_rooms(_pairs(c["rooms"], nbh), kernel="block")
        _assert_on(a, len(c["rooms"]))
        a.set_fused_steps(4)                             # accepted and ignored while rooms are on
        for eng in (a, b):                               # the same step index on both afterwards
            eng.reset()
            eng.step(T)
        a.set_fused_steps(1)
        a.set_env_rooms([])
        assert a.launch_info() == created and a.env_rooms() is None
        before = [eng.counters() for eng in (a, b)]
        for eng in (a, b):
            eng.reset()
        a.step(T)
        for _ in range(T):
            b.step(1)
        got, want = _snapshot(a), _snapshot(b)
        for sn, c0 in zip((got, want), before):          # the counters count from create: this run's share
            for k in ("agent_steps", "resets"):
                sn[k] -= c0[k]
        _assert_same(got, want, "after set_env_rooms([]) + reset()")
    finally:
        a.close()
        b.close()


# 7. errors: each raises as specified and leaves the engine as it was
ERRORS = {
    # kernel="block" where there is no block form
    "group": (dict(room="R0", A=32, N=3), ("R0", "R1"), NotImplementedError),
    "mt": (dict(room="R0", A=40, N=3, rng="mt"), ("R0", "R1"), NotImplementedError),
    "f64": (dict(room="R0", A=40, N=3, f64=True), ("R0", "R1"), NotImplementedError),
    "scratch": (dict(room="P128", A=32, N=3), ("P128",), NotImplementedError),
    # the K records and room indices pass 64 KB at a forced K that fills the LDS
    "lds": (dict(room="R0", A=36, N=3, epb=64), ("R0", "R1"), NotImplementedError),
    "too_small": (dict(room="R0", A=40, N=3), ("R0", "TINY"), ValueError),
}
ERROR_KERNELS = {"group": "group", "mt": "wave", "f64": "block", "scratch": "block_scratch", "lds": "block",
                 "too_small": "wave"}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_errors_leave_the_engine_untouched(case):
    kw, rooms, exc = ERRORS[case]
    kw = dict(kw)
    room, A, N = kw.pop("room"), kw.pop("A"), kw.pop("N")
    E, T, nbh = 5, 10, "neumann"
    a, b = (_engine(room, A, N, nbh, E, **kw) for _ in range(2))
    try:
        created = a.launch_info()
        assert created["kernel"] == ERROR_KERNELS[case]
        with pytest.raises(exc):
            a.set_env_rooms(_pairs(rooms, nbh), kernel="block")
        assert a.launch_info() == created and a.env_rooms() is None
        if case in ("group", "too_small"):               # the setting is as it was: a plain call takes the lane form, or refuses
            if case == "group":
                a.set_env_rooms(_pairs(rooms, nbh))
                assert a.launch_info()["kernel"] == "lane"
                a.set_env_rooms(None)
            else:
                with pytest.raises(NotImplementedError):
                    a.set_env_rooms(_pairs(("R0", "R1"), nbh))
            assert a.launch_info() == created
        if kw.get("rng") == "mt":
            return                                       # MT engines are placed by the caller: nothing to step
        for eng in (a, b):
            eng.reset()
            eng.step(T)
        _assert_same(_snapshot(a), _snapshot(b), case)
    finally:
        a.close()
        b.close()


def test_mode_change_while_rooms_are_on():
    c = CASES["q20"]
    nbh, E, T, R = "neumann", 5, 10, len(c["rooms"])
    a, b = (_engine(c["rooms"][0], c["A"], c["N"], nbh, E) for _ in range(2))
    try:
        for eng in (a, b):
            eng.set_env_rooms(_pairs(c["rooms"], nbh), kernel="block")
        on = _assert_on(a, R)
        with pytest.raises(ValueError):
            a.set_env_rooms(_pairs(c["rooms"], nbh), kernel="lane")
        with pytest.raises(ValueError):
            a.set_env_rooms(_pairs(c["rooms"], nbh), kernel="wave")       # not a kernel name
        assert a.launch_info() == on
        for eng in (a, b):
            eng.reset()
            eng.step(T)
        _assert_same(_snapshot(a), _snapshot(b), "after the refused change")
        a.set_env_rooms(None, kernel="lane")             # off first, then the mode may change
        with pytest.raises(NotImplementedError):
            a.set_env_rooms(_pairs(c["rooms"], nbh))     # the lane form has no 20x20
        a.set_env_rooms(_pairs(c["rooms"], nbh), kernel="block")
        _assert_on(a, R)
    finally:
        a.close()
        b.close()
