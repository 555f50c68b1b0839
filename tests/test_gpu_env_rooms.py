"""Per-env rooms (ffm_engine_set_env_rooms / Engine.set_env_rooms).

The contract: env e of an engine with per-env rooms (global id env_base + e, room
rooms[room_of_env[e]]) evolves bit for bit like the env with the same global id of a homogeneous
engine created with that room's map and SFF (and, with per-env parameters on as well, that env's
parameter set).  The expected state comes from the oracle, one env at a time: one
oracle.Core(map, sff, params) per (room, set), step_philox_batch on the env's one-row slices with
its own N and global id, reset_philox for its placements.  Compared: positions (the live ones),
counts, DFF bits, the episodes counter, the agent_steps / resets counters and, where on, the
episode-log records and the trajectory rows.  Every case asserts launch_info()["kernel"] == "lane"
and ["env_rooms"] before comparing anything, and every case with auto-reset asserts from the
oracle's result that at least one env of every room completed an episode: only then has every
room's own free list and F been placed from.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 42
CREATE = (3, 1, 0.2, 0.2, 3)          # the create-time parameters (k_S, k_D, diffuse, decay, N)
KEYS = ("k_S", "k_D", "diffuse", "decay", "n_agents")
# the sets of tests/test_gpu_env_params.py
SETS5 = ((3, 1, 0.2, 0.2, 32), (0.5, 0, 0.2, 0.2, 5), (10, 2.5, 0.05, 0.6, 17), (1.5, 1, 0.5, 0.1, 1),
         (1, 4, 0.3, 0.3, 24))
ROOMS12 = ("R0", "R1", "R2", "R3")
ROOMS16 = ("S0", "S1")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def _room(name):
    """(map, float32 L1 SFF) of a named room; the four 12x12 rooms are trap-free under l1_sff."""
    from ffm_amd.data import make_room, l1_sff
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
    elif name == "S0":
        m = make_room(16, 16)
    elif name == "S1":
        m = make_room(16, 16, exit_pos=(0, 4), exit_width=2)
    elif name == "TINY":                     # two free cells
        m = make_room(12, 12)
        m[1:11, 1:11] = 2
        m[1, 5:7] = 0
    else:
        raise KeyError(name)
    s = l1_sff(m)
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


def test_room_free_cells():
    assert [int((_room(r)[0] == 0).sum()) for r in ROOMS12] == [100, 100, 92, 96]


def _params(s, nbh):
    return {"k_S": s[0], "k_D": s[1], "diffuse": s[2], "decay": s[3], "neighborhood": nbh}


def _dicts(sets):
    return [dict(zip(KEYS, s)) for s in sets]


def _episodes(eng):
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


# ---------------------------------------------------------------------------
# The oracle mirror: one Core per (room, set), one env per call.
# rooms: room names; roe / soe: per-env indices (tuples); sets: parameter sets, or None (CREATE).
# ops: ("step", n) | ("snap",) | ("reset_envs", mask tuple) | ("drain",)
# sel: envs whose trajectory rows are mirrored.  Returns the snapshots, the episode records and,
# per ("drain",), the rows {(env, k): (steps, [positions])} since the drain before.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(A, nbh, rooms, roe, sets, soe, ops, sel=()):
    from oracle import oracle as O
    E = len(roe)
    H, W = _room(rooms[0])[0].shape
    sets = sets or (CREATE,)
    soe = soe or (0,) * E
    cores = {}

    def core(e):
        key = (rooms[roe[e]], sets[soe[e]][:4])
        if key not in cores:
            m, s = _room(key[0])
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
    rec = np.asarray(recs, np.int64).reshape(-1, 4)
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))].astype(np.int32)
    for sn in snaps:
        for v in sn.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    rec.setflags(write=False)
    return tuple(snaps), rec, tuple(drains)


def _engine(rooms, A, nbh, E, create=CREATE, epb=0, rng="philox", room=None, f64=False):
    from ffm_amd.engine import Engine
    m, s = _room(room or rooms[0])
    return Engine(m, s.astype(np.float64) if f64 else s, n_envs=E, n_agents=create[4], agent_capacity=A,
                  params=_params(create, nbh), rng=rng, seed=SEED, auto_reset=True, envs_per_block=epb)


def _pairs(rooms):
    return [_room(r) for r in rooms]


def _snapshot(eng):
    pos, cnt, dff = eng.get_state()
    c = eng.counters()
    return {"pos": pos, "cnt": cnt, "dff": dff, "eps": _episodes(eng), "agent_steps": c["agent_steps"],
            "resets": c["resets"]}


def _assert_same(got, want, what=""):
    assert np.array_equal(got["cnt"], want["cnt"]), f"{what}: counts differ"
    assert np.array_equal(got["eps"], want["eps"]), f"{what}: episodes differ"
    for e in range(len(want["cnt"])):
        n = want["cnt"][e]
        assert np.array_equal(got["pos"][e, :n], want["pos"][e, :n]), f"{what}: positions differ (env {e})"
    assert np.array_equal(got["dff"].view(np.uint32), want["dff"].view(np.uint32)), f"{what}: DFF bits differ"
    assert got["agent_steps"] == want["agent_steps"], f"{what}: agent_steps"
    assert got["resets"] == want["resets"], f"{what}: resets"


def _assert_on(eng, n_rooms):
    info = eng.launch_info()
    assert info["kernel"] == "lane" and info["env_rooms"] == n_rooms and info["step_shards"] == 1
    return info


def _assert_coverage(eps, roe, n_rooms):
    """Every room's own free list and F was placed from: an env of each ended an episode."""
    roe = np.asarray(roe)
    for r in range(n_rooms):
        assert (eps[roe == r] > 0).any(), f"oracle: no env of room {r} ended an episode"


def _run(rooms, A, nbh, roe, snaps_at, before="group", check_rooms=False):
    E = len(roe)
    ops, last = [], 0
    for T in snaps_at:
        ops += [("step", T - last), ("snap",)]
        last = T
    want, _, _ = _oracle(A, nbh, rooms, tuple(roe), None, None, tuple(ops))
    _assert_coverage(want[-1]["eps"], roe, len(rooms))
    eng = _engine(rooms, A, nbh, E)
    try:
        assert eng.launch_info()["kernel"] == before and eng.launch_info()["env_rooms"] == 0
        assert eng.env_rooms() is None
        eng.set_env_rooms(_pairs(rooms), None if check_rooms else np.asarray(roe, np.int32))
        info = _assert_on(eng, len(rooms))
        if check_rooms:                                  # the default mapping and the getter
            maps, sffs, got_roe = eng.env_rooms()
            assert np.array_equal(got_roe, np.asarray(roe, np.int32))
            for r, (m, s) in enumerate(_pairs(rooms)):
                assert np.array_equal(maps[r], m) and np.array_equal(sffs[r].view(np.uint32), s.view(np.uint32))
        eng.reset()
        last = 0
        for T, w in zip(snaps_at, want):
            eng.step(T - last)
            last = T
            _assert_same(_snapshot(eng), w, f"{nbh} after {T} steps")
    finally:
        eng.close()
    return info


# 1. room e % 4, both neighbourhoods (E odd: the last pair is half empty)
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_four_rooms_match_oracle(nbh):
    _run(ROOMS12, 32, nbh, [e % 4 for e in range(11)], (1, 17, 40), check_rooms=True)


# 2. an arbitrary mapping: same and different rooms within a pair and across consecutive pairs
def test_arbitrary_mapping():
    _run(ROOMS12, 32, "neumann", [0, 0, 1, 2, 2, 2, 3, 0, 1], (1, 17, 40))


# 3. one persistent block: every wave steps about 17 pairs and re-stages between them; the deferred
#    placements find each env's room
@pytest.mark.parametrize("roe_mod", [4, 3])
def test_one_persistent_block(monkeypatch, roe_mod):
    monkeypatch.setenv("FFM_WAVE_BLOCKS", "1")
    rooms = ROOMS12[:roe_mod]                 # % 3: a half's room changes from pair to pair of its wave
    info = _run(rooms, 32, "neumann", [e % roe_mod for e in range(130)], (25,))
    assert info["blocks"] == 1


# 4. crossed with per-env parameters, in either call order; kernel="group" is remembered, not used
@pytest.mark.parametrize("order", ["rooms_params", "params_rooms_group"])
def test_crossed_with_env_params(order):
    E, A, T = 20, 32, 40
    roe = tuple(e % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    (want,), _, _ = _oracle(A, "neumann", ROOMS12, roe, SETS5, soe, (("step", T), ("snap",)))
    _assert_coverage(want["eps"], roe, 4)
    eng = _engine(ROOMS12, A, "neumann", E, create=SETS5[0])
    try:
        created = eng.launch_info()
        assert created["kernel"] == "group"
        if order == "rooms_params":
            eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe, np.int32))
            eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32))
        else:
            eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32), kernel="group")
            assert eng.launch_info()["kernel"] == "group"
            eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe, np.int32))
        _assert_on(eng, 4)
        eng.reset()
        eng.step(T)
        _assert_same(_snapshot(eng), want, order)
        eng.set_env_rooms(None)
        info = eng.launch_info()
        assert info["env_rooms"] == 0 and eng.env_rooms() is None
        # the parameter sets stay on, with the kernel they asked for
        assert info["kernel"] == ("group" if order == "params_rooms_group" else "lane")
        assert [s["n_agents"] for s in eng.env_params()[0]] == [s[4] for s in SETS5]
        eng.set_env_params(None)
        assert eng.launch_info() == created
    finally:
        eng.close()


# 5. masked reset_envs + the episode log + trajectory capture of two envs in different rooms
def test_reset_envs_log_and_capture():
    E, A = 11, 32
    roe = tuple(e % 4 for e in range(E))
    sel = (2, 5)                                         # rooms R2 and R1
    mask = tuple(1 if e in (0, 2, 7, 10) else 0 for e in range(E))
    ops = (("step", 12), ("snap",), ("drain",), ("reset_envs", mask), ("step", 28), ("snap",), ("drain",))
    want, rec, drains = _oracle(A, "moore", ROOMS12, roe, None, None, ops, sel)
    _assert_coverage(want[-1]["eps"], roe, 4)
    eng = _engine(ROOMS12, A, "moore", E)
    try:
        eng.set_env_rooms(_pairs(ROOMS12))
        _assert_on(eng, 4)
        eng.set_episode_log(capacity=E * 64)
        eng.reset()
        eng.set_trajectory_capture(np.asarray(sel, np.int32))
        got_rec = []
        for i, (n, m) in enumerate(((12, mask), (28, None))):
            eng.step(n)
            _assert_same(_snapshot(eng), want[i], f"segment {i}")
            got_rec.append(eng.drain_episodes())
            rows = eng.drain_trajectories()              # before the masked reset
            assert set(rows) == set(drains[i]), f"segment {i}: captured episodes"
            for key, (st, ps) in drains[i].items():
                assert list(rows[key][0]) == st, f"segment {i} {key}: steps"
                assert all(np.array_equal(a, b) for a, b in zip(rows[key][1], ps)), f"segment {i} {key}: positions"
            if m is not None:
                eng.reset_envs(np.asarray(m, np.uint8))
        got = np.concatenate(got_rec)
        got = got[np.lexsort((got[:, 1], got[:, 0]))]
        assert np.array_equal(got, rec)
    finally:
        eng.close()


# 6. the generic template: 16x16 rooms (a lane engine)
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_generic_template_16x16(nbh):
    _run(ROOMS16, 24, nbh, [e % 2 for e in range(5)], (40,), before="lane", check_rooms=True)


# 7. engine against engine
def test_one_room_equals_untouched_engine_and_off_again():
    E, A, T = 37, 32, 20
    a, b = _engine(("R2",), A, "neumann", E), _engine(("R2",), A, "neumann", E)
    try:
        created = a.launch_info()
        a.set_env_rooms(_pairs(("R2",)))                 # the create-time room
        _assert_on(a, 1)
        a.set_fused_steps(4)                             # accepted and ignored while rooms are on
        for eng in (a, b):
            eng.reset()
        a.step(T)
        for _ in range(T):
            b.step(1)
        want = _snapshot(b)
        _assert_same(_snapshot(a), want, "one room against an untouched engine")
        assert want["eps"].sum() > 0
        a.set_fused_steps(1)
        a.set_env_rooms([])
        assert a.launch_info() == created
        for eng in (a, b):
            eng.reset()
            eng.step(T)
        _assert_same(_snapshot(a), _snapshot(b), "after set_env_rooms(None) + reset()")
    finally:
        a.close()
        b.close()


# 8. errors: each raises as specified and leaves the engine as it was
def _bad_border():
    m, s = _room("R0")
    m = np.array(m)
    m[0, 3] = 0
    return [(m, s)]


ERRORS = {
    "mt": (dict(rng="mt"), lambda: _pairs(ROOMS12), None, NotImplementedError),
    "block64": (dict(room="B64"), None, None, NotImplementedError),
    "f64": (dict(f64=True), lambda: _pairs(ROOMS12), None, NotImplementedError),
    "shape": ({}, lambda: [_room("S0")], None, ValueError),
    "border": ({}, _bad_border, None, ValueError),
    "index": ({}, lambda: _pairs(ROOMS12), [0, 1, 2, 4, 0, 1, 2], ValueError),
    "too_small": ({}, lambda: [_room("R0"), _room("TINY")], None, ValueError),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_errors_leave_the_engine_untouched(case):
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    kw, rooms, roe, exc = ERRORS[case]
    E, A, T = 7, 32, 20

    def make():
        if case == "block64":
            m = make_room(64, 64)
            return Engine(m, l1_sff(m), n_envs=E, n_agents=3, agent_capacity=A, params=_params(CREATE, "neumann"),
                          seed=SEED, auto_reset=True)
        return _engine(ROOMS12, A, "neumann", E, **kw)

    a, b = make(), make()
    try:
        created = a.launch_info()
        if case == "block64":
            assert created["kernel"] not in ("lane", "group")
            m = make_room(64, 64, exit_pos=(0, 10))
            rooms = lambda: [(m, l1_sff(m))]
        with pytest.raises(exc):
            a.set_env_rooms(rooms(), roe)
        assert a.launch_info() == created and a.env_rooms() is None
        for eng in (a, b):
            eng.reset()
            eng.step(T)
        _assert_same(_snapshot(a), _snapshot(b), case)
    finally:
        a.close()
        b.close()
