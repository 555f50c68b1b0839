"""Per-env rooms on the group kernel (Engine.set_env_rooms(..., kernel="group"),
ffm_engine_set_env_rooms_kernel mode 2).

The contract is that of tests/test_gpu_env_rooms.py: env e of an engine with per-env rooms evolves bit
for bit like the env with the same global id of a homogeneous engine created with that room's map and
SFF (and that env's parameter set).  The expected state comes from the oracle, one env at a time (the
helpers of tests/env_sweep_util.py).  Every case asserts
launch_info()["kernel"] == "group", ["group_one"] and ["env_rooms"] before comparing anything, and from
the oracle's result that at least one env of every room ended an episode: only then has every room's
own free list and F been placed from.  Every case fails without the feature, where kernel="group" is a
ValueError.
"""
import functools

import numpy as np
import pytest

import env_sweep_util as U
from env_sweep_util import SETS5, _assert_coverage, _assert_same, _dicts, _snapshot

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOMS12 = ("R0", "R1", "R2", "R3")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _map(name):
    """The map of a named room; the four 12x12 rooms are trap-free under l1_sff."""
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
    elif name == "S0":
        m = make_room(16, 16)
    elif name == "TINY":                     # two free cells
        m = make_room(12, 12)
        m[1:11, 1:11] = 2
        m[1, 5:7] = 0
    else:
        raise KeyError(name)
    return m


_room = U.rooms(_map)                        # name -> (map, float32 L1 SFF)
# the shared helpers (env_sweep_util.py) over this file's rooms; rooms on: the group kernel's single-group form
_oracle = functools.partial(U._oracle, _room)   # (A, nbh, rooms, roe, sets, soe, ops, sel=())
_assert_on = functools.partial(U._assert_on, kernel="group")   # (eng, n_rooms, g=None)


def test_room_free_cells():
    assert [int((_room(r)[0] == 0).sum()) for r in ROOMS12] == [100, 100, 92, 96]


def _engine(rooms, A, nbh, E, room=None, **kw):
    return U._engine(_room(room or rooms[0]), A, nbh, E, **kw)


def _pairs(rooms):
    return [_room(r) for r in rooms]


def _run(rooms, A, nbh, roe, snaps_at, g=None, shards=None, chunk=None):
    """set_env_rooms(kernel="group") on a group engine, reset, then step to every snapshot (in step(chunk)
    calls) and compare with the oracle."""
    E = len(roe)
    ops, last = [], 0
    for T in snaps_at:
        ops += [("step", T - last), ("snap",)]
        last = T
    want, _, _ = _oracle(A, nbh, rooms, tuple(roe), None, None, tuple(ops))
    _assert_coverage(want[-1]["eps"], roe, len(rooms))
    eng = _engine(rooms, A, nbh, E)
    try:
        created = eng.launch_info()
        assert created["kernel"] == "group" and created["env_rooms"] == 0
        eng.set_env_rooms(_pairs(rooms), np.asarray(roe, np.int32), kernel="group")
        info = _assert_on(eng, len(rooms), g)
        if shards is not None:
            assert info["step_shards"] == shards
        eng.reset()
        last = 0
        for T, w in zip(snaps_at, want):
            n = T - last
            while n > 0:
                k = min(n, chunk or n)
                eng.step(k)
                n -= k
            last = T
            _assert_same(_snapshot(eng), w, f"{nbh} after {T} steps")
        eng.set_env_rooms(None)
        assert eng.launch_info() == created
    finally:
        eng.close()
    return info


# 1. room e % 4, both neighbourhoods, the default G (2 at this size); E odd: a partial last group
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_four_rooms_match_oracle(nbh):
    _run(ROOMS12, 32, nbh, [e % 4 for e in range(11)], (1, 17, 40), g=2)


# 2. forced G = 4: equal and different rooms inside a group, a partial group of one env in room 1;
#    E below G
@pytest.mark.parametrize("case", ["nine", "one", "three"])
def test_forced_g4_arbitrary_mapping(monkeypatch, case):
    monkeypatch.setenv("FFM_GROUP_ENVS", "4")
    rooms, roe = {"nine": (ROOMS12, [0, 0, 1, 2, 2, 2, 3, 0, 1]),
                  "one": (("R1",), [0]),
                  "three": (("R0", "R2", "R3"), [1, 0, 2])}[case]
    _run(rooms, 32, "neumann", roe, (1, 17, 40), g=4)


# 3. crossed with per-env parameters at forced G = 4 (envs 4-7 hold 78 live agents: the second agent
#    chunk runs with per-env SFFs), in either call order and with kernel="group" remembered for the sets
@pytest.mark.parametrize("order", ["rooms_params", "params_rooms", "params_group_rooms"])
def test_crossed_with_env_params(monkeypatch, order):
    monkeypatch.setenv("FFM_GROUP_ENVS", "4")
    E, A, T, T2 = 20, 32, 40, 15
    roe = tuple(e % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    (want,), _, _ = _oracle(A, "neumann", ROOMS12, roe, SETS5, soe, (("step", T), ("snap",)))
    _assert_coverage(want["eps"], roe, 4)
    eng, twin = (_engine(ROOMS12, A, "neumann", E, create=SETS5[0]) for _ in range(2))
    try:
        created = eng.launch_info()
        assert created["kernel"] == "group"
        pk = "group" if order == "params_group_rooms" else None
        if order == "rooms_params":
            eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe, np.int32), kernel="group")
            eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32))
        else:
            eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32), kernel=pk)
            assert eng.launch_info()["kernel"] == ("group" if pk else "lane")
            eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe, np.int32), kernel="group")
        _assert_on(eng, 4, 4)
        eng.reset()
        eng.step(T)
        _assert_same(_snapshot(eng), want, order)
        eng.set_env_rooms(None)
        info = eng.launch_info()
        assert info["env_rooms"] == 0 and eng.env_rooms() is None
        # the parameter sets stay on, with the kernel they asked for
        assert info["kernel"] == ("group" if pk else "lane")
        assert [s["n_agents"] for s in eng.env_params()[0]] == [s[4] for s in SETS5]
        # ... and the same bits as a twin that never had rooms (same step indices: reset, T steps, reset)
        twin.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32), kernel=pk)
        assert twin.launch_info() == info
        twin.reset()
        twin.step(T)
        for e in (eng, twin):
            e.reset()
            e.step(T2)
        _assert_same(_snapshot(eng), _snapshot(twin), order + ": after rooms off", counters=False)
        eng.set_env_params(None)
        assert eng.launch_info() == created
    finally:
        eng.close()
        twin.close()


# 4. step shards: every shard's launch takes room_of_env + e0 and envp + e0
@pytest.mark.parametrize("shards", [2, 3])
def test_step_shards(monkeypatch, shards):
    monkeypatch.setenv("FFM_STEP_SHARDS", str(shards))
    roe = [(e * 7 + e // 5) % 4 for e in range(37)]
    info = _run(ROOMS12, 32, "neumann", roe, (12, 40), shards=shards, chunk=7)
    assert info["step_shards"] == shards


# 5. FFM_WAVE_BLOCKS=1 does not shrink the room form's grid: a wave per group
def test_wave_blocks_override_keeps_the_grid(monkeypatch):
    monkeypatch.setenv("FFM_WAVE_BLOCKS", "1")
    E = 130
    info = _run(ROOMS12, 32, "neumann", [e % 4 for e in range(E)], (25,))
    groups = -(-E // info["group_g"])
    assert info["blocks"] == -(-groups // 4) and info["blocks"] > 1 and info["group_one"]


# 6. masked reset_envs + the episode log + trajectory capture of two envs in different rooms
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
        eng.set_env_rooms(_pairs(ROOMS12), kernel="group")
        _assert_on(eng, 4)
        eng.set_episode_log(capacity=E * 64, hist_bins=16)
        eng.reset()
        eng.set_trajectory_capture(np.asarray(sel, np.int32))
        info = _assert_on(eng, 4)
        assert info["step_shards"] == 1                  # capture: one launch per step
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
        stats = eng.episode_stats()
        assert stats["count"] == len(rec) and stats["min"] == int(rec[:, 2].min()) and stats["max"] == int(rec[:, 2].max())
        assert stats["sum"] == int(rec[:, 2].sum())
    finally:
        eng.close()


# 7. a second set_env_rooms call changes some envs' rooms; reset_envs over exactly those, then step
def test_room_change_then_reset_envs():
    E, A = 13, 32
    roe1 = tuple(e % 4 for e in range(E))
    roe2 = tuple((r + 1) % 4 if e % 3 == 0 else r for e, r in enumerate(roe1))
    mask = tuple(int(a != b) for a, b in zip(roe1, roe2))
    assert 0 < sum(mask) < E
    ops = (("step", 10), ("snap",), ("rooms", roe2), ("reset_envs", mask), ("step", 40), ("snap",))
    want, _, _ = _oracle(A, "neumann", ROOMS12, roe1, None, None, ops)
    _assert_coverage(want[-1]["eps"] - want[0]["eps"], roe2, 4)
    eng = _engine(ROOMS12, A, "neumann", E)
    try:
        eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe1, np.int32), kernel="group")
        _assert_on(eng, 4)
        eng.reset()
        eng.step(10)
        _assert_same(_snapshot(eng), want[0], "before the change")
        eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe2, np.int32), kernel="group")
        _assert_on(eng, 4)
        assert np.array_equal(eng.env_rooms()[2], np.asarray(roe2, np.int32))
        eng.reset_envs(np.asarray(mask, np.uint8))
        eng.step(40)
        _assert_same(_snapshot(eng), want[1], "after the change")
    finally:
        eng.close()


# 8. engine against engine: the group form and the lane form, same rooms, sets and seed
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_group_form_equals_lane_form(nbh):
    E, A, T = 64, 32, 60
    roe = tuple((e + e // 4) % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    (want,), rec, _ = _oracle(A, nbh, ROOMS12, roe, SETS5, soe, (("step", T), ("snap",)))
    _assert_coverage(want["eps"], roe, 4)
    engs = {k: _engine(ROOMS12, A, nbh, E, create=SETS5[0]) for k in ("lane", "group")}
    try:
        out = {}
        for k, eng in engs.items():
            eng.set_env_rooms(_pairs(ROOMS12), np.asarray(roe, np.int32), kernel=k)
            eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32))
            info = eng.launch_info()
            assert info["kernel"] == k and info["env_rooms"] == 4 and info["group_one"] == (k == "group")
            eng.set_episode_log(capacity=E * 64)
            eng.reset()
            eng.step(T)
            got = eng.drain_episodes()
            out[k] = (_snapshot(eng), got[np.lexsort((got[:, 1], got[:, 0]))], eng.counters())
        _assert_same(out["group"][0], out["lane"][0], "group form against lane form")
        assert np.array_equal(out["group"][0]["pos"][out["lane"][0]["cnt"][:, None] > np.arange(A)],
                              out["lane"][0]["pos"][out["lane"][0]["cnt"][:, None] > np.arange(A)])
        assert np.array_equal(out["group"][1], out["lane"][1]) and len(out["group"][1]) > 0
        assert out["group"][2] == out["lane"][2]
        _assert_same(out["group"][0], want, "group form against the oracle")
        assert np.array_equal(out["group"][1], rec)
    finally:
        for eng in engs.values():
            eng.close()


# 9. errors: each raises as specified and leaves the engine as it was
REFUSED = {
    "lane16": (dict(room="S0", A=24), lambda: [_room("S0")], NotImplementedError),
    "wave": (dict(A=40), lambda: _pairs(ROOMS12), NotImplementedError),
    "mt": (dict(rng="mt"), lambda: _pairs(ROOMS12), NotImplementedError),
    "too_small": ({}, lambda: [_room("R0"), _room("TINY")], ValueError),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_errors_leave_the_engine_untouched(case):
    kw, rooms, exc = REFUSED[case]
    kw = dict(kw)
    E, A, T = 7, kw.pop("A", 32), 20
    auto = kw.get("rng") != "mt"

    def make():
        return _engine(ROOMS12, A, "neumann", E, **kw)

    a, b = make(), make()
    try:
        created = a.launch_info()
        assert created["kernel"] == {"lane16": "lane", "wave": "wave", "too_small": "group"}.get(case, created["kernel"])
        assert case != "mt" or created["kernel"] != "group"
        with pytest.raises(exc):
            a.set_env_rooms(rooms(), None, kernel="group")
        assert a.launch_info() == created and a.env_rooms() is None
        if auto:                                         # (an MT engine places on the host: nothing to step here)
            for eng in (a, b):
                eng.reset()
                eng.step(T)
            _assert_same(_snapshot(a), _snapshot(b), case)
        if case == "too_small":                          # the refusal left the kernel setting alone as well
            a.set_env_rooms(_pairs(ROOMS12))
            assert a.launch_info()["kernel"] == "lane"
    finally:
        a.close()
        b.close()


def test_kernel_change_while_on_is_refused():
    E, A, T = 9, 32, 30
    roe = np.asarray([e % 4 for e in range(E)], np.int32)
    (want,), _, _ = _oracle(A, "neumann", ROOMS12, tuple(int(r) for r in roe), None, None, (("step", T), ("snap",)))
    _assert_coverage(want["eps"], roe, 4)
    eng = _engine(ROOMS12, A, "neumann", E)
    try:
        created = eng.launch_info()
        eng.set_env_rooms(_pairs(ROOMS12), roe, kernel="group")
        on = _assert_on(eng, 4)
        for other in ("lane", "block"):
            with pytest.raises(ValueError):
                eng.set_env_rooms(_pairs(ROOMS12), roe, kernel=other)
            assert eng.launch_info() == on
        eng.reset()
        eng.step(T)
        _assert_same(_snapshot(eng), want, "after the refused kernel changes")
        eng.set_env_rooms(None)
        assert eng.launch_info() == created
    finally:
        eng.close()
