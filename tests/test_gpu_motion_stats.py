"""Motion statistics on the device (ffm_engine_set_motion_stats): per-cell flux, speed curves and
the egress time by origin.

The expected arrays come from the oracle mirror of tests/motion_mirror.py, which finds leavers and
successors by sequential order-preserving walks, not by the kernel's set and rank rules, and keeps
the origins in a Python list; the device's five tables must equal them exactly.
tests/test_motion_mirror.py pins on the CPU that every case here is not vacuous; the checks that
cost nothing are repeated.
"""
import numpy as np
import pytest

import exit_flow_mirror as X
import motion_mirror as M
from env_sweep_util import SETS5, _dicts
from motion_mirror import BINS, ENGINES, M32, PAR, TABLES

import env_sweep_util as U

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS", "FFM_GROUP_ONE", "FFM_FIELD_STATS_FORM",
            "FFM_FIELD_STATS_SLOTS", "FFM_FIELD_STATS_BLOCKS", "FFM_EXIT_FLOW_FORM", "FFM_EXIT_FLOW_BLOCKS",
            "FFM_MOTION_STATS_FORM", "FFM_MOTION_STATS_BLOCKS")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    """The switches are read when the engine is created and when the feature is set."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _engine(room, A, N, nbh, E, auto=True, epb=0, rng="philox"):
    from ffm_amd.engine import Engine
    m, s = X.room(room)
    return Engine(m, s, n_envs=E, n_agents=N, agent_capacity=A, params=U._params(PAR, nbh), rng=rng, seed=U.SEED,
                  auto_reset=auto, envs_per_block=epb)


def _state(eng):
    pos, cnt, dff = eng.get_state()
    return {"pos": pos, "cnt": cnt, "dff": dff, "eps": U._episodes(eng), "ctr": eng.counters(), "t": eng.step_index}


def _assert_same_state(a, b):
    assert np.array_equal(a["cnt"], b["cnt"]), "counts"
    for e in range(len(a["cnt"])):
        assert np.array_equal(a["pos"][e, :a["cnt"][e]], b["pos"][e, :b["cnt"][e]]), f"env {e} positions"
    assert np.array_equal(a["dff"].view(np.uint32), b["dff"].view(np.uint32)), "DFF bits"
    assert np.array_equal(a["eps"], b["eps"]), "episodes"
    assert a["ctr"] == b["ctr"], (a["ctr"], b["ctr"])
    assert a["t"] == b["t"]


def _positions(cells, A):
    pos = np.full((len(cells), A), 0xFFFF, np.uint16)
    for e, c in enumerate(cells):
        pos[e, :len(c)] = c
    return pos, np.array([len(c) for c in cells], np.int32)


def _drive(eng, ops, mo, t0=0, chunk=None):
    """reset() at step index t0, then the ops; mo = dict of set_motion_stats' arguments or None (feature
    off: "on" and "mark" are skipped).  Without an "on" op the feature is set before the reset.  A
    ("mark",) reads and clears; returns the reads (None for a mark before the feature is on)."""
    is_on = mo is not None and not any(op[0] == "on" for op in ops)
    if is_on:
        eng.set_motion_stats(**mo)
    eng.step_index = t0 & M32
    eng.reset()
    reads = []
    for op in ops:
        if op[0] == "step":
            left = op[1]
            while left:
                n = min(left, chunk or left)
                eng.step(n)
                left -= n
        elif op[0] == "reset_envs":
            eng.reset_envs(np.asarray(op[1], np.uint8))
        elif op[0] == "set_state":
            pos, cnt = _positions(op[1], eng.A)
            eng.set_state(0, positions=pos, counts=cnt)
        elif op[0] == "on" and mo is not None:
            eng.set_motion_stats(**mo)
            is_on = True
        elif op[0] == "mark" and mo is not None:
            reads.append(eng.motion_stats(clear=True) if is_on else None)
    if mo is not None:
        reads.append(eng.motion_stats())
    return reads


def _assert_motion(got, w, nbh, egress=True):
    for k in TABLES if egress else TABLES[:3]:
        assert got[k].dtype == np.uint64 and got[k].shape == w[k].shape, (k, got[k].shape, w[k].shape)
        assert np.array_equal(got[k], w[k]), k
    assert tuple(got["directions"]) == M.NEIGHBOURS[nbh] + ((0, 0),)
    M.assert_identities(got)


def _sum(ws, keys=TABLES + ("exited", "outflow")):
    return {k: sum(w[k].astype(np.uint64) for w in ws) for k in keys}


def _mo3(E):
    return dict(classes=X.cls3(E), n_classes=3, curve_bins=BINS)


def _run_plain(name, nbh, ops=None, auto=True, t0=0, on=True, chunk=None, fused=1, check=None, E=None):
    """An engine of ENGINES under ops (default: T steps); classes e % 3, BINS bins.  Returns (reads, state)."""
    room, A, N, E0, T, epb, kernel = ENGINES[name]
    E = E or E0
    ops = ops or (("step", T),)
    eng = _engine(room, A, N, nbh, E, auto, epb)
    try:
        assert eng.launch_info()["kernel"] == kernel
        if fused > 1:
            eng.set_fused_steps(fused)
        reads = _drive(eng, ops, _mo3(E) if on else None, t0, chunk)
        if check is not None:
            check(eng)
        return reads, _state(eng)
    finally:
        eng.close()


# 1. every step kernel, both neighbourhoods; the step itself does not change
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_every_step_kernel(name, nbh):
    (w,), eps, _ = M.plain(name, nbh)
    M.assert_not_vacuous(w, eps, ENGINES[name][0])
    (got,), on = _run_plain(name, nbh, chunk=7)
    _assert_motion(got, w, nbh)
    assert int(got["egress_count"].sum()) == on["ctr"]["exits"]
    _, off = _run_plain(name, nbh, chunk=7, on=False)
    _assert_same_state(on, off)


# 2. no auto-reset: everybody leaves exactly once, and `present` is the field statistics' `remaining`
@pytest.mark.parametrize("name", ["group", "block"])
def test_no_auto_reset(name):
    room, A, N, E, T, epb, _ = ENGINES[name]
    (first, last), _, _ = M.plain(name, "moore", (("step", T), ("mark",), ("step", 10)), auto=False)
    assert int(first["egress_count"].sum()) == E * N and last["events"] == 0
    eng = _engine(room, A, N, "moore", E, auto=False, epb=epb)
    try:
        eng.set_field_stats(X.cls3(E), 3, BINS)
        eng.set_motion_stats(**_mo3(E))
        eng.reset()
        eng.step(T)
        got = eng.motion_stats()
        _assert_motion(got, first, "moore")
        assert int(got["egress_count"].sum()) == E * N == eng.counters()["exits"]
        eng.step(10)                                     # the envs are empty: nothing more
        _assert_motion(eng.motion_stats(), first, "moore")
        rem = eng.field_stats()["remaining"]
        for tau in range(2, BINS - 1):
            assert np.array_equal(got["present"][:, tau], rem[:, tau - 1]), tau
    finally:
        eng.close()


# 3. launch geometry: the bits of case 1's group run
GEOMETRY = {
    "two_shards": (dict(FFM_STEP_SHARDS=2), dict(step_shards=2), {}),
    "group_envs_4": (dict(FFM_GROUP_ENVS=4), dict(group_g=4), {}),
    "global_form": (dict(FFM_MOTION_STATS_FORM="global"), {}, dict(form="global")),
    "one_block": (dict(FFM_MOTION_STATS_BLOCKS=1), {}, dict(form="lds", blocks=1)),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(monkeypatch, case):
    env, info, motion_info = GEOMETRY[case]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))

    def check(eng):
        li, mi = eng.launch_info(), eng.motion_stats_info()
        for k, v in info.items():
            assert li[k] == v, (k, li)
        assert mi["classes"] == 3 and mi["curve_bins"] == BINS and mi["slots"] >= 1
        for k, v in motion_info.items():
            assert mi[k] == v, (k, mi)
    (w,), _, _ = M.plain("group", "moore")
    (got,), _ = _run_plain("group", "moore", chunk=50, check=check)     # step(n > 1): the shards are in effect
    _assert_motion(got, w, "moore")


def test_fused_steps_setting():
    """With the feature on the fused path is not taken: the same tables, and the state of a fused engine
    with the feature off."""
    def check(eng):
        assert eng.launch_info()["multi"]
    (w,), _, _ = M.plain("group", "moore")
    (got,), on = _run_plain("group", "moore", chunk=50, fused=4, check=check)
    _assert_motion(got, w, "moore")
    _, off = _run_plain("group", "moore", chunk=50, fused=4, on=False, check=check)
    _assert_same_state(on, off)


def test_lds_form_refused_beyond_the_budget(monkeypatch):
    """40 classes x (144 x 10 + 256) words are 271 KB as u32: the global form by itself; forcing lds raises."""
    room, A, N, E = ENGINES["group"][:4]
    eng = _engine(room, A, N, "moore", E)
    try:
        eng.set_motion_stats(classes=X.cls3(E), n_classes=40, curve_bins=128)
        assert eng.motion_stats_info()["form"] == "global"
        before = eng.launch_info(), eng.motion_stats_info()
        monkeypatch.setenv("FFM_MOTION_STATS_FORM", "lds")
        with pytest.raises(ValueError):
            eng.set_motion_stats(classes=X.cls3(E), n_classes=40, curve_bins=128)
        assert (eng.launch_info(), eng.motion_stats_info()) == before
    finally:
        eng.close()


# 4. with the exit flow, the field statistics, the episode log and capture on, on a caller's stream
def test_callers_stream_with_everything_on():
    room, A, N, E, T = ENGINES["group"][:5]
    nbh, sel = "moore", [0, 5, 36]
    (w,), _, doors = M.plain("group", nbh)
    st = torch.cuda.Stream()
    out = []
    for on in (True, False):
        eng = _engine(room, A, N, nbh, E)
        try:
            eng.set_episode_log(capacity=E * T, hist_bins=32, stream=st)
            eng.set_field_stats(X.cls3(E), 3, BINS, stream=st)
            eng.set_exit_flow(stream=st, classes=X.cls3(E), n_classes=3, curve_bins=BINS)
            if on:
                eng.set_motion_stats(stream=st, **_mo3(E))
            eng.set_trajectory_capture(sel, period=1, capacity_rows=len(sel) * (T + 8), stream=st)
            eng.reset(stream=st)
            for _ in range(T // 50):
                eng.step(50, stream=st)
            if on:
                _assert_motion(eng.motion_stats(stream=st), w, nbh)      # the same as alone (case 1's mirror)
            flow = eng.exit_flow(stream=st)
            # the flow's tables are right with the motion kernel running before its own (the carry hand-over)
            assert np.array_equal(flow["exited"], w["exited"]) and np.array_equal(flow["outflow"], w["outflow"])
            assert np.array_equal(flow["door_of_cell"], doors)
            out.append((eng.drain_episodes(stream=st), eng.field_stats(stream=st), eng.drain_trajectories(stream=st),
                        _state(eng)))
        finally:
            eng.close()
    (rec, fs, rows, s1), (rec0, fs0, rows0, s0) = out
    assert len(rec0) >= 2 * E and np.array_equal(rec, rec0)
    assert all(np.array_equal(fs[k], fs0[k]) for k in fs0)
    assert rows.keys() == rows0.keys() and len(rows) >= 2 * len(sel)
    for k in rows:
        assert np.array_equal(rows[k][0], rows0[k][0])
        assert all(np.array_equal(p, q) for p, q in zip(rows[k][1], rows0[k][1]))
    _assert_same_state(s1, s0)


def test_flow_and_motion_come_and_go():
    """The snapshot is shared: the flow turned on and off while the motion statistics stay on, and the
    reverse; each still equals its mirror."""
    room, A, N, E = ENGINES["group"][:4]
    nbh = "moore"
    flow3 = dict(classes=X.cls3(E), n_classes=3, curve_bins=BINS)
    ws, _, _ = M.plain("group", nbh, (("step", 100), ("mark",), ("step", 100), ("mark",), ("step", 100)))
    assert all(w["events"] > 0 for w in ws)
    eng = _engine(room, A, N, nbh, E)
    try:
        eng.set_motion_stats(**_mo3(E))
        eng.reset()
        eng.step(100)
        eng.set_exit_flow(**flow3)
        eng.step(100)
        flow = eng.exit_flow()
        assert np.array_equal(flow["exited"], ws[1]["exited"]) and np.array_equal(flow["outflow"], ws[1]["outflow"])
        eng.set_exit_flow(n_classes=0)
        assert eng.launch_info()["exit_flow"] == "off" and eng.motion_stats_info() != "off"
        eng.step(100)
        _assert_motion(eng.motion_stats(), _sum(ws), nbh)
    finally:
        eng.close()
    ws, _, _ = M.plain("group", nbh, (("step", 100), ("on", "keep"), ("mark",), ("step", 100), ("mark",), ("step", 100)))
    eng = _engine(room, A, N, nbh, E)
    try:
        eng.set_exit_flow(**flow3)
        eng.reset()
        eng.step(100)
        eng.set_motion_stats(**_mo3(E))
        eng.step(100)
        _assert_motion(eng.motion_stats(), ws[1], nbh)
        eng.set_motion_stats(n_classes=0)
        assert eng.motion_stats_info() == "off" and eng.launch_info()["exit_flow"] != "off"
        eng.step(100)
        flow, want = eng.exit_flow(), _sum(ws)
        assert np.array_equal(flow["exited"], want["exited"]) and np.array_equal(flow["outflow"], want["outflow"])
    finally:
        eng.close()


# 5. whoever writes pos, cnt or ep_start refreshes the snapshot; a placement renews the origins
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_snapshot_and_origins(nbh):
    E = ENGINES["group"][3]
    every = (1,) * E
    third = tuple(int(e % 3 == 0) for e in range(E))
    for mask in (every, third):
        ops = (("step", 30), ("reset_envs", mask), ("mark",), ("step", 1), ("mark",), ("step", 29))
        ws, _, _ = M.plain("group", nbh, ops)
        assert ws[1]["tau1"] > 0                         # agents placed next to an exit leave with tau = 1
        reads, _ = _run_plain("group", nbh, ops)
        for got, w in zip(reads, ws):
            _assert_motion(got, w, nbh)
    # two calls in a row: the envs of the first are first stepped with tau = 2, not 1
    other = tuple(int(e % 3 == 1) for e in range(E))
    ops = (("step", 30), ("reset_envs", third), ("reset_envs", other), ("mark",), ("step", 1), ("mark",), ("step", 29))
    ws, _, _ = M.plain("group", nbh, ops)
    assert ws[1]["late_first"] > 0 and ws[1]["tau1"] > 0
    reads, _ = _run_plain("group", nbh, ops)
    for got, w in zip(reads, ws):
        _assert_motion(got, w, nbh)
    ops = (("step", 30), ("mark",), ("set_state", X.ring_state(E, 32)), ("step", 30))
    (w0, w1), _, _ = M.plain("group", nbh, ops)
    (g0, g1), _ = _run_plain("group", nbh, ops)
    _assert_motion(g0, w0, nbh)
    _assert_motion(g1, w1, nbh, egress=False)            # the origins of written envs are undefined


# 6. lifecycle: on mid-run (ep_start absent, and there already), clear, off and on again
@pytest.mark.parametrize("log_on", [False, True])
def test_lifecycle(log_on):
    room, A, N, E = ENGINES["group"][:4]
    nbh = "moore"
    on = ("on", "keep") if log_on else ("on",)
    ops = (("step", 20), on, ("mark",), ("step", 100), ("mark",), ("step", 60), ("mark",), ("step", 20),
           on, ("mark",), ("step", 60))
    (_, w1, w2, _, w4), _, _ = M.plain("group", nbh, ops)
    assert w1["events"] > 0 and w2["events"] > 0 and w4["events"] > 0
    eng = _engine(room, A, N, nbh, E)
    ref = _engine(room, A, N, nbh, E)
    try:
        if log_on:
            eng.set_episode_log(hist_bins=32)            # ep_start is there when the feature comes on
        for g in (eng, ref):
            g.reset()
            g.step(20)
        assert eng.motion_stats_info() == "off"
        with pytest.raises(ValueError):
            eng.motion_stats()
        eng.set_motion_stats(**_mo3(E))
        for g in (eng, ref):
            g.step(100)
        _assert_motion(eng.motion_stats(), w1, nbh)
        _assert_motion(eng.motion_stats(clear=True), w1, nbh)        # a read clears nothing by itself
        for g in (eng, ref):
            g.step(60)
        _assert_motion(eng.motion_stats(), w2, nbh)                  # counted from the clear; the origins stayed
        eng.set_motion_stats(n_classes=0)
        assert eng.motion_stats_info() == "off"
        with pytest.raises(ValueError):
            eng.motion_stats()
        for g in (eng, ref):
            g.step(20)
        eng.set_motion_stats(**_mo3(E))
        for g in (eng, ref):
            g.step(60)
        _assert_motion(eng.motion_stats(), w4, nbh)
        eng.reset()                                                  # clears nothing
        ref.reset()
        _assert_motion(eng.motion_stats(), w4, nbh)
        _assert_same_state(_state(eng), _state(ref))
    finally:
        eng.close()
        ref.close()


# 7. per-env rooms: rooms of 1, 2, 3 and 4 exit cells, env e in room e % 4, the class is the room
ROOM_FORMS = {
    "lane": (("X1", "X2", "X3", "X4"), 32, 32, -2, None, "lane"),
    "group": (("X1", "X2", "X3", "X4"), 32, 32, 0, "group", "group"),
    "block": (("Y1", "Y2", "Y3", "Y4"), 16, 10, 0, "block", "block"),
}


@pytest.mark.parametrize("form", sorted(ROOM_FORMS))
def test_env_rooms(form):
    rooms, A, N, epb, kernel, runs_on = ROOM_FORMS[form]
    E, T, nbh = 36, 300, "moore"
    roe = tuple(e % 4 for e in range(E))
    (w,), _, _ = M.motion(rooms, roe, A, nbh, (PAR + (N,),), (0,) * E, (("step", T),), roe, 4)
    eng = _engine(rooms[0], A, N, nbh, E, epb=epb)
    try:
        eng.set_env_rooms([X.room(r) for r in rooms], np.asarray(roe, np.int32), kernel=kernel)
        assert eng.launch_info()["kernel"] == runs_on and eng.launch_info()["env_rooms"] == 4
        eng.set_motion_stats(classes=roe, curve_bins=BINS)
        assert eng.motion_stats_info()["classes"] == 4
        eng.reset()
        eng.step(T)
        _assert_motion(eng.motion_stats(), w, nbh)
    finally:
        eng.close()


def test_env_rooms_with_params_and_refusal():
    """Crossed with set_env_params; set_env_rooms while the feature is on is refused and changes nothing."""
    rooms, A, E, T, nbh = ("X1", "X2", "X3", "X4"), 32, 40, 400, "moore"
    roe = tuple(e % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    ops = (("step", 250), ("mark",), ("step", T - 250))
    (wa, wb), _, _ = M.motion(rooms, roe, A, nbh, SETS5, soe, ops, roe, 4)
    eng = _engine(rooms[0], A, 3, nbh, E, epb=-2)
    try:
        eng.set_env_rooms([X.room(r) for r in rooms], np.asarray(roe, np.int32))
        eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32))
        eng.set_motion_stats(classes=roe, curve_bins=BINS)
        eng.reset()
        eng.step(250)
        _assert_motion(eng.motion_stats(clear=True), wa, nbh)
        before = eng.launch_info(), eng.motion_stats_info()
        with pytest.raises(ValueError):
            eng.set_env_rooms([X.room(r) for r in rooms[:2]], np.asarray([e % 2 for e in range(E)], np.int32))
        with pytest.raises(ValueError):
            eng.set_env_rooms(None)
        assert (eng.launch_info(), eng.motion_stats_info()) == before
        eng.step(T - 250)
        _assert_motion(eng.motion_stats(), wb, nbh)
    finally:
        eng.close()


def test_mt_engines_are_refused():
    eng = _engine("T12", 8, 8, "moore", 3, rng="mt")
    try:
        before = eng.launch_info()
        with pytest.raises(NotImplementedError):
            eng.set_motion_stats()
        assert eng.launch_info() == before and eng.motion_stats_info() == "off"
    finally:
        eng.close()


def test_bad_arguments_change_nothing():
    room, A, N, E, T = ENGINES["group"][:5]
    cls = X.cls3(E)
    (w,), _, _ = M.plain("group", "moore")
    eng = _engine(room, A, N, "moore", E)
    try:
        eng.set_motion_stats(**_mo3(E))
        eng.reset()
        eng.step(120)
        before = eng.launch_info(), eng.motion_stats_info()
        bad = np.asarray(cls, np.int32).copy()
        bad[E - 1] = 3
        for kw in (dict(classes=bad, n_classes=3), dict(classes=-bad, n_classes=3), dict(classes=cls, n_classes=3, curve_bins=-1),
                   dict(classes=cls, n_classes=-2), dict(classes=cls[:-1], n_classes=3),
                   dict(classes=cls, n_classes=1 << 20, curve_bins=1 << 12)):       # beyond FFM_MOTION_STATS_MAX_BYTES
            with pytest.raises(ValueError):
                eng.set_motion_stats(**kw)
            assert (eng.launch_info(), eng.motion_stats_info()) == before
        eng.step(T - 120)
        _assert_motion(eng.motion_stats(), w, "moore")   # still counting into the tables it had
    finally:
        eng.close()


# 8. the step index wraps inside the run: tau is a wrapping difference
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_step_index_wrap(nbh):
    t0, E = (1 << 32) - 20, 7
    (w,), _, _ = M.plain("group", nbh, (("step", 60),), t0=t0, E=E)
    assert w["before_wrap"] > 0 and w["after_wrap"] > 0
    (got,), on = _run_plain("group", nbh, (("step", 60),), t0=t0, chunk=13, E=E)
    assert on["t"] == (t0 + 61) & M32 < 100
    _assert_motion(got, w, nbh)


# 9. more than one chunk of agents: 512 agents in a 64x64 room, the global form by size
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_many_agents(nbh):
    E, A = 3, 512
    (w,), _, _ = M.motion(("R64",), (0,) * E, A, nbh, (PAR + (A,),), (0,) * E, (("step", 120),), X.cls3(E), 3, False)
    assert w["chunk_shift"] > 0
    eng = _engine("R64", A, A, nbh, E, auto=False)
    try:
        eng.set_motion_stats(**_mo3(E))
        assert eng.motion_stats_info()["form"] == "global"
        eng.reset()
        eng.step(120)
        got = eng.motion_stats()
        _assert_motion(got, w, nbh)
        assert int(got["egress_count"].sum()) == eng.counters()["exits"]
    finally:
        eng.close()
