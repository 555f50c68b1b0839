"""Exit flow on the device (ffm_engine_set_exit_flow): per-door usage and outflow curves.

The expected arrays come from the oracle mirror of tests/exit_flow_mirror.py, which finds the
leavers by the sequential order-preserving walk, not by the kernel's set rule; the device's
`exited` and `outflow` must equal them exactly.  tests/test_exit_flow_mirror.py pins on the CPU
that every case here is not vacuous; the checks that cost nothing are repeated.
"""
import ctypes as C

import numpy as np
import pytest

import exit_flow_mirror as X
from env_sweep_util import SETS5, _dicts
from exit_flow_mirror import BINS, ENGINES, M32, PAR

import env_sweep_util as U

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS", "FFM_GROUP_ONE", "FFM_FIELD_STATS_FORM",
            "FFM_FIELD_STATS_SLOTS", "FFM_FIELD_STATS_BLOCKS", "FFM_EXIT_FLOW_FORM", "FFM_EXIT_FLOW_BLOCKS")


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


def _drive(eng, ops, xf, t0=0, chunk=None):
    """reset() at step index t0, then the ops; xf = dict of set_exit_flow's arguments or None (feature off:
    "on" is skipped).  Without an ("on",) op the feature is set before the reset.  chunk: steps per step() call."""
    if xf is not None and ("on",) not in ops:
        eng.set_exit_flow(**xf)
    eng.step_index = t0 & M32                            # (also for a second run in the same engine)
    eng.reset()
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
        elif op[0] == "on" and xf is not None:
            eng.set_exit_flow(**xf)


def _assert_flow(got, w, doors=None):
    for k in ("exited", "outflow"):
        assert got[k].dtype == np.uint64 and got[k].shape == w[k].shape, (k, got[k].shape, w[k].shape)
        assert np.array_equal(got[k], w[k]), k
    if got["outflow"].shape[2]:
        assert np.array_equal(got["outflow"].sum(axis=2), got["exited"])
        assert not got["outflow"][:, :, 0].any()            # tau >= 1 always
    if doors is not None:
        assert got["door_of_cell"].dtype == np.int32 and np.array_equal(got["door_of_cell"], doors)


def _xf3(E):
    return dict(classes=X.cls3(E), n_classes=3, curve_bins=BINS)


def _run_plain(name, nbh, ops=None, auto=True, t0=0, on=True, chunk=None, fused=1, check=None, E=None):
    """An engine of ENGINES under ops (default: T steps); classes e % 3, BINS bins.  Returns (flow, state)."""
    room, A, N, E0, T, epb, kernel = ENGINES[name]
    E = E or E0
    ops = ops or (("step", T),)
    eng = _engine(room, A, N, nbh, E, auto, epb)
    try:
        assert eng.launch_info()["kernel"] == kernel
        if fused > 1:
            eng.set_fused_steps(fused)
        _drive(eng, ops, _xf3(E) if on else None, t0, chunk)
        if check is not None:
            check(eng.launch_info())
        return (eng.exit_flow() if on else None), _state(eng)
    finally:
        eng.close()


# 1. every step kernel, both neighbourhoods; the step itself does not change
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_every_step_kernel(name, nbh):
    (w,), eps, doors = X.plain(name, nbh)
    X.assert_not_vacuous(w, eps)
    got, on = _run_plain(name, nbh, chunk=7)
    _assert_flow(got, w, doors)
    _, off = _run_plain(name, nbh, chunk=7, on=False)
    _assert_same_state(on, off)


# 2. no auto-reset: everybody leaves exactly once, and the field statistics' curve has the same slope
@pytest.mark.parametrize("name", ["group", "block"])
def test_no_auto_reset(name):
    room, A, N, E, T, epb, _ = ENGINES[name]
    (first, last), _, doors = X.plain(name, "moore", (("step", T), ("mark",), ("step", 10)), auto=False)
    assert int(first["exited"].sum()) == E * N and last["events"] == 0
    eng = _engine(room, A, N, "moore", E, auto=False, epb=epb)
    try:
        eng.set_field_stats(X.cls3(E), 3, BINS)
        eng.set_exit_flow(**_xf3(E))
        eng.reset()
        eng.step(T)
        got = eng.exit_flow()
        _assert_flow(got, first, doors)
        assert int(got["exited"].sum()) == E * N == eng.counters()["exits"]
        eng.step(10)                                     # the envs are empty: nothing more
        _assert_flow(eng.exit_flow(), first, doors)
        rem = eng.field_stats()["remaining"].astype(np.int64)
        out = got["outflow"].sum(axis=1).astype(np.int64)
        for tau in range(2, 15):
            assert np.array_equal(out[:, tau], rem[:, tau - 1] - rem[:, tau]), tau
    finally:
        eng.close()


# 3. launch geometry: the bits of case 1's group run
GEOMETRY = {
    "two_shards": (dict(FFM_STEP_SHARDS=2), dict(step_shards=2), {}),
    "group_envs_4": (dict(FFM_GROUP_ENVS=4), dict(group_g=4), {}),
    "global_form": (dict(FFM_EXIT_FLOW_FORM="global"), {}, dict(form="global")),
    "one_block": (dict(FFM_EXIT_FLOW_BLOCKS=1), {}, dict(form="lds", blocks=1)),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(monkeypatch, case):
    env, info, flow_info = GEOMETRY[case]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))

    def check(li):
        for k, v in info.items():
            assert li[k] == v, (k, li)
        xf = li["exit_flow"]
        assert xf["classes"] == 3 and xf["doors"] == 3 and xf["curve_bins"] == BINS and xf["slots"] >= 1
        for k, v in flow_info.items():
            assert xf[k] == v, (k, li)
    (w,), _, doors = X.plain("group", "moore")
    got, _ = _run_plain("group", "moore", chunk=50, check=check)     # step(n > 1): the shards are in effect
    _assert_flow(got, w, doors)


def test_fused_steps_setting():
    """With the feature on the fused path is not taken: the same flow, and the state of a fused engine
    with the feature off."""
    def check(li):
        assert li["multi"], li
    (w,), _, doors = X.plain("group", "moore")
    got, on = _run_plain("group", "moore", chunk=50, fused=4, check=check)
    _assert_flow(got, w, doors)
    _, off = _run_plain("group", "moore", chunk=50, fused=4, on=False, check=check)
    _assert_same_state(on, off)


def test_lds_form_refused_beyond_the_budget(monkeypatch):
    """200 classes x 3 doors x 129 words are 310 KB as u32: the global form by itself; forcing lds raises."""
    room, A, N, E = ENGINES["group"][:4]
    eng = _engine(room, A, N, "moore", E)
    try:
        eng.set_exit_flow(classes=X.cls3(E), n_classes=200, curve_bins=128)
        assert eng.launch_info()["exit_flow"]["form"] == "global"
        before = eng.launch_info()
        monkeypatch.setenv("FFM_EXIT_FLOW_FORM", "lds")
        with pytest.raises(ValueError):
            eng.set_exit_flow(classes=X.cls3(E), n_classes=200, curve_bins=128)
        assert eng.launch_info() == before
    finally:
        eng.close()


# 4. door labels: a 4-wide exit as four doors and as one
def test_door_labels():
    E, T, nbh = 37, 300, "moore"
    args = (("X4",), (0,) * E, 32, nbh, (PAR + (32,),), (0,) * E, (("step", T),), X.cls3(E), 3)
    (w4,), _, doors4 = X.flow(*args)
    (w1,), _, doors1 = X.flow(*args, labels=((0,) * 144,))
    assert (w4["exited"] > 0).all()
    eng = _engine("X4", 32, 32, nbh, E)
    try:
        _drive(eng, (("step", T),), _xf3(E))
        got4 = eng.exit_flow()
        _assert_flow(got4, w4, doors4)
        assert eng.launch_info()["exit_flow"]["doors"] == 4
        _drive(eng, (("step", T),), dict(doors=np.zeros((12, 12), np.int32), **_xf3(E)))
        got1 = eng.exit_flow()
        _assert_flow(got1, w1, doors1)
        assert eng.launch_info()["exit_flow"]["doors"] == 1
        assert np.array_equal(got4["exited"].sum(axis=1, keepdims=True), got1["exited"])
        # the C call reads the same labels back
        doc = np.zeros((1, 12, 12), np.int32)
        nd = C.c_int32()
        assert eng._L.ffm_engine_get_exit_doors(eng._h, doc.ctypes.data_as(C.c_void_p), C.byref(nd)) == 0
        assert nd.value == 1 and np.array_equal(doc, got1["door_of_cell"])
        # a label out of range is refused and changes nothing
        before = eng.launch_info()
        bad = np.zeros((12, 12), np.int32)
        bad[0, 5] = -1                                   # an exit cell
        with pytest.raises(ValueError):
            eng.set_exit_flow(doors=bad, **_xf3(E))
        lab = np.zeros(144, np.int32)
        lab[5] = 2
        from ffm_amd.engine import E_INVALID
        assert eng._L.ffm_engine_set_exit_flow(eng._h, lab.ctypes.data_as(C.c_void_p), 2, None, 1, 0, None) == E_INVALID
        assert eng._L.ffm_engine_set_exit_flow(eng._h, lab.ctypes.data_as(C.c_void_p), 256, None, 1, 0, None) == E_INVALID
        assert eng.launch_info() == before
        _assert_flow(eng.exit_flow(), w1, doors1)
        ok = np.full((12, 12), 7, np.int32)              # entries off the exits are not read
        ok[0, 4:8] = (1, 0, 0, 1)
        eng.set_exit_flow(doors=ok, **_xf3(E))
        assert np.array_equal(eng.exit_flow()["door_of_cell"][0, 0, 4:8], (1, 0, 0, 1))
        assert (eng.exit_flow()["door_of_cell"] >= 0).sum() == 4
    finally:
        eng.close()


# 5. per-env rooms: rooms of 1, 2, 3 and 4 exit cells, env e in room e % 4, the class is the room
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
    (w,), _, doors = X.flow(rooms, roe, A, nbh, (PAR + (N,),), (0,) * E, (("step", T),), roe, 4)
    for r in range(4):
        assert (w["exited"][r, :r + 1] > 0).all() and not w["exited"][r, r + 1:].any()
    eng = _engine(rooms[0], A, N, nbh, E, epb=epb)
    try:
        eng.set_env_rooms([X.room(r) for r in rooms], np.asarray(roe, np.int32), kernel=kernel)
        assert eng.launch_info()["kernel"] == runs_on and eng.launch_info()["env_rooms"] == 4
        eng.set_exit_flow(classes=roe, curve_bins=BINS)
        assert eng.launch_info()["exit_flow"]["doors"] == 4 and eng.launch_info()["exit_flow"]["classes"] == 4
        eng.reset()
        eng.step(T)
        _assert_flow(eng.exit_flow(), w, doors)
    finally:
        eng.close()


def test_env_rooms_with_params_and_refusal():
    """Crossed with set_env_params; set_env_rooms while the flow is on is refused and changes nothing."""
    rooms, A, E, T, nbh = ("X1", "X2", "X3", "X4"), 32, 40, 400, "moore"
    roe = tuple(e % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    ops = (("step", 250), ("mark",), ("step", T - 250))
    (wa, wb), _, doors = X.flow(rooms, roe, A, nbh, SETS5, soe, ops, roe, 4)
    eng = _engine(rooms[0], A, 3, nbh, E, epb=-2)
    try:
        eng.set_env_rooms([X.room(r) for r in rooms], np.asarray(roe, np.int32))
        eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32))
        eng.set_exit_flow(classes=roe, curve_bins=BINS)
        eng.reset()
        eng.step(250)
        _assert_flow(eng.exit_flow(clear=True), wa, doors)
        before = eng.launch_info()
        with pytest.raises(ValueError):
            eng.set_env_rooms([X.room(r) for r in rooms[:2]], np.asarray([e % 2 for e in range(E)], np.int32))
        with pytest.raises(ValueError):
            eng.set_env_rooms(None)
        assert eng.launch_info() == before
        eng.step(T - 250)
        _assert_flow(eng.exit_flow(), wb, doors)
    finally:
        eng.close()


# 6. whoever writes pos, cnt or ep_start refreshes the snapshot
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_snapshot_refresh(nbh):
    room, A, N, E = ENGINES["group"][:4]
    every = (1,) * E
    third = tuple(int(e % 3 == 0) for e in range(E))
    for mask in (every, third):
        ops = (("step", 30), ("reset_envs", mask), ("mark",), ("step", 1), ("mark",), ("step", 29))
        (w0, w1, w2), _, doors = X.plain("group", nbh, ops)
        assert w1["tau1"] > 0                            # agents placed next to a door leave with tau = 1
        eng = _engine(room, A, N, nbh, E)
        try:
            eng.set_exit_flow(**_xf3(E))
            eng.reset()
            eng.step(30)
            eng.reset_envs(np.asarray(mask, np.uint8))
            _assert_flow(eng.exit_flow(clear=True), w0, doors)
            eng.step(1)
            _assert_flow(eng.exit_flow(clear=True), w1, doors)
            eng.step(29)
            _assert_flow(eng.exit_flow(), w2, doors)
        finally:
            eng.close()
    ops = (("step", 30), ("set_state", X.ring_state(E, A)), ("step", 30))
    (w,), _, doors = X.plain("group", nbh, ops)
    got, _ = _run_plain("group", nbh, ops)
    _assert_flow(got, w, doors)


# 7. lifecycle: on mid-run, clear, off and on again, a caller's stream with everything else on
def test_lifecycle():
    room, A, N, E = ENGINES["group"][:4]
    nbh = "moore"
    ops = (("step", 20), ("on",), ("mark",), ("step", 100), ("mark",), ("step", 60), ("mark",), ("step", 20),
           ("on",), ("mark",), ("step", 60))
    (_, w1, w2, _, w4), _, doors = X.plain("group", nbh, ops)
    assert w1["events"] > 0 and w2["events"] > 0 and w4["events"] > 0
    eng = _engine(room, A, N, nbh, E)
    ref = _engine(room, A, N, nbh, E)
    try:
        for g in (eng, ref):
            g.reset()
            g.step(20)
        assert eng.launch_info()["exit_flow"] == "off"
        with pytest.raises(ValueError):
            eng.exit_flow()
        eng.set_exit_flow(**_xf3(E))
        for g in (eng, ref):
            g.step(100)
        _assert_flow(eng.exit_flow(), w1, doors)
        _assert_flow(eng.exit_flow(clear=True), w1, doors)           # a read clears nothing by itself
        for g in (eng, ref):
            g.step(60)
        _assert_flow(eng.exit_flow(), w2, doors)                     # counted from the clear
        eng.set_exit_flow(n_classes=0)
        assert eng.launch_info()["exit_flow"] == "off"
        with pytest.raises(ValueError):
            eng.exit_flow()
        for g in (eng, ref):
            g.step(20)
        eng.set_exit_flow(**_xf3(E))
        for g in (eng, ref):
            g.step(60)
        _assert_flow(eng.exit_flow(), w4, doors)
        eng.reset()                                                  # clears nothing
        ref.reset()
        _assert_flow(eng.exit_flow(), w4, doors)
        _assert_same_state(_state(eng), _state(ref))
    finally:
        eng.close()
        ref.close()


def test_callers_stream_with_everything_on():
    """A caller's stream, with the episode log, trajectory capture and the field statistics on."""
    room, A, N, E, T = ENGINES["group"][:5]
    nbh, sel = "moore", [0, 5, 36]
    (w,), _, doors = X.plain("group", nbh)
    st = torch.cuda.Stream()
    out = []
    for on in (True, False):
        eng = _engine(room, A, N, nbh, E)
        try:
            eng.set_episode_log(capacity=E * T, hist_bins=32, stream=st)
            eng.set_field_stats(X.cls3(E), 3, BINS, stream=st)
            if on:
                eng.set_exit_flow(stream=st, **_xf3(E))
            eng.set_trajectory_capture(sel, period=1, capacity_rows=len(sel) * (T + 8), stream=st)
            eng.reset(stream=st)
            for _ in range(T // 50):
                eng.step(50, stream=st)
            if on:
                _assert_flow(eng.exit_flow(stream=st), w, doors)
            out.append((eng.drain_episodes(stream=st), eng.field_stats(stream=st), eng.drain_trajectories(stream=st)))
        finally:
            eng.close()
    (rec, fs, rows), (rec0, fs0, rows0) = out
    assert len(rec0) >= 2 * E and np.array_equal(rec, rec0)
    assert all(np.array_equal(fs[k], fs0[k]) for k in fs0)
    assert rows.keys() == rows0.keys() and len(rows) >= 2 * len(sel)
    for k in rows:
        assert np.array_equal(rows[k][0], rows0[k][0])
        assert all(np.array_equal(p, q) for p, q in zip(rows[k][1], rows0[k][1]))


def test_ep_start_is_shared():
    """The flow keeps ep_start while the log and the field statistics come and go."""
    room, A, N, E, T = ENGINES["group"][:5]
    (w,), _, doors = X.plain("group", "moore")
    eng = _engine(room, A, N, "moore", E)
    try:
        eng.set_exit_flow(**_xf3(E))
        eng.set_episode_log(hist_bins=32)
        eng.set_field_stats(X.cls3(E), 3, BINS)
        eng.reset()
        eng.step(100)
        eng.set_episode_log(0, 0)
        eng.step(100)
        eng.set_field_stats(n_classes=0)
        eng.step(T - 200)
        _assert_flow(eng.exit_flow(), w, doors)
    finally:
        eng.close()


def test_mt_engines_are_refused():
    eng = _engine("T12", 8, 8, "moore", 3, rng="mt")
    try:
        before = eng.launch_info()
        with pytest.raises(NotImplementedError):
            eng.set_exit_flow()
        assert eng.launch_info() == before
    finally:
        eng.close()


def test_bad_arguments_change_nothing():
    room, A, N, E, T = ENGINES["group"][:5]
    cls = X.cls3(E)
    (w,), _, doors = X.plain("group", "moore")
    eng = _engine(room, A, N, "moore", E)
    try:
        eng.set_exit_flow(**_xf3(E))
        eng.reset()
        eng.step(120)
        before = eng.launch_info()
        bad = np.asarray(cls, np.int32).copy()
        bad[E - 1] = 3
        for kw in (dict(classes=bad, n_classes=3), dict(classes=-bad, n_classes=3), dict(classes=cls, n_classes=3, curve_bins=-1),
                   dict(classes=cls, n_classes=-2), dict(classes=cls[:-1], n_classes=3),
                   dict(classes=cls, n_classes=3, doors=np.zeros((2, 12, 12), np.int32)),
                   dict(classes=cls, n_classes=1 << 20, curve_bins=1 << 12)):       # beyond FFM_EXIT_FLOW_MAX_BYTES
            with pytest.raises(ValueError):
                eng.set_exit_flow(**kw)
            assert eng.launch_info() == before
        eng.step(T - 120)
        _assert_flow(eng.exit_flow(), w, doors)          # still counting into the tables it had
    finally:
        eng.close()


# 8. the step index wraps inside the run: tau is a wrapping difference
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_step_index_wrap(nbh):
    t0, E = (1 << 32) - 20, 7
    (w,), _, doors = X.plain("group", nbh, (("step", 60),), t0=t0, E=E)
    assert w["before_wrap"] > 0 and w["after_wrap"] > 0
    got, on = _run_plain("group", nbh, (("step", 60),), t0=t0, chunk=13, E=E)
    assert on["t"] == (t0 + 61) & M32 < 100
    _assert_flow(got, w, doors)


# 9. more than one chunk of agents: 512 agents in a 64x64 room
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_many_agents(nbh):
    E, A = 3, 512
    (w,), _, doors = X.flow(("R64",), (0,) * E, A, nbh, (PAR + (A,),), (0,) * E, (("step", 120),), X.cls3(E), 3, False)
    assert w["idx64"] > 0
    eng = _engine("R64", A, A, nbh, E, auto=False)
    try:
        eng.set_exit_flow(**_xf3(E))
        eng.reset()
        eng.step(120)
        got = eng.exit_flow()
        _assert_flow(got, w, doors)
        assert int(got["exited"].sum()) == eng.counters()["exits"]
    finally:
        eng.close()
