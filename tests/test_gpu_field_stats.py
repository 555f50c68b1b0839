"""On-device field statistics (ffm_engine_set_field_stats): occupancy maps and evacuation curves.

The expected arrays come from an oracle mirror: the oracle.Cores are stepped env by env from
reset_philox(N, seed, t0, e) with start[e] = t0, start[e] is set again at every placement (the
auto-reset: `eps` grew; reset_envs), and after the step keyed t every env with n = cnt[e] > 0 and
tau = (t - start[e]) mod 2^32 > 0 adds, with c its class and b = min(tau, bins - 1),
occupancy[c][pos[e][:n]] += 1, observed[c] += 1, remaining[c][b] += n, alive[c][b] += 1 (NumPy).
Every case first asserts on the oracle's arrays alone that it is not vacuous, then that the GPU's
four arrays equal them exactly, and the identities that tie them together.
"""
import functools

import numpy as np
import pytest

import env_sweep_util as U
from env_sweep_util import SEED, SETS5, _dicts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS", "FFM_GROUP_ONE", "FFM_FIELD_STATS_FORM",
            "FFM_FIELD_STATS_SLOTS", "FFM_FIELD_STATS_BLOCKS")
BINS = 16
PAR = (3, 1, 0.2, 0.2)
M32 = 0xFFFFFFFF
KEYS = ("occupancy", "observed", "remaining", "alive")


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


def _map(name):
    from ffm_amd.data import make_room
    if name == "R12":
        return make_room(12, 12)
    if name in ("R12W1", "R12W2", "R12W4"):
        return make_room(12, 12, exit_pos=(0, 4), exit_width=int(name[4:]))
    if name == "P14":
        return make_room(14, 14)
    if name in ("P14W1", "P14W2", "P14W4"):
        return make_room(14, 14, exit_pos=(0, 5), exit_width=int(name[4:]))
    if name == "P64":
        return make_room(64, 64)
    raise KeyError(name)


_room = U.rooms(_map)


# ---------------------------------------------------------------------------
# The oracle mirror.  rooms: names; roe / soe: per-env room / set indices; sets: (k_S, k_D, diffuse,
# decay, N) tuples.  ops: ("step", n) | ("reset_envs", mask tuple) | ("on",): the feature is set
# here (an engine whose ep_start is absent initialises it to t - 1) | ("mark",): a window boundary.
# Returns the windows between marks: lists of (pos, cnt, tau) per step launch, and eps.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(rooms, roe, A, nbh, sets, soe, ops, auto=True, t0=0):
    from oracle import oracle as O
    E = len(roe)
    H, W = _room(rooms[0])[0].shape
    cores = {}

    def core(e):
        key = (rooms[roe[e]], sets[soe[e]][:4])
        if key not in cores:
            m, s = _room(key[0])
            cores[key] = O.Core(np.array(m), np.array(s), U._params(key[1], nbh))
        return cores[key]

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
    windows, cur = [], []
    for op in ops:
        if op[0] == "step":
            for _ in range(op[1]):
                for e in range(E):
                    k0 = int(eps[e])
                    core(e).step_philox_batch(pos[e:e + 1], cnt[e:e + 1], dff[e:e + 1], eps[e:e + 1], SEED, t & M32,
                                              auto, N[e], e, 1)
                    if eps[e] != k0:                      # placed by this step's auto-reset
                        start[e] = t & M32
                cur.append((pos.copy(), cnt.copy(), ((t & M32) - start) & M32))
                t += 1
        elif op[0] == "reset_envs":
            for e in np.flatnonzero(np.asarray(op[1])):
                pos[e] = 0xFFFF
                pos[e, :N[e]] = core(e).reset_philox(N[e], SEED, t & M32, e)
                cnt[e] = N[e]
                dff[e] = 0.0
                start[e] = t & M32
            t += 1
        elif op[0] == "on":
            start[:] = (t - 1) & M32
        elif op[0] == "mark":
            windows.append(cur)
            cur = []
        else:
            raise ValueError(op)
    windows.append(cur)
    eps.setflags(write=False)
    return tuple(windows), eps


def _want(obs, cls, C, bins, HW):
    """The three rules over the step launches `obs`; also what the vacuity checks count."""
    occ = np.zeros((C, HW), np.uint64)
    observed = np.zeros(C, np.uint64)
    rem = np.zeros((C, bins), np.uint64)
    alive = np.zeros((C, bins), np.uint64)
    skipped_tau0 = skipped_empty = clamped = 0
    for pos, cnt, tau in obs:
        for e in range(len(cnt)):
            n, ta, c = int(cnt[e]), int(tau[e]), int(cls[e])
            if n == 0:
                skipped_empty += 1
                continue
            if ta == 0:
                skipped_tau0 += 1
                continue
            np.add.at(occ[c], pos[e, :n].astype(np.int64), np.uint64(1))
            observed[c] += np.uint64(1)
            if bins:
                b = min(ta, bins - 1)
                clamped += ta > bins - 1
                rem[c, b] += np.uint64(n)
                alive[c, b] += np.uint64(1)
    return {"occupancy": occ, "observed": observed, "remaining": rem, "alive": alive,
            "skipped_tau0": skipped_tau0, "skipped_empty": skipped_empty, "clamped": clamped}


def _assert_not_vacuous(want, eps, auto=True, bins=BINS, classes=None):
    obs = want["observed"] if classes is None else want["observed"][list(classes)]
    assert (obs > 0).all(), "oracle: a class was never observed"
    if auto:
        assert want["skipped_tau0"] > 0, "oracle: no state skipped for tau = 0 with agents present"
        assert (eps >= 2).all(), "oracle: an env finished fewer than two episodes"
    else:          # nothing is ever re-placed: the skipped states are the empty ones
        assert want["skipped_tau0"] == 0 and want["skipped_empty"] > 0
    if bins:
        assert want["clamped"] > 0 and (want["alive"][:, bins - 1] > 0).any(), "oracle: nothing clamped into the last bin"


def _assert_stats(got, want, rooms, roe, cls, H, W):
    C = len(want["observed"])
    assert got["occupancy"].dtype == np.uint64 and got["occupancy"].shape == (C, H, W)
    for k in KEYS:
        assert got[k].dtype == np.uint64
        assert np.array_equal(got[k].reshape(want[k].shape), want[k]), k
    occ = got["occupancy"].reshape(C, -1)
    if got["remaining"].shape[1]:
        assert np.array_equal(occ.sum(axis=1), got["remaining"].sum(axis=1))
        assert np.array_equal(got["alive"].sum(axis=1), got["observed"])
        assert not got["remaining"][:, 0].any() and not got["alive"][:, 0].any()   # tau = 0 is never observed
    # walls and exits hold nobody: in every room some env of the class stands in
    for c in range(C):
        free = np.zeros(H * W, bool)
        for e in np.flatnonzero(np.asarray(cls) == c):
            free |= (_room(rooms[roe[e]])[0] == 0).reshape(-1)
        assert not occ[c][~free].any(), f"class {c}: a wall or exit cell was counted"


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


def _engine(room, A, N, nbh, E, auto=True, epb=0, rng="philox"):
    from ffm_amd.engine import Engine
    m, s = _room(room)
    return Engine(m, s, n_envs=E, n_agents=N, agent_capacity=A, params=U._params(PAR, nbh), rng=rng, seed=SEED,
                  auto_reset=auto, envs_per_block=epb)


def _drive(eng, ops, fs, t0=0, chunk=None):
    """reset() at step index t0, then the ops; fs = (classes, C, bins) or None (feature off: "on" is skipped).
    Without an ("on",) op the feature is set before the reset.  chunk: steps per step() call."""
    if fs is not None and ("on",) not in ops:
        eng.set_field_stats(fs[0], fs[1], fs[2])
    if t0:
        eng.step_index = t0 & M32
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
        elif op[0] == "on" and fs is not None:
            eng.set_field_stats(fs[0], fs[1], fs[2])


# name: room, A, N, E, T, envs_per_block, the create-time kernel
ENGINES = {
    "group": ("R12", 32, 32, 37, 300, 0, "group"),
    "lane": ("R12", 32, 32, 37, 300, -2, "lane"),
    "wave": ("R12", 40, 40, 13, 400, 0, "wave"),
    "wave_odd": ("R12", 35, 33, 13, 400, 0, "wave"),        # rows of an odd agent capacity: no whole dwords
    "block": ("P14", 16, 10, 19, 200, 0, "block"),
}


def _cls3(E):
    return tuple(e % 3 for e in range(E))


def _plain_oracle(name, nbh, ops=None, auto=True, t0=0):
    room, A, N, E, T, _, _ = ENGINES[name]
    ops = ops or (("step", T),)
    return _oracle((room,), (0,) * E, A, nbh, (PAR + (N,),), (0,) * E, ops, auto, t0)


def _run_plain(name, nbh, ops=None, auto=True, t0=0, fs=True, chunk=None, fused=1, check=None):
    """An engine of ENGINES under ops (default: T steps); classes e % 3, BINS bins.  Returns (stats, state)."""
    room, A, N, E, T, epb, kernel = ENGINES[name]
    ops = ops or (("step", T),)
    eng = _engine(room, A, N, nbh, E, auto, epb)
    try:
        assert eng.launch_info()["kernel"] == kernel
        if fused > 1:
            eng.set_fused_steps(fused)
        _drive(eng, ops, (_cls3(E), 3, BINS) if fs else None, t0, chunk)
        if check is not None:
            check(eng.launch_info())
        return (eng.field_stats() if fs else None), _state(eng)
    finally:
        eng.close()


def _check_plain(name, nbh, got, ops=None, auto=True, t0=0):
    room, A, N, E, T, _, _ = ENGINES[name]
    (obs,), eps = _plain_oracle(name, nbh, ops, auto, t0)
    H, W = _room(room)[0].shape
    want = _want(obs, _cls3(E), 3, BINS, H * W)
    _assert_not_vacuous(want, eps, auto)
    _assert_stats(got, want, (room,), (0,) * E, _cls3(E), H, W)
    return want


# 1. every step kernel, both neighbourhoods; the step itself does not change
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_every_step_kernel(name, nbh):
    got, on = _run_plain(name, nbh, chunk=7)
    _check_plain(name, nbh, got)
    _, off = _run_plain(name, nbh, chunk=7, fs=False)
    _assert_same_state(on, off)


# 2. no auto-reset: envs empty and then add nothing
@pytest.mark.parametrize("name", ["group", "block"])
def test_no_auto_reset(name):
    T = ENGINES[name][4]
    ops = (("step", T), ("mark",), ("step", 10))
    room, A, N, E = ENGINES[name][:4]
    (first, last), eps = _plain_oracle(name, "moore", ops, auto=False)
    assert all((cnt == 0).all() for _, cnt, _ in last), "oracle: an env still holds agents"
    H, W = _room(room)[0].shape
    want = _want(first + last, _cls3(E), 3, BINS, H * W)
    _assert_not_vacuous(want, eps, auto=False)
    got, on = _run_plain(name, "moore", ops, auto=False)
    _assert_stats(got, want, (room,), (0,) * E, _cls3(E), H, W)
    _, off = _run_plain(name, "moore", ops, auto=False, fs=False)
    _assert_same_state(on, off)


# 3. launch geometry: the bits of case 1
GEOMETRY = {
    "one_shard": (dict(FFM_STEP_SHARDS=1), "group", dict(step_shards=1)),
    "two_shards": (dict(FFM_STEP_SHARDS=2), "group", dict(step_shards=2)),
    "three_shards": (dict(FFM_STEP_SHARDS=3), "group", dict(step_shards=3)),      # 16 + 16 + 5 envs
    "group_envs_4": (dict(FFM_GROUP_ENVS=4), "group", dict(group_g=4)),
    "wave_blocks_1": (dict(FFM_WAVE_BLOCKS=1), "group", dict(blocks=1)),
    "wave_blocks_1_lane": (dict(FFM_WAVE_BLOCKS=1), "lane", dict(blocks=1)),
    "loop_form": (dict(FFM_GROUP_ONE=0), "group", dict(group_one=False)),
    # the observer's own grid: runs of 4 envs (the last one partial) over 3 blocks, then a block per run
    "observer_3_blocks": (dict(FFM_FIELD_STATS_RUN=4, FFM_FIELD_STATS_BLOCKS=3, FFM_FIELD_STATS_SLOTS=2), "group",
                          dict(field_stats={"form": "lds", "blocks": 3, "slots": 2, "classes": 3, "curve_bins": BINS})),
    "observer_3_blocks_global": (dict(FFM_FIELD_STATS_RUN=4, FFM_FIELD_STATS_BLOCKS=3, FFM_FIELD_STATS_SLOTS=2,
                                      FFM_FIELD_STATS_FORM="global"), "wave_odd",
                                 dict(field_stats={"form": "global", "blocks": 3, "slots": 2, "classes": 3,
                                                   "curve_bins": BINS})),
    "observer_block_per_run": (dict(FFM_FIELD_STATS_RUN=3, FFM_STEP_SHARDS=2), "group",
                               dict(step_shards=2, field_stats={"form": "lds", "blocks": 13, "slots": 16, "classes": 3,
                                                                "curve_bins": BINS})),
    "observer_one_block": (dict(FFM_FIELD_STATS_BLOCKS=1, FFM_FIELD_STATS_RUN=5, FFM_FIELD_STATS_SLOTS=1), "wave_odd",
                           dict(field_stats={"form": "lds", "blocks": 1, "slots": 1, "classes": 3, "curve_bins": BINS})),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(monkeypatch, case):
    env, name, info = GEOMETRY[case]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))

    def check(li):
        for k, v in info.items():
            assert li[k] == v, (k, li)
    got, _ = _run_plain(name, "moore", chunk=50, check=check)     # step(n > 1): the shards are in effect
    _check_plain(name, "moore", got)


def test_fused_steps_setting():
    """With the feature on the fused path is not taken: the same statistics, and the state of a fused
    engine with the feature off."""
    def check(li):
        assert li["multi"], li
    got, on = _run_plain("group", "moore", chunk=50, fused=4, check=check)
    _check_plain("group", "moore", got)
    _, off = _run_plain("group", "moore", chunk=50, fused=4, fs=False, check=check)
    _assert_same_state(on, off)


# 4. the two forms
@pytest.mark.parametrize("name", ["group", "wave_odd"])
@pytest.mark.parametrize("form", ["lds", "global"])
def test_forms(monkeypatch, form, name):
    monkeypatch.setenv("FFM_FIELD_STATS_FORM", form)

    def check(li):
        assert li["field_stats"]["form"] == form, li
    got, _ = _run_plain(name, "moore", chunk=50, check=check)
    _check_plain(name, "moore", got)


def test_tables_beyond_the_lds_budget(monkeypatch):
    """256 classes at 12x12 with 16 bins are 181 KB as u32: the global form by itself; forcing lds raises."""
    room, A, N, E, T, epb, _ = ENGINES["group"]
    (obs,), eps = _plain_oracle("group", "moore")
    cls = tuple(100 * c for c in _cls3(E))          # classes 0, 100, 200 of 256
    want = _want(obs, cls, 256, BINS, 144)
    _assert_not_vacuous(want, eps, classes=(0, 100, 200))
    eng = _engine(room, A, N, "moore", E, epb=epb)
    try:
        assert eng.launch_info()["field_stats"] == "off"
        eng.set_field_stats(cls, 256, BINS)
        fs = eng.launch_info()["field_stats"]
        assert fs["form"] == "global" and fs["classes"] == 256 and fs["curve_bins"] == BINS and fs["blocks"] >= 1
        eng.reset()
        eng.step(T)
        _assert_stats(eng.field_stats(), want, (room,), (0,) * E, cls, 12, 12)
        before = eng.launch_info()
        monkeypatch.setenv("FFM_FIELD_STATS_FORM", "lds")
        with pytest.raises(ValueError):
            eng.set_field_stats(cls, 256, BINS)
        assert eng.launch_info() == before
        eng.set_field_stats(_cls3(E), 3, BINS)       # three classes fit
        assert eng.launch_info()["field_stats"]["form"] == "lds"
    finally:
        eng.close()


def test_large_map_several_classes():
    """64x64 with five classes (82 KB as u32) takes the global form; with two, the LDS form."""
    A, N, E, T, nbh = 300, 6, 5, 400, "moore"
    cls = tuple(range(E))
    (obs,), eps = _oracle(("P64",), (0,) * E, A, nbh, (PAR + (N,),), (0,) * E, (("step", T),))
    want = _want(obs, cls, E, BINS, 64 * 64)
    _assert_not_vacuous(want, eps)
    for C, form in ((5, "global"), (2, "lds")):
        c = tuple(x % C for x in cls)
        w = want if C == 5 else _want(obs, c, C, BINS, 64 * 64)
        eng = _engine("P64", A, N, nbh, E)
        try:
            eng.set_field_stats(c, C, BINS)
            assert eng.launch_info()["field_stats"]["form"] == form
            eng.reset()
            eng.step(T)
            _assert_stats(eng.field_stats(), w, ("P64",), (0,) * E, c, 64, 64)
        finally:
            eng.close()


# 5. sweeps: the class is the combination index
SWEEP_T = 400


@pytest.mark.parametrize("kernel", ["lane", "group"])
def test_env_params_sweep(kernel):
    A, E, nbh = 32, 35, "moore"
    soe = tuple(e % 5 for e in range(E))
    (obs,), eps = _oracle(("R12",), (0,) * E, A, nbh, SETS5, soe, (("step", SWEEP_T),))
    want = _want(obs, soe, 5, BINS, 144)
    _assert_not_vacuous(want, eps)
    assert {1, 5} <= {s[4] for s in SETS5}
    eng = _engine("R12", A, 3, nbh, E)
    try:
        eng.set_env_params(_dicts(SETS5), np.asarray(soe, np.int32), kernel=kernel)
        assert eng.launch_info()["kernel"] == kernel
        eng.set_field_stats(soe, curve_bins=BINS)    # n_classes: max + 1
        assert eng.launch_info()["field_stats"]["classes"] == 5
        eng.reset()
        eng.step(SWEEP_T)
        _assert_stats(eng.field_stats(), want, ("R12",), (0,) * E, soe, 12, 12)
    finally:
        eng.close()


ROOM_SWEEPS = {
    "lane": (("R12W1", "R12W2", "R12W4"), 32, 32, 13, 300, None, "lane"),
    "block": (("P14W1", "P14W2", "P14W4"), 16, 10, 19, 200, "block", "block"),
}


@pytest.mark.parametrize("form", sorted(ROOM_SWEEPS))
def test_env_rooms_sweep(form):
    rooms, A, N, E, T, kernel, runs_on = ROOM_SWEEPS[form]
    nbh = "moore"
    roe = tuple(e % 3 for e in range(E))
    (obs,), eps = _oracle(rooms, roe, A, nbh, (PAR + (N,),), (0,) * E, (("step", T),))
    H, W = _room(rooms[0])[0].shape
    want = _want(obs, roe, 3, BINS, H * W)
    _assert_not_vacuous(want, eps)
    # a wider exit is used: its cells' neighbours differ between the classes
    assert not np.array_equal(want["occupancy"][0], want["occupancy"][2])
    eng = _engine(rooms[0], A, N, nbh, E, epb=-2 if form == "lane" else 0)
    try:
        eng.set_env_rooms([_room(r) for r in rooms], np.asarray(roe, np.int32), kernel=kernel)
        assert eng.launch_info()["kernel"] == runs_on and eng.launch_info()["env_rooms"] == 3
        eng.set_field_stats(roe, 3, BINS)
        eng.reset()
        eng.step(T)
        _assert_stats(eng.field_stats(), want, rooms, roe, roe, H, W)
    finally:
        eng.close()


# 6. lifecycle
def _sum(*ws):
    return {k: sum(w[k] for w in ws) for k in KEYS + ("skipped_tau0", "skipped_empty", "clamped")}


def test_lifecycle():
    """On mid-run, reset_envs, clear, off and on again; the state is that of an engine without the feature."""
    room, A, N, E = ENGINES["group"][:4]
    nbh, cls = "moore", _cls3(E)
    mask = tuple(int(e % 4 == 1) for e in range(E))
    ops = (("step", 40), ("on",), ("mark",), ("step", 60), ("reset_envs", mask), ("step", 90), ("mark",),
           ("step", 70), ("mark",), ("step", 20), ("on",), ("mark",), ("step", 60))
    (_, w1, w2, _, w4), eps = _plain_oracle("group", nbh, ops)     # (the first and fourth window: feature off)
    want1, want2, want4 = (_want(w, cls, 3, BINS, 144) for w in (w1, w2, w4))
    _assert_not_vacuous(_sum(want1, want2), eps)
    # turned on mid-run: the first observed tau is 1 for every env; and again for the masked envs after reset_envs
    assert (w1[0][2] == 1).all() and (w4[0][2] == 1).all()
    m = np.asarray(mask, bool)
    assert (w1[60][2][m] == 1).all() and (w1[60][2][~m] != 1).any()
    rooms, roe = (room,), (0,) * E

    eng = _engine(room, A, N, nbh, E)
    ref = _engine(room, A, N, nbh, E)
    try:
        for g in (eng, ref):
            g.reset()
            g.step(40)
        eng.set_field_stats(cls, 3, BINS)
        for g in (eng, ref):
            g.step(60)
            g.reset_envs(np.asarray(mask, np.uint8))
            g.step(90)
        _assert_stats(eng.field_stats(), want1, rooms, roe, cls, 12, 12)
        _assert_stats(eng.field_stats(clear=True), want1, rooms, roe, cls, 12, 12)      # a read clears nothing by itself
        for g in (eng, ref):
            g.step(70)
        _assert_stats(eng.field_stats(), want2, rooms, roe, cls, 12, 12)               # counted from the clear
        eng.set_field_stats(n_classes=0)
        assert eng.launch_info()["field_stats"] == "off"
        with pytest.raises(ValueError):
            eng.field_stats()
        for g in (eng, ref):
            g.step(20)
        eng.set_field_stats(cls, 3, BINS)
        for g in (eng, ref):
            g.step(60)
        _assert_stats(eng.field_stats(), want4, rooms, roe, cls, 12, 12)
        eng.reset()                                    # clears nothing, and its placement is not observed
        ref.reset()
        _assert_stats(eng.field_stats(), want4, rooms, roe, cls, 12, 12)
        _assert_same_state(_state(eng), _state(ref))
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("name", ["group", "block"])
def test_episode_log_on_then_off(name):
    """The log and the statistics share ep_start: the records equal the log's alone, and with the log off
    again the curve still counts."""
    room, A, N, E, T, epb, _ = ENGINES[name]
    nbh, cls = "moore", _cls3(E)
    (obs,), eps = _plain_oracle(name, nbh, (("step", T + 60),))
    H, W = _room(room)[0].shape
    want = _want(obs, cls, 3, BINS, H * W)
    _assert_not_vacuous(want, eps)
    eng = _engine(room, A, N, nbh, E, epb=epb)
    ref = _engine(room, A, N, nbh, E, epb=epb)
    try:
        eng.set_field_stats(cls, 3, BINS)
        for g in (eng, ref):
            g.set_episode_log(hist_bins=32)
            g.reset()
            g.step(T)
        rec, rec_ref = eng.drain_episodes(), ref.drain_episodes()
        assert len(rec_ref) >= 2 * E and np.array_equal(rec, rec_ref)
        a, b = eng.episode_stats(), ref.episode_stats()
        assert np.array_equal(a.pop("hist"), b.pop("hist")) and a == b
        for g in (eng, ref):
            g.set_episode_log(0, 0)                    # off: the statistics keep ep_start
            g.step(60)
        _assert_stats(eng.field_stats(), want, (room,), (0,) * E, cls, H, W)
        _assert_same_state(_state(eng), _state(ref))
        # and the other way round: statistics off while the log is on keeps the log's ep_start
        for g in (eng, ref):
            g.set_episode_log(hist_bins=32)
            g.reset()
            g.step(30)
        eng.set_field_stats(n_classes=0)
        for g in (eng, ref):
            g.step(T)
        rec, rec_ref = eng.drain_episodes(), ref.drain_episodes()
        assert len(rec_ref) >= E and np.array_equal(rec, rec_ref)
    finally:
        eng.close()
        ref.close()


# 7. a caller's stream, with trajectory capture on at the same time
def test_callers_stream_with_capture():
    room, A, N, E, T = ENGINES["group"][:5]
    nbh, cls, sel = "moore", _cls3(E), [0, 5, 36]
    (obs,), eps = _plain_oracle("group", nbh)
    want = _want(obs, cls, 3, BINS, 144)
    _assert_not_vacuous(want, eps)
    st = torch.cuda.Stream()
    rows = []
    for fs in (True, False):
        eng = _engine(room, A, N, nbh, E)
        try:
            if fs:
                eng.set_field_stats(cls, 3, BINS, stream=st)
            eng.set_trajectory_capture(sel, period=1, capacity_rows=len(sel) * (T + 8), stream=st)
            eng.reset(stream=st)
            for _ in range(T // 50):
                eng.step(50, stream=st)
            if fs:
                _assert_stats(eng.field_stats(stream=st), want, (room,), (0,) * E, cls, 12, 12)
            rows.append(eng.drain_trajectories(stream=st))
        finally:
            eng.close()
    on, off = rows
    assert on.keys() == off.keys() and len(on) >= 2 * len(sel)
    for k in on:
        assert np.array_equal(on[k][0], off[k][0])
        assert all(np.array_equal(p, q) for p, q in zip(on[k][1], off[k][1]))


# 8. the step index wraps inside the run: tau is a wrapping difference
@pytest.mark.parametrize("name", ["group", "block"])
def test_step_index_wrap(name):
    t0 = (1 << 32) - 5
    got, on = _run_plain(name, "moore", t0=t0, chunk=50)
    assert on["t"] == (t0 + 1 + ENGINES[name][4]) & M32 < 1000
    want = _check_plain(name, "moore", got, t0=t0)
    # not the statistics of a run that starts at 0: the draws are keyed by t
    (obs0,), _ = _plain_oracle(name, "moore")
    E, HW = ENGINES[name][3], int(np.prod(_room(ENGINES[name][0])[0].shape))
    assert not np.array_equal(_want(obs0, _cls3(E), 3, BINS, HW)["occupancy"], want["occupancy"])


# 9. errors leave the engine as it was
def test_mt_engines_are_refused():
    eng = _engine("R12", 8, 8, "moore", 3, rng="mt")
    try:
        before = eng.launch_info()
        with pytest.raises(NotImplementedError):
            eng.set_field_stats()
        assert eng.launch_info() == before
    finally:
        eng.close()


@pytest.mark.parametrize("was_on", [False, True])
def test_bad_arguments_change_nothing(was_on):
    room, A, N, E = ENGINES["group"][:4]
    nbh, cls = "moore", _cls3(E)
    (obs,), eps = _plain_oracle("group", nbh, (("step", 300),))
    want = _want(obs, cls, 3, BINS, 144)
    eng = _engine(room, A, N, nbh, E)
    ref = _engine(room, A, N, nbh, E)
    try:
        if was_on:
            eng.set_field_stats(cls, 3, BINS)
        for g in (eng, ref):
            g.reset()
            g.step(120)
        before, state = eng.launch_info(), _state(eng)
        bad = np.asarray(cls, np.int32).copy()
        bad[E - 1] = 3
        for args in ((bad, 3, BINS), (-bad, 3, BINS), (cls, 3, -1), (cls, -2, BINS), (cls[:-1], 3, BINS)):
            with pytest.raises(ValueError):
                eng.set_field_stats(*args)
            assert eng.launch_info() == before
        _assert_same_state(_state(eng), state)
        for g in (eng, ref):
            g.step(180)
        if was_on:                                      # still counting into the tables it had
            _assert_stats(eng.field_stats(), want, (room,), (0,) * E, cls, 12, 12)
        else:
            with pytest.raises(ValueError):
                eng.field_stats()
        _assert_same_state(_state(eng), _state(ref))
    finally:
        eng.close()
        ref.close()
