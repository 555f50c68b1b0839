"""Masked resets (reset_envs) against trajectory capture, caller streams and slot tails.

The capture rule (include/ffm_amd.h, ffm_engine_set_trajectory_capture), which the mirror below
implements from its text and not from the kernel:

* after every step a selected env e gets one row when its episode index k at the start of the
  step satisfies (k + phase) % period == 0 -- and none if it was empty before the step and is
  still empty after it;
* the row's step is the number of steps since the latest of the env's current placement
  (reset, reset_envs, auto-reset) and the set_trajectory_capture call;
* count and cells are the oracle's state after the step; a step that ended the episode gives
  the empty row (before the re-placement);
* reset_envs changes no k; a masked env's steps restart at 1 and an emptied one logs again.

The engine runs the same ops script as the mirror and drains at the same points (always before
a reset_envs: the drain sorts by (env, k, step)).  Every comparison is exact, and every case
first asserts on the oracle's own output that the workload does what the case is about.

ops: ("step", n) | ("reset_envs", mask) | ("reset",) | ("capture", sel, period, phases) |
     ("drain",) | ("sets", sets)
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 13
H = W = 12
E37 = 37                                   # the last lane pair and the last group are ragged
SEL = (0, 6, 18, 26, 28, 36)
BASE = (3, 1, 0.2, 0.2)                    # k_S, k_D, diffuse, decay
KEYS = ("k_S", "k_D", "diffuse", "decay", "n_agents")
KERNEL_OF = {0: "group", -3: "group", -2: "lane", -1: "wave", 3: "block"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def _room(h=H, w=W):
    from ffm_amd.data import make_room, l1_sff
    m = make_room(h, w)
    return m, l1_sff(m)


def _params(st, nbh):
    return {"k_S": st[0], "k_D": st[1], "diffuse": st[2], "decay": st[3], "neighborhood": nbh}


def _mask(E, f):
    return tuple(int(bool(f(e))) for e in range(E))


# ---------------------------------------------------------------------------
# The mirror: the oracle stepped under the ops, rows by the rule above.
# Returns (drains, snaps): per ("drain",) the rows (global env, k, step, count, cells) logged
# since the previous one, and the oracle's counts / episode counters at that point.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mirror(nbh, E, N, ops, auto=True, env_base=0):
    from oracle import oracle as O
    m, s = _room()
    cores = {}

    def core(st):
        if st[:4] not in cores:
            cores[st[:4]] = O.Core(m, s, _params(st, nbh))
        return cores[st[:4]]

    A = N
    cur = [BASE + (N,)] * E
    pos = np.full((E, A), 0xFFFF, np.uint16)
    cnt = np.zeros(E, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    since = np.zeros(E, np.int64)          # steps since the env's placement or the capture call
    sel, period, phases = (), 1, ()
    t, rows, drains, snaps = 0, [], [], []

    def place(e):                          # keyed by the step index, which the caller advances
        n = cur[e][4]
        pos[e] = 0xFFFF
        pos[e, :n] = core(cur[e]).reset_philox(n, SEED, t, env_base + e)
        cnt[e] = n
        dff[e] = 0.0
        since[e] = 0

    for op in ops:
        if op[0] == "reset":
            eps[:] = 0
            for e in range(E):
                place(e)
            t += 1
        elif op[0] == "reset_envs":        # no k changes
            for e in np.flatnonzero(np.asarray(op[1])):
                place(e)
            t += 1
        elif op[0] == "sets":              # parameters now, N at the env's next placement
            cur = [tuple(op[1][e % len(op[1])]) for e in range(E)]
        elif op[0] == "capture":
            sel, period = tuple(op[1]), op[2]
            phases = tuple(op[3]) if op[3] is not None else (0,) * len(sel)
            since[:] = 0
            rows = []
        elif op[0] == "step":
            for _ in range(op[1]):
                k0, c0 = eps.copy(), cnt.copy()
                if len(set(cur)) == 1:
                    core(cur[0]).step_philox_batch(pos, cnt, dff, eps, SEED, t, auto, cur[0][4], env_base, 8)
                else:
                    for e in range(E):
                        core(cur[e]).step_philox_batch(pos[e:e + 1], cnt[e:e + 1], dff[e:e + 1], eps[e:e + 1], SEED,
                                                       t, auto, cur[e][4], env_base + e, 1)
                for e, ph in zip(sel, phases):
                    ended = eps[e] != k0[e]
                    rc = 0 if ended else int(cnt[e])
                    if c0[e] == 0 and rc == 0:
                        continue
                    since[e] += 1
                    if (int(k0[e]) + ph) % period == 0:
                        rows.append((env_base + e, int(k0[e]), int(since[e]), rc, tuple(pos[e, :rc].tolist())))
                    if ended:
                        since[e] = 0       # the auto-reset placed the next episode
                t += 1
        elif op[0] == "drain":
            drains.append(tuple(rows))
            rows = []
            snaps.append({"cnt": cnt.copy(), "eps": eps.copy()})
        else:
            raise ValueError(op)
    return tuple(drains), tuple(snaps)


def _grouped(rows):
    """Rows in drain_trajectories()' form: {(global env, k): (steps, positions)}."""
    out = {}
    for g, k, st, rc, cells in sorted(rows, key=lambda r: r[:3]):
        cc = np.asarray(cells, np.int32).reshape(-1)
        steps, ps = out.setdefault((g, k), ([], []))
        steps.append(st)
        ps.append(np.stack([cc // W, cc % W], axis=1))
    return out


def _raw(rows, A):
    """Rows as the drain's raw arrays, sorted by (env, k, step): meta [n, 4], cells [n, A]."""
    rows = sorted(rows, key=lambda r: r[:3])
    meta = np.asarray([r[:4] for r in rows], np.int32).reshape(-1, 4)
    cells = np.full((len(rows), A), 0xFFFF, np.uint16)
    for i, r in enumerate(rows):
        cells[i, :r[3]] = r[4]
    return meta, cells


# ---------------------------------------------------------------------------
# The engine under the same ops
# ---------------------------------------------------------------------------
def _engine(nbh, E, N, auto=True, env_base=0, epb=0):
    from ffm_amd.engine import Engine
    m, s = _room()
    return Engine(m, s, n_envs=E, n_agents=N, params=_params(BASE, nbh), rng="philox", seed=SEED, auto_reset=auto,
                  env_base=env_base, envs_per_block=epb)


def _drain_raw(eng, cap):
    """ffm_engine_drain_trajectory itself: (meta, cells, dropped), sorted by (env, k, step)."""
    meta = np.full((cap, 4), -1, np.int32)
    cells = np.zeros((cap, eng.A), np.uint16)
    n, dropped = C.c_int64(), C.c_int64()
    rc = eng._L.ffm_engine_drain_trajectory(eng._h, meta.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                                            cap, C.byref(n), C.byref(dropped), None)
    assert rc == 0, eng._L.ffm_last_error()
    meta, cells = meta[:n.value], cells[:n.value]
    order = np.lexsort((meta[:, 2], meta[:, 1], meta[:, 0]))
    return meta[order], cells[order], int(dropped.value)


def _run(eng, ops, raw=False):
    drains = []
    for op in ops:
        if op[0] == "step":
            eng.step(op[1])
        elif op[0] == "reset":
            eng.reset()
        elif op[0] == "reset_envs":
            eng.reset_envs(np.asarray(op[1], np.uint8))
        elif op[0] == "sets":
            eng.set_env_params([dict(zip(KEYS, st)) for st in op[1]])
        elif op[0] == "capture":
            eng.set_trajectory_capture(np.asarray(op[1], np.int32), period=op[2], phases=op[3])
        elif op[0] == "drain":
            drains.append(_drain_raw(eng, eng._traj_cap) if raw else eng.drain_trajectories())
        else:
            raise ValueError(op)
    return drains


def _assert_rows(got, want_rows, what):
    want = _grouped(want_rows)
    assert sorted(got) == sorted(want), f"{what}: (env, k) keys {sorted(got)} != {sorted(want)}"
    for key, (st, ps) in want.items():
        assert got[key][0] == st, f"{what} {key}: steps {got[key][0]} != {st}"
        assert len(got[key][1]) == len(ps), f"{what} {key}: row count"
        for i, (a, b) in enumerate(zip(got[key][1], ps)):
            assert np.array_equal(a, b), f"{what} {key}: positions of step {st[i]}"


def _final_counts(eng, snap):
    _, cnt, _ = eng.get_state()
    assert np.array_equal(cnt, snap["cnt"]), "final counts"


def _script(steps0, mask, steps1, sel=SEL, period=1, phases=None):
    return (("capture", tuple(sel), period, phases), ("reset",), ("step", steps0), ("drain",),
            ("reset_envs", mask), ("step", steps1), ("drain",))


def _segment(rows, g):
    return [r for r in rows if r[0] == g]


# ---------------------------------------------------------------------------
# Case 1 (and 3): a masked reset in the middle of an episode, auto_reset on
# ---------------------------------------------------------------------------
THIRD = _mask(E37, lambda e: e % 3 == 0)
OPS1 = _script(25, THIRD, 80)


def _assert_case1_workload(drains, snaps, sel, mask, env_base=0):
    """The oracle's own output: nothing ended before the reset, every masked selected env and
    an unmasked one end an episode after it; the masked envs' second segment restarts at
    step 1 under the k they had and runs down to the empty row."""
    # (of the selected envs: with Moore moves three other envs are through their first episode)
    assert (snaps[0]["eps"][list(sel)] == 0).all(), "a selected env's episode ended before the masked reset"
    assert (snaps[0]["cnt"] > 0).all()
    masked = [e for e in sel if mask[e]]
    unmasked = [e for e in sel if not mask[e]]
    assert masked and unmasked
    assert all(snaps[1]["eps"][e] >= 1 for e in masked), "a masked selected env ended no episode"
    assert any(snaps[1]["eps"][e] >= 1 for e in unmasked), "no unmasked selected env ended an episode"
    for e in masked:
        seg = [r for r in _segment(drains[1], env_base + e) if r[1] == 0]
        assert [r[2] for r in seg] == list(range(1, len(seg) + 1)) and seg[-1][3] == 0 and len(seg) > 1
        assert all(r[3] > 0 for r in seg[:-1])
    for e in unmasked:                      # their step count runs on across the reset
        assert _segment(drains[1], env_base + e)[0][2] == 26


def _case1(nbh, epb, fused=1):
    want, snaps = _mirror(nbh, E37, 20, OPS1)
    _assert_case1_workload(want, snaps, SEL, THIRD)
    eng = _engine(nbh, E37, 20, epb=epb)
    try:
        info = eng.launch_info()
        assert info["kernel"] == KERNEL_OF[epb], info
        if epb == 3:
            assert info["K"] == 3, info
        if fused > 1:
            assert info["multi"], info
            eng.set_fused_steps(fused)
        got = _run(eng, OPS1)
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_rows(g, w, f"drain {i}")
        _final_counts(eng, snaps[1])
    finally:
        eng.close()


@pytest.mark.parametrize("nbh,epb", [("neumann", 0), ("neumann", -3), ("neumann", -2), ("neumann", -1), ("neumann", 3),
                                     ("moore", -2), ("moore", 3)])
def test_engine_capture_restarts_at_masked_reset(nbh, epb):
    """reset_envs(e % 3 == 0) at step 25 of 37 envs of 20 agents, every one of them mid-episode:
    the masked envs' rows restart at step 1 under the same k and end with the empty row, the
    unmasked envs' rows are untouched by the reset.

    Before the capture refresh in ffm_engine_reset_envs this failed with
    "drain 1 (0, 0): steps [26, 27, ...] != [1, 2, ...]" (the abandoned episode's count ran on)."""
    _case1(nbh, epb)


def test_engine_capture_masked_reset_with_fused_steps_set():
    """Case 1 on the group kernel with set_fused_steps(7): capture keeps one launch per step, the
    rows are those of the unfused run (the same mirror)."""
    _case1("neumann", 0, fused=7)


# ---------------------------------------------------------------------------
# Case 2: auto_reset off -- emptied envs are re-placed and log again
# ---------------------------------------------------------------------------
EVEN = _mask(E37, lambda e: e % 2 == 0)
# SEL is all even (all masked under e % 2 == 0): the case also needs unmasked selected envs, an
# empty one among them, so the odd envs 7, 21 and 35 join the selection
SEL2 = (0, 6, 7, 18, 21, 26, 28, 35, 36)
OPS2 = _script(25, EVEN, 40, sel=SEL2)


@pytest.mark.parametrize("epb", [0, -2])
def test_engine_capture_logs_again_after_masked_reset_without_auto_reset(epb):
    """auto_reset off, 8 agents: at step 25 most envs are empty and have stopped logging.
    reset_envs(e % 2 == 0) re-places empty and live envs alike: each logs from step 1 down to one
    empty row, then nothing; unmasked empty envs log nothing.

    Before the capture refresh this failed with "drain 1 (0, 0): steps [22, 23, ...] != [1, 2,
    ...]" -- the re-placed env 0 logged on from the count it had when it emptied."""
    want, snaps = _mirror("neumann", E37, 8, OPS2, auto=False)
    c25, c65 = snaps[0]["cnt"], snaps[1]["cnt"]
    masked = [e for e in SEL2 if EVEN[e]]
    assert any(c25[e] == 0 for e in masked), "no masked selected env was empty"
    assert any(c25[e] > 0 for e in masked), "no masked selected env was live"
    quiet = [e for e in SEL2 if not EVEN[e] and c25[e] == 0]
    assert quiet, "no unmasked selected env was empty"
    assert all(c65[e] == 0 for e in masked), "a masked selected env did not empty again"
    assert (snaps[1]["eps"] == 0).all()
    for e in masked:
        seg = _segment(want[1], e)
        assert [r[2] for r in seg] == list(range(1, len(seg) + 1)) and len(seg) > 1
        assert seg[-1][3] == 0 and all(r[3] > 0 for r in seg[:-1])
    for e in quiet:
        assert not _segment(want[1], e)
    eng = _engine("neumann", E37, 8, auto=False, epb=epb)
    try:
        assert eng.launch_info()["kernel"] == KERNEL_OF[epb]
        got = _run(eng, OPS2)
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_rows(g, w, f"drain {i}")
        _final_counts(eng, snaps[1])
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Case 4: per-env parameters (the lane kernel's per-env form)
# ---------------------------------------------------------------------------
SETS4 = ((3, 1, 0.2, 0.2, 20), (3, 0, 0.2, 0.2, 5), (3, 4, 0.2, 0.2, 17))     # env e runs set e % 3
MASK4 = _mask(E37, lambda e: e in (0, 26, 28) or e % 7 == 3)                   # a selected env of every set
OPS4 = (("sets", SETS4),) + _script(25, MASK4, 100)


def test_engine_capture_with_env_params_across_masked_reset():
    """Capture works unchanged with per-env parameters: rows carry each env's own N cells and
    0xFFFF behind them, through a masked reset and every set's auto-resets."""
    want, snaps = _mirror("neumann", E37, 20, OPS4)
    for p in range(3):
        mine = [e for e in SEL if e % 3 == p]
        assert mine and all(snaps[1]["eps"][e] >= 1 for e in mine), f"set {p}: a selected env ended no episode"
        assert any(MASK4[e] for e in mine), f"set {p}: no masked selected env"
        for e in mine:                      # each env's rows hold up to its own set's N cells
            assert max(r[3] for r in _segment(want[0] + want[1], e)) == SETS4[p][4]
    assert any(not MASK4[e] for e in SEL)
    eng = _engine("neumann", E37, 20)
    try:
        assert eng.launch_info()["kernel"] == "group"
        _run(eng, OPS4[:1])
        assert eng.launch_info()["kernel"] == "lane"
        got = _run(eng, OPS4[1:], raw=True)
        for i, ((meta, cells, dropped), w) in enumerate(zip(got, want)):
            wm, wc = _raw(w, 20)
            assert dropped == 0
            assert np.array_equal(meta, wm), f"drain {i}: meta"
            assert np.array_equal(cells, wc), f"drain {i}: cells (0xFFFF behind each row's count)"
        _final_counts(eng, snaps[1])
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Case 5: env_base -- meta[0] is the global env id
# ---------------------------------------------------------------------------
def test_engine_capture_rows_carry_global_env_ids():
    E, base, sel = 9, 1000, (0, 4, 8)
    mask = _mask(E, lambda e: e % 3 == 0)          # 0 masked, 4 and 8 not
    ops = _script(25, mask, 80, sel=sel)
    want, snaps = _mirror("neumann", E, 20, ops, env_base=base)
    assert _mirror("neumann", E, 20, ops)[0] != want, "the base must matter to the oracle's rows"
    _assert_case1_workload(want, snaps, sel, mask, env_base=base)
    eng = _engine("neumann", E, 20, env_base=base)
    try:
        got = _run(eng, ops)
        assert {k[0] for d in got for k in d} == {base + e for e in sel}
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_rows(g, w, f"drain {i}")
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Case 6: capture turned on in the middle of a run
# ---------------------------------------------------------------------------
OPS6 = (("reset",), ("step", 10), ("capture", SEL, 1, None), ("step", 60), ("drain",),
        ("capture", (), 1, None), ("step", 1), ("drain",))


@pytest.mark.parametrize("epb", [0, -2])
def test_engine_capture_turned_on_mid_run(epb):
    """The episode in flight logs from step 1 (the steps since the call) under the engine's
    current k, later episodes count from their placement; capture off drains nothing."""
    want, snaps = _mirror("neumann", E37, 20, OPS6)
    assert not want[1]
    for e in SEL:
        seg = _segment(want[0], e)
        assert seg[0][1:3] == (0, 1) and len(seg) == 60
    nxt = [[r for r in _segment(want[0], e) if r[1] == 1] for e in SEL]
    assert any(nxt), "no selected env began a later episode"
    for e, seg in zip(SEL, nxt):                 # ... which counts from its placement
        if seg:
            assert seg[0][2] == 1 and [r for r in _segment(want[0], e) if r[1] == 0][-1][3] == 0
    eng = _engine("neumann", E37, 20, epb=epb)
    try:
        assert eng.launch_info()["kernel"] == KERNEL_OF[epb]
        got = _run(eng, OPS6)
        _assert_rows(got[0], want[0], "drain 0")
        assert got[1] == {}
        _final_counts(eng, snaps[1])
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Case 7: overflow
# ---------------------------------------------------------------------------
def test_engine_capture_overflow_is_reported_and_recovers():
    """capacity_rows 10, three envs, 20 steps: 60 rows, 50 of them dropped.  drain_trajectories()
    raises and names them; the raw drain returns exactly 10 distinct rows of the mirror's 60; and
    after either drain the next 3 steps' 9 rows are complete."""
    sel = (0, 18, 36)
    ops = (("capture", sel, 1, None), ("reset",), ("step", 20), ("drain",), ("step", 3), ("drain",),
           ("step", 20), ("drain",), ("step", 3), ("drain",))
    want, _ = _mirror("neumann", E37, 20, ops)
    assert [len(w) for w in want] == [60, 9, 60, 9]
    eng = _engine("neumann", E37, 20)
    try:
        eng.set_trajectory_capture(np.asarray(sel, np.int32), period=1, capacity_rows=10)
        eng.reset()
        eng.step(20)
        with pytest.raises(RuntimeError, match=r"\b50 rows lost"):
            eng.drain_trajectories()
        eng.step(3)
        _assert_rows(eng.drain_trajectories(), want[1], "after the raising drain")
        eng.step(20)
        meta, cells, dropped = _drain_raw(eng, 10)
        assert len(meta) == 10 and dropped == 50
        wm, wc = _raw(want[2], 20)
        index = {tuple(r): i for i, r in enumerate(wm[:, :3].tolist())}
        seen = set()
        for r, c in zip(meta, cells):
            key = tuple(r[:3].tolist())
            assert key in index and key not in seen, f"row {key}: not one of the 60, or twice"
            seen.add(key)
            assert np.array_equal(r, wm[index[key]]) and np.array_equal(c, wc[index[key]]), f"row {key}"
        eng.step(3)
        meta, cells, dropped = _drain_raw(eng, 10)
        wm, wc = _raw(want[3], 20)
        assert dropped == 0 and np.array_equal(meta, wm) and np.array_equal(cells, wc)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Learner: capture across a masked reset (case 8), slot tails (case 9)
# ---------------------------------------------------------------------------
def _learner(variant, mode, E, N, A=None, maxs=30, seed=11, room=(H, W)):
    from ffm_amd.engine import Learner
    m, s = _room(*room)
    return Learner(m, s, variant, n_envs=E, n_agents=N, agent_capacity=A, mode=mode,
                   params={"epsilon": 0.1, "block_size": 1}, seed=seed, max_steps=maxs)


@pytest.mark.parametrize("variant,mode", [("actor_only", None), ("unified", "critic_only")])
def test_learner_capture_restarts_at_masked_reset(variant, mode):
    """The batched learner's capture across reset_envs on half of the envs, against the CPU
    restatement stepped in phases: a masked env's rows restart at step 1 under the same k."""
    from oracle import learn as LO
    from oracle import oracle as O
    E, N, seed, maxs = 24, 12, 11, 30
    sel = (0, 5, 10, 17, 22, 23)
    mask = _mask(E, lambda e: e % 2 == 0)
    m, s = _room()
    p = {"epsilon": 0.1, "block_size": 1}
    cpu = LO.Learn(m, s, variant, mode, p, log2_cap=20)
    sh = LO.Shard(cpu, E, N, N, seed, 0, maxs, nthreads=8)
    core = O.Core(m, s, {"neighborhood": "neumann"})

    def steps(n):
        rows = []
        for _ in range(n):
            sh.step_local()
            sh.step_apply("V")
            if sh.actor:
                sh.step_apply("H")
            for e in sel:                  # after the step, before the auto-reset re-places
                c = int(sh.counts[e])
                rows.append((e, int(sh.episodes[e]), int(sh.ep_steps[e]) + 1, c, tuple(sh.pos[e, :c].tolist())))
            sh.step_end()
        return rows

    want0 = steps(20)
    k_at, st_at = sh.episodes.copy(), sh.ep_steps.copy()
    for e in np.flatnonzero(np.asarray(mask)):          # placed with the step index, which advances
        sh.pos[e] = 0xFFFF
        sh.pos[e, :N] = core.reset_philox(N, seed, sh.t, e)
        sh.counts[e], sh.ep_steps[e] = N, 0
        sh.dff[e] = 0.0
    sh.t += 1
    want1 = steps(45)
    masked = [e for e in sel if mask[e]]
    assert masked and len(masked) < len(sel)
    assert all(st_at[e] > 0 for e in masked), "a masked selected env was not mid-episode"
    for e in masked:
        seg = _segment(want1, e)
        assert seg[0][1:3] == (int(k_at[e]), 1), "the mirror's masked env restarts at step 1, same k"
    for e in sel:
        if not mask[e]:
            assert _segment(want1, e)[0][1:3] == (int(k_at[e]), int(st_at[e]) + 1)
    assert all(sh.episodes[e] > k_at[e] for e in sel), "a selected env ended no episode after the reset"

    L = _learner(variant, mode, E, N, maxs=maxs, seed=seed)
    try:
        L.set_trajectory_capture(np.asarray(sel, np.int32), period=1)
        L.reset()
        L.step(20)
        got0 = L.drain_trajectories()
        L.reset_envs(np.asarray(mask, np.uint8))
        L.step(45)
        got1 = L.drain_trajectories()
        _assert_rows(got0, want0, "drain 0")
        _assert_rows(got1, want1, "drain 1")
        gp, gc, _ = L.get_state()
        assert np.array_equal(gc, sh.counts)
        for e in range(E):
            assert np.array_equal(gp[e, :gc[e]], sh.pos[e, :gc[e]]), f"env {e} final positions"
    finally:
        L.close()


@pytest.mark.parametrize("room", [(12, 12), (20, 20)], ids=["wave_placement", "block_placement"])
@pytest.mark.parametrize("part", ["plain", "quota", "fewer_agents"])
def test_learner_masked_reset_clears_slot_tails(part, room):
    """After reset_envs the whole position row of a masked env is its placement and 0xFFFF
    behind it (agent_capacity 20, 12 agents), like after reset(); unmasked rows are untouched.
    quota: an env past its episode quota is re-placed with no agents -- count 0, the row all
    0xFFFF.  fewer_agents: set_placement lowered the agent count to 3 before the masked reset.
    12x12 places with the wave-per-env kernel, 20x20 (324 free cells) with the workgroup one.

    Before reset_env cleared the tail this failed in the quota part with "env 0: row past its
    quota" (the finished episode's cells were still in the row) and in the fewer_agents part
    with "env 0: tail" (the abandoned episode's agents from slot 3 on); the plain part passes either way,
    no step writes behind slot 12."""
    from oracle import oracle as O
    E, N, A, seed, maxs = 24, 12, 20, 11, 30
    m, s = _room(*room)
    core = O.Core(m, s, {"neighborhood": "neumann"})
    mask = np.asarray(_mask(E, lambda e: e % 2 == 0), bool)
    caps = np.where(np.arange(E) % 4 == 0, 1, 3).astype(np.int32)
    L = _learner("unified", "critic_only", E, N, A=A, maxs=maxs, seed=seed, room=room)
    try:
        if part == "quota":
            L.set_episode_caps(caps)
        L.reset()
        L.step(35 if part == "quota" else 15)
        p0, c0, _ = L.get_state()
        eps, _ = L.episodes()
        assert len(set(c0.tolist())) > 1, "the counts must differ between envs"
        n_new = N
        if part == "quota":                       # envs 0, 4, ...: one episode done, empty since
            past = (caps == 1)
            assert (eps[past] == 1).all() and (c0[past] == 0).all() and (c0[~past] > 0).any()
        elif part == "fewer_agents":
            n_new = 3
            L.set_placement(None, n_new)
            assert (c0[mask] > n_new).all()    # live agents sit in the slots behind the new count
        t = L.step_index
        L.reset_envs(mask)
        p1, c1, _ = L.get_state()
        for e in range(E):
            if not mask[e]:
                assert c1[e] == c0[e] and np.array_equal(p1[e], p0[e]), f"env {e}: unmasked row touched"
            elif part == "quota" and caps[e] == 1:
                assert c1[e] == 0 and (p1[e] == 0xFFFF).all(), f"env {e}: row past its quota {p1[e]}"
            else:
                assert c1[e] == n_new
                assert np.array_equal(p1[e, :n_new], core.reset_philox(n_new, seed, t, e)), f"env {e}: placement"
                assert (p1[e, n_new:] == 0xFFFF).all(), f"env {e}: tail {p1[e, n_new:]}"
    finally:
        L.close()


# ---------------------------------------------------------------------------
# Case 10: the mask's upload and conversion are ordered with the caller's stream
# ---------------------------------------------------------------------------
E10, N10 = 4096, 20


@functools.lru_cache(maxsize=None)
def _placements(t):
    from oracle import oracle as O
    m, s = _room()
    core = O.Core(m, s, {"neighborhood": "neumann"})
    out = np.stack([core.reset_philox(N10, SEED, t, e) for e in range(E10)])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("kind", ["cuda_bool", "cuda_int64", "host_bool"])
@pytest.mark.parametrize("who", ["engine", "learner"])
def test_reset_envs_mask_is_converted_on_the_callers_stream(who, kind):
    """reset_envs(mask, stream=side) while torch's current stream is busy for tens of ms: the
    mask's conversion to bytes must be queued on `side`, where the reset reads it.  A conversion
    on the current stream runs after the busy work, and the reset reads the block the caching
    allocator handed it -- here freed blocks of ones, so it would re-place every env (valid
    memory: the wrong envs, nothing else).

    With the conversion on torch's current stream, one run failed with "unmasked envs were
    re-placed" in engine-cuda_int64, learner-cuda_bool and learner-cuda_int64; engine-cuda_bool,
    the process's first case, passed there (the warm-up launches below came after that run), and
    host_bool is a regression test only (its blocking upload leaves a window of microseconds)."""
    mask = np.arange(E10) % 3 == 0
    if who == "engine":
        obj = _engine("neumann", E10, N10)
    else:
        from ffm_amd.engine import Learner
        m, s = _room()
        obj = Learner(m, s, "unified", n_envs=E10, n_agents=N10, mode="critic_only", params={"block_size": 1},
                      seed=SEED, max_steps=30)
    try:
        obj.reset()                               # placements keyed by step index 0
        assert obj.step_index == 1
        torch.cuda.synchronize()
        if kind == "cuda_bool":
            mk = torch.as_tensor(mask).cuda()
        elif kind == "cuda_int64":
            mk = torch.as_tensor(mask.astype(np.int64) * 5).cuda()
        else:
            mk = mask
        side = torch.cuda.Stream()
        busy = torch.zeros(1 << 27, dtype=torch.float32, device="cuda")      # 512 MiB
        busy.add_(1.0)                            # the kernels' first launch loads them, which
        for dt in (torch.bool, torch.int64):      # would hold the host back while the busy work drains
            (torch.zeros(E10, dtype=dt, device="cuda") != 0).to(torch.uint8)
        stale = [torch.ones(E10, dtype=torch.uint8, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        del stale                                 # the allocator's next E10-byte blocks hold ones
        for _ in range(100):                      # ~1 GiB of traffic each: tens of ms in all
            busy.add_(1.0)
        obj.reset_envs(mk, stream=side)
        torch.cuda.synchronize()
        pos, cnt, _ = obj.get_state()
        assert (cnt == N10).all()
        keep, new = _placements(0), _placements(1)
        assert np.array_equal(pos[~mask], keep[~mask]), "unmasked envs were re-placed"
        assert np.array_equal(pos[mask], new[mask]), "masked envs were not re-placed"
    finally:
        obj.close()
