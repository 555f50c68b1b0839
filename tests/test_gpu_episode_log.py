"""The core engine's evacuation-time log and on-device statistics (ffm_engine_set_episode_log).

The expected log comes from the oracle: from reset_philox(N, seed, 0, env_base + e) with
start = 0, every step t = 1.. of Core.step_philox_batch in which an env that held agents was
re-placed (auto_reset: its `eps` grew) or emptied (no auto_reset: cnt == 0) yields the record
(env_base + e, eps before, t - start[e], t), and start[e] = t.  The sorted GPU records must
equal that array exactly; the histogram and summary must equal np.bincount (lengths clamped
into the last bin) and the integer sums of its `steps` column; and the final positions, counts,
DFF bits, episode counters and the four counters must equal, bit for bit, those of the same
engine with the feature off.  Every case asserts that the oracle's log holds at least one
record per env, so an empty log cannot pass.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS")
SEED = 42
BINS = 32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _setenv(monkeypatch, **kw):
    """The switches are read when the engine is created."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def _params(nbh):
    return {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


def _room(H, W):
    from ffm_amd.data import make_room, l1_sff
    m = make_room(H, W)
    return m, l1_sff(m)


def _third(E):
    return tuple(int(e % 3 == 0) for e in range(E))


# ---------------------------------------------------------------------------
# The oracle's log.  ops: ("step", n) | ("reset_envs", mask tuple) | ("log_on",)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(H, W, N, nbh, E, ops, auto=True, env_base=0):
    from oracle import oracle as O
    m, s = _room(H, W)
    core = O.Core(m, s, _params(nbh))
    pos = np.stack([core.reset_philox(N, SEED, 0, env_base + e) for e in range(E)])
    cnt = np.full(E, N, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    start = np.zeros(E, np.int64)
    recs, t = [], 1                       # t: the next step index (reset() used 0)
    for op in ops:
        if op[0] == "step":
            for _ in range(op[1]):
                before, e0 = cnt.copy(), eps.copy()
                core.step_philox_batch(pos, cnt, dff, eps, SEED, t, auto, N, env_base, 16)
                ended = (before > 0) & ((eps > e0) if auto else (cnt == 0))
                for e in np.flatnonzero(ended):
                    recs.append((env_base + e, e0[e], t - start[e], t))
                    start[e] = t
                t += 1
        elif op[0] == "reset_envs":        # tests/test_gpu_parity.py:192-240: placed with index t, which advances
            for e in np.flatnonzero(np.asarray(op[1])):
                pos[e] = core.reset_philox(N, SEED, t, env_base + e)
                cnt[e] = N
                dff[e] = 0.0
                start[e] = t
            t += 1
        elif op[0] == "log_on":            # episodes in flight count from the steps taken after it
            recs = []
            start[:] = t - 1
    rec = np.asarray(recs, np.int64).reshape(-1, 4)
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))].astype(np.int32)
    rec.setflags(write=False)
    return rec


def _want_stats(rec, bins=BINS):
    st = rec[:, 2].astype(np.int64)
    return {"hist": np.bincount(np.minimum(st, bins - 1), minlength=bins).astype(np.uint64),
            "count": int(st.size), "sum": int(st.sum()), "sum_sq": int((st * st).sum()),
            "min": int(st.min()) if st.size else 0, "max": int(st.max()) if st.size else 0}


def _assert_stats(got, rec, bins=BINS):
    want = _want_stats(rec, bins)
    assert np.array_equal(got["hist"], want["hist"]), (got["hist"], want["hist"])
    for k in ("count", "sum", "sum_sq", "min", "max"):
        assert got[k] == want[k], (k, got[k], want[k])
    if want["count"]:
        st = rec[:, 2].astype(np.float64)
        assert got["mean"] == pytest.approx(st.mean(), rel=1e-12)
        assert got["std"] == pytest.approx(st.std(), rel=1e-9, abs=1e-9)


def _assert_covers(rec, E, env_base=0):
    assert set(rec[:, 0].tolist()) == set(range(env_base, env_base + E)), "oracle log: an env without a record"


# ---------------------------------------------------------------------------
# The engine under the same ops
# ---------------------------------------------------------------------------
def _episodes(eng):
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


def _make(H, W, N, nbh, E, auto=True, env_base=0, epb=0, rng="philox"):
    from ffm_amd.engine import Engine
    m, s = _room(H, W)
    return Engine(m, s, n_envs=E, n_agents=N, params=_params(nbh), rng=rng, seed=SEED, auto_reset=auto,
                  env_base=env_base, envs_per_block=epb)


def _drive(eng, ops, log, fused=1, check=None):
    """reset(), then the ops; log = (capacity, bins) or None (feature off)."""
    if log is not None and ("log_on",) not in ops:
        eng.set_episode_log(*log)
    if fused > 1:
        eng.set_fused_steps(fused)
    if check is not None:
        check(eng.launch_info())
    eng.reset()
    for op in ops:
        if op[0] == "step":
            eng.step(op[1])
        elif op[0] == "reset_envs":
            eng.reset_envs(np.asarray(op[1], np.uint8))
        elif op[0] == "log_on" and log is not None:
            eng.set_episode_log(*log)
    pos, cnt, dff = eng.get_state()
    return {"pos": pos, "cnt": cnt, "dff": dff, "eps": _episodes(eng), "ctr": eng.counters(), "t": eng.step_index}


def _assert_same_state(a, b):
    assert np.array_equal(a["cnt"], b["cnt"]), "counts"
    for e in range(len(a["cnt"])):
        assert np.array_equal(a["pos"][e, :a["cnt"][e]], b["pos"][e, :b["cnt"][e]]), f"env {e} positions"
    assert np.array_equal(a["dff"].view(np.uint32), b["dff"].view(np.uint32)), "DFF bits"
    assert np.array_equal(a["eps"], b["eps"]), "episodes"
    assert a["ctr"] == b["ctr"], (a["ctr"], b["ctr"])
    assert a["t"] == b["t"]


def _case(H, W, N, nbh, E, ops, auto=True, env_base=0, epb=0, fused=1, check=None, cover=True):
    """Log on against the oracle's log and statistics, and against the same engine with it off."""
    want = _oracle(H, W, N, nbh, E, ops, auto, env_base)
    if cover:
        _assert_covers(want, E, env_base)
    on = _make(H, W, N, nbh, E, auto, env_base, epb)
    a = _drive(on, ops, (None, BINS), fused, check)
    got = on.drain_episodes()
    stats = on.episode_stats()
    on.close()
    off = _make(H, W, N, nbh, E, auto, env_base, epb)
    b = _drive(off, ops, None, fused, check)
    off.close()
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    _assert_stats(stats, want)
    _assert_same_state(a, b)
    return want


def _kernel_is(name, **more):
    def check(li):
        assert li["kernel"] == name, li
        for k, v in more.items():
            assert li[k] == v, li
    return check


STEP150 = (("step", 150),)


# 1. the group kernel, both group sizes
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("N", [12, 32])
@pytest.mark.parametrize("G", [2, 4])
def test_group_kernel_log(monkeypatch, G, N, nbh, auto):
    _setenv(monkeypatch, FFM_GROUP_ENVS=G)
    want = _case(12, 12, N, nbh, 40, STEP150, auto=auto, epb=-3, check=_kernel_is("group", group_g=G))
    if not auto:
        assert len(want) == 40 and not want[:, 1].any()      # one episode per env, index 0
    if nbh == "neumann":
        assert _want_stats(want)["hist"][BINS - 1] > 0         # the overflow bin fills (lengths past 31)


# 2. step shards: one step(150) call, shards on streams of their own
@pytest.mark.parametrize("E,S", [(40, 3), (13, 2)])          # shards of 16 / 16 / 8 envs, and of 8 / 5
def test_step_shards_log(monkeypatch, E, S):
    _setenv(monkeypatch, FFM_STEP_SHARDS=3)
    _case(12, 12, 12, "neumann", E, STEP150, check=_kernel_is("group", step_shards=S))


# 3. fused multi-step launches: records carry the inner step's index
def test_fused_steps_log(monkeypatch):
    _setenv(monkeypatch)
    _case(12, 12, 12, "neumann", 40, STEP150, fused=7, check=lambda li: li["multi"] or pytest.fail(str(li)))


# 4. lane and wave kernels
@pytest.mark.parametrize("epb,name", [(-2, "lane"), (-1, "wave")])
def test_lane_and_wave_kernel_log(monkeypatch, epb, name):
    _setenv(monkeypatch)
    _case(14, 16, 20, "moore", 40, (("step", 120),), epb=epb, check=_kernel_is(name))


# 5. block kernel
def test_block_kernel_log(monkeypatch):
    _setenv(monkeypatch)
    _case(40, 40, 16, "neumann", 24, (("step", 200),), epb=1, check=_kernel_is("block"))


# 6. block kernel in global scratch, placement by workgroups
def test_block_scratch_kernel_log(monkeypatch):
    _setenv(monkeypatch)
    _case(110, 110, 6, "neumann", 8, (("step", 320),), check=_kernel_is("block_scratch"))


# 7. global env ids
@pytest.mark.parametrize("auto", [True, False])
def test_env_base_log(monkeypatch, auto):
    _setenv(monkeypatch)
    want = _case(12, 12, 12, "neumann", 40, STEP150, auto=auto, env_base=77, epb=-3)
    assert want[:, 0].min() == 77 and want[:, 0].max() == 116


# 8. a full log drops records and counts them; the statistics drop nothing
def test_overflow(monkeypatch):
    _setenv(monkeypatch)
    want = _oracle(12, 12, 12, "neumann", 40, STEP150)
    _assert_covers(want, 40)
    eng = _make(12, 12, 12, "neumann", 40)
    _drive(eng, STEP150, (8, BINS))
    buf = np.full((8, 4), -1, np.int32)
    n, dropped = C.c_int64(), C.c_int64()
    rc = eng._L.ffm_engine_drain_episodes(eng._h, buf.ctypes.data_as(C.c_void_p), 8, C.byref(n), C.byref(dropped), None)
    assert rc == 0 and n.value == 8 and dropped.value == len(want) - 8
    rows = {tuple(r) for r in want.tolist()}
    assert len({tuple(r) for r in buf.tolist()}) == 8 and all(tuple(r) in rows for r in buf.tolist())
    _assert_stats(eng.episode_stats(), want)
    eng.close()
    eng = _make(12, 12, 12, "neumann", 40)
    _drive(eng, STEP150, (8, 0))
    with pytest.raises(RuntimeError, match="overflowed"):
        eng.drain_episodes()
    eng.close()


# 9. reset_envs is not an episode end
def test_reset_envs(monkeypatch):
    _setenv(monkeypatch)
    E = 40
    mask = _third(E)
    ops = (("step", 25), ("reset_envs", mask), ("step", 125))
    want = _case(12, 12, 32, "neumann", E, ops)         # the GPU log equals this one exactly
    for e in range(E):
        rows = want[want[:, 0] == e]
        assert np.array_equal(rows[:, 1], np.arange(len(rows)))        # indices 0, 1, ..: the abandoned episode took none
        # no episode ends within 25 steps here, so a masked env's first record counts from the
        # re-placement's step index (26) and nothing was logged for what it abandoned
        assert rows[0, 2] == rows[0, 3] - (26 if mask[e] else 0)
        assert rows[0, 3] > 26


# 10. turned on after 10 steps
def test_log_turned_on_mid_run(monkeypatch):
    _setenv(monkeypatch)
    E = 40
    ops = (("step", 10), ("log_on",), ("step", 140))
    want = _case(12, 12, 12, "neumann", E, ops)
    full = _oracle(12, 12, 12, "neumann", E, STEP150)
    assert np.array_equal(want[:, [0, 1, 3]], full[:, [0, 1, 3]])     # no episode ends within 10 steps
    for e in range(E):
        w, f = want[want[:, 0] == e], full[full[:, 0] == e]
        assert w[0, 2] == w[0, 3] - 10 == f[0, 2] - 10
        assert np.array_equal(w[1:], f[1:])                             # later records as usual


# 11. run_episodes
def test_run_episodes(monkeypatch):
    _setenv(monkeypatch)
    E = 40
    full = _oracle(12, 12, 12, "neumann", E, STEP150)
    eng = _make(12, 12, 12, "neumann", E)
    eng.reset()
    got = eng.run_episodes(per_env=3)
    eng.close()
    assert got.dtype == np.int32 and got.shape == (E, 3)
    for e in range(E):
        f = full[full[:, 0] == e]
        assert len(f) >= 3 and np.array_equal(f[:3, 1], [0, 1, 2])
        assert np.array_equal(got[e], f[:3, 2]), e
    one = _oracle(12, 12, 12, "neumann", E, STEP150, False)
    _assert_covers(one, E)
    eng = _make(12, 12, 12, "neumann", E, auto=False)
    eng.reset()
    with pytest.raises(ValueError):
        eng.run_episodes(per_env=2)
    got = eng.run_episodes(per_env=1)
    assert got.shape == (E, 1) and np.array_equal(got[:, 0], one[:, 2])
    assert not eng.get_state()[1].any()                                # it stopped with every env empty
    eng.close()
    eng = _make(12, 12, 12, "neumann", E)
    eng.reset()
    with pytest.raises(RuntimeError, match="max_steps"):
        eng.run_episodes(per_env=1, max_steps=5)
    eng.close()


# 12. errors and the empty states
def test_errors_and_empty_states(monkeypatch):
    _setenv(monkeypatch)
    mt = _make(12, 12, 8, "neumann", 4, rng="mt")
    with pytest.raises(NotImplementedError):
        mt.set_episode_log()
    mt.close()
    eng = _make(12, 12, 12, "neumann", 40)
    eng.reset()
    eng.step(60)
    got = eng.drain_episodes()                                         # log off: nothing
    assert got.shape == (0, 4) and got.dtype == np.int32
    assert eng.episode_stats()["count"] == 0
    with pytest.raises(ValueError):
        eng.set_episode_log(capacity=-1)
    eng.set_episode_log(capacity=0, hist_bins=BINS)                    # statistics without the record log
    eng.step(60)
    assert eng.drain_episodes().shape == (0, 4)
    st = eng.episode_stats(clear=True)
    assert st["count"] > 0 and st["min"] > 0 and st["hist"].sum() == st["count"]
    st = eng.episode_stats()
    assert st["count"] == st["sum"] == st["sum_sq"] == st["min"] == st["max"] == 0 and not st["hist"].any()
    assert st["mean"] == 0.0 and st["std"] == 0.0
    eng.step(60)                                                       # min starts from its empty value again
    st = eng.episode_stats()
    assert st["count"] > 0 and 0 < st["min"] <= st["max"]
    eng.set_episode_log(capacity=0, hist_bins=0)                       # off again
    eng.step(20)
    assert eng.drain_episodes().shape == (0, 4) and eng.episode_stats()["count"] == 0
    eng.close()


# 13. drained every 16 steps
def test_chunked_drains(monkeypatch):
    _setenv(monkeypatch)
    E = 40
    want = _oracle(12, 12, 12, "neumann", E, STEP150)
    eng = _make(12, 12, 12, "neumann", E)
    eng.set_episode_log(capacity=16 * E, hist_bins=BINS)
    eng.reset()
    parts = []
    for t0 in range(0, 150, 16):
        eng.step(min(16, 150 - t0))
        parts.append(eng.drain_episodes())
    stats = eng.episode_stats()
    eng.close()
    got = np.concatenate(parts)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert np.array_equal(got, want)
    assert sum(len(p) > 0 for p in parts) > 3
    _assert_stats(stats, want)


# 14. next to trajectory capture (one launch per step, its kernel after every step)
def test_with_trajectory_capture(monkeypatch):
    _setenv(monkeypatch)
    E = 40
    want = _oracle(12, 12, 12, "neumann", E, STEP150)
    eng = _make(12, 12, 12, "neumann", E)
    eng.set_episode_log(hist_bins=BINS)
    eng.set_trajectory_capture([0, 7])
    eng.reset()
    eng.step(150)
    got = eng.drain_episodes()
    traj = eng.drain_trajectories()
    eng.close()
    assert np.array_equal(got, want)
    for env, k, steps, _ in want[np.isin(want[:, 0], [0, 7])].tolist():
        assert traj[(env, k)][0][-1] == steps                          # the captured episode's last step number
