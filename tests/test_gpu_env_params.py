"""Per-env parameters and agent counts (ffm_engine_set_env_params / Engine.set_env_params).

The contract: env e of an engine with per-env parameters (global id env_base + e, set
sets[set_of_env[e]]) evolves bit for bit like the env with the same global id of a homogeneous
engine created with that set.  The expected state comes from the oracle, one env at a time:
Core(map, sff, set).step_philox_batch on the env's one-row slices with its own N and global id,
Core.reset_philox for its placements.  Compared: positions (the live ones), counts, DFF bits,
the episodes counter, the agent_steps / resets counters and, where the log is on, the
episode-log records.  Every case asserts launch_info()["kernel"] before comparing anything, so
a case cannot pass on another kernel than the one it is about.
"""
import functools

import numpy as np
import pytest

from env_sweep_util import _assert_same, _dicts, _params, _snapshot

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 42
# the 12x12 sets (k_S, k_D, diffuse, decay, N); env e runs set e % 5
SETS5 = ((3, 1, 0.2, 0.2, 32), (0.5, 0, 0.2, 0.2, 5), (10, 2.5, 0.05, 0.6, 17), (1.5, 1, 0.5, 0.1, 1),
         (1, 4, 0.3, 0.3, 24))
SETS5_40 = SETS5                                                  # A = 40: every N is below the cap already
SETS3 = ((3, 1, 0.2, 0.2, 24), (0.5, 0, 0.2, 0.2, 3), (10, 2.5, 0.05, 0.6, 13))
SETS2 = ((3, 1, 0.2, 0.2, 40), (8, 0.5, 0.1, 0.4, 7))
# the sets the mid-run case switches to (another N for every env)
SETS5_B = ((1, 4, 0.3, 0.3, 9), (3, 1, 0.2, 0.2, 32), (0.5, 0, 0.2, 0.2, 20), (10, 2.5, 0.05, 0.6, 3),
           (1.5, 1, 0.5, 0.1, 28))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def _room(H, W, f64=False):
    from ffm_amd.data import make_room, l1_sff
    m = make_room(H, W)
    return m, l1_sff(m, dtype=np.float64 if f64 else np.float32)


# ---------------------------------------------------------------------------
# The oracle mirror: one Core per set, one env per call.
# ops: ("step", n) | ("snap",) | ("sets", sets) | ("reset_envs", mask tuple) | ("update_dff",)
# Returns the snapshots {pos, cnt, dff, eps, agent_steps, resets} and the episode records.
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(H, W, A, nbh, E, sets, ops, f64=False, env_base=0):
    from oracle import oracle as O
    m, s = _room(H, W, f64)
    cores = {}

    def core(st):
        if st not in cores:
            cores[st] = O.Core(m, s, _params(st, nbh))
        return cores[st]

    cur = [sets[e % len(sets)] for e in range(E)]
    pos = np.full((E, A), 0xFFFF, np.uint16)
    cnt = np.zeros(E, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    for e in range(E):                                   # reset(): placement keyed t = 0
        N = cur[e][4]
        pos[e, :N] = core(cur[e]).reset_philox(N, SEED, 0, env_base + e)
        cnt[e] = N
    start = np.zeros(E, np.int64)
    agent_steps, t, snaps, recs = 0, 1, [], []
    for op in ops:
        if op[0] == "step":
            for _ in range(op[1]):
                agent_steps += int(cnt.sum())
                for e in range(E):
                    k0 = eps[e]
                    core(cur[e]).step_philox_batch(pos[e:e + 1], cnt[e:e + 1], dff[e:e + 1], eps[e:e + 1], SEED, t,
                                                   True, cur[e][4], env_base + e, 1)
                    if eps[e] != k0:
                        recs.append((env_base + e, k0, t - start[e], t))
                        start[e] = t
                t += 1
        elif op[0] == "snap":
            snaps.append({"pos": pos.copy(), "cnt": cnt.copy(), "dff": dff.copy(), "eps": eps.copy(),
                          "agent_steps": agent_steps, "resets": int(eps.sum())})
        elif op[0] == "sets":                            # parameters now, N at the env's next placement
            cur = [op[1][e % len(op[1])] for e in range(E)]
        elif op[0] == "reset_envs":                      # placed with index t, which advances
            for e in np.flatnonzero(np.asarray(op[1])):
                N = cur[e][4]
                pos[e] = 0xFFFF
                pos[e, :N] = core(cur[e]).reset_philox(N, SEED, t, env_base + e)
                cnt[e] = N
                dff[e] = 0.0
                start[e] = t
            t += 1
        elif op[0] == "update_dff":
            for e in range(E):
                core(cur[e]).update_dff(dff[e])
    rec = np.asarray(recs, np.int64).reshape(-1, 4)
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))].astype(np.int32)
    for sn in snaps:
        for v in sn.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    rec.setflags(write=False)
    return tuple(snaps), rec


def _engine(H, W, A, nbh, E, create, epb=0, f64=False, env_base=0, rng="philox"):
    from ffm_amd.engine import Engine
    m, s = _room(H, W, f64)
    return Engine(m, s, n_envs=E, n_agents=create[4], agent_capacity=A, params=_params(create, nbh), rng=rng,
                  seed=SEED, auto_reset=True, env_base=env_base, envs_per_block=epb)


def _assert_resets(eps, sets, which):
    """Auto-reset with per-env N is exercised: every env of the sets `which` ended an episode."""
    P = len(sets)
    for p in which:
        assert (eps[p::P] > 0).all(), f"oracle: an env of set {p} ended no episode"


def _run_vs_oracle(H, W, A, nbh, E, sets, T, epb, before, after, f64=False, fused=1, resets=()):
    eng = _engine(H, W, A, nbh, E, sets[0], epb, f64)
    try:
        assert eng.launch_info()["kernel"] == before
        eng.set_env_params(_dicts(sets))
        info = eng.launch_info()
        assert info["kernel"] == after and info["step_shards"] == 1
        if fused > 1:
            assert info["multi"]
            eng.set_fused_steps(fused)
        eng.reset()
        eng.step(T)
        got = _snapshot(eng)
    finally:
        eng.close()
    (want,), _ = _oracle(H, W, A, nbh, E, sets, (("step", T), ("snap",)), f64)
    _assert_resets(want["eps"], sets, resets)
    _assert_same(got, want, f"{H}x{W} {nbh} {after}")
    return info


# 1. against the oracle, lane kernel (E odd: the last pair is half empty)
@pytest.mark.parametrize("epb,before", [(0, "group"), (-2, "lane")])
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_lane_kernel_matches_oracle(nbh, epb, before):
    _run_vs_oracle(12, 12, 32, nbh, 135, SETS5, 120, epb, before, "lane", resets=(0, 1, 2, 3))


# 2. the fused multi-step kernel (119 = 17 launches of 7 steps)
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_fused_steps_match_oracle(nbh):
    _run_vs_oracle(12, 12, 32, nbh, 135, SETS5, 119, 0, "group", "lane", fused=7, resets=(0, 1, 2, 3))


# 3. block kernel with K > 1 envs per workgroup
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_block_kernel_matches_oracle(nbh):
    info = _run_vs_oracle(20, 20, 24, nbh, 23, SETS3, 150, 0, "block", "block", resets=(0, 1, 2))
    assert info["K"] > 1


# 4. a wave engine steps with the block kernel meanwhile
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_wave_engine_falls_to_block_kernel(nbh):
    _run_vs_oracle(12, 12, 40, nbh, 11, SETS5_40, 120, 0, "wave", "block", resets=(0, 1, 2, 3))


# 5. the block kernel's global-scratch form
def test_scratch_form_matches_oracle():
    _run_vs_oracle(160, 160, 40, "neumann", 3, SETS2, 40, 0, "block_scratch", "block_scratch")


# 6. float64 SFF (block kernel, kS64)
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_f64_sff_matches_oracle(nbh):
    _run_vs_oracle(12, 12, 32, nbh, 10, SETS5, 120, 0, "block", "block", f64=True, resets=(0, 1, 2, 3))


# 7. against the shipped kernels: homogeneous group engines, same global ids
@pytest.mark.parametrize("env_base", [0, 1000])
def test_rows_equal_homogeneous_group_engines(env_base):
    E, T, nbh = 135, 120, "neumann"
    het = _engine(12, 12, 32, nbh, E, SETS5[0], 0, env_base=env_base)
    try:
        het.set_env_params(_dicts(SETS5))
        assert het.launch_info()["kernel"] == "lane"
        het.reset()
        het.step(T)
        got = _snapshot(het)
    finally:
        het.close()
    for p, st in enumerate(SETS5):
        hom = _engine(12, 12, 32, nbh, E, st, 0, env_base=env_base)
        try:
            assert hom.launch_info()["kernel"] == "group"
            hom.reset()
            hom.step(T)
            ref = _snapshot(hom)
        finally:
            hom.close()
        rows = np.arange(p, E, 5)
        assert np.array_equal(got["cnt"][rows], ref["cnt"][rows]), f"set {p}: counts"
        assert np.array_equal(got["eps"][rows], ref["eps"][rows]), f"set {p}: episodes"
        assert np.array_equal(got["dff"][rows].view(np.uint32), ref["dff"][rows].view(np.uint32)), f"set {p}: DFF"
        for e in rows:
            n = ref["cnt"][e]
            assert np.array_equal(got["pos"][e, :n], ref["pos"][e, :n]), f"set {p}: positions (env {e})"


# 8. identity and the off switch
def test_identity_and_off_switch():
    E, nbh, st = 135, "neumann", SETS5[0]
    a = _engine(12, 12, 32, nbh, E, st)
    b = _engine(12, 12, 32, nbh, E, st)
    try:
        created = a.launch_info()
        assert created["kernel"] == "group" and b.launch_info() == created
        a.set_env_params(_dicts([st, st]))
        assert a.launch_info()["kernel"] == "lane"
        sets, soe = a.env_params()
        assert sets == _dicts([st, st]) and np.array_equal(soe, np.arange(E) % 2)
        for eng in (a, b):
            eng.reset()
            eng.step(60)
        _assert_same(_snapshot(a), _snapshot(b), "identity")
        a.set_env_params(None)
        assert a.launch_info() == created
        assert a.env_params() == ([], None)
        for eng in (a, b):
            eng.step(60)
        _assert_same(_snapshot(a), _snapshot(b), "after the off switch")
    finally:
        a.close()
        b.close()


# 9. new sets mid-run: parameters at once, N at the env's next placement
def test_mid_run_change():
    E, nbh = 135, "neumann"
    eng = _engine(12, 12, 32, nbh, E, SETS5[0])
    try:
        eng.set_env_params(_dicts(SETS5))
        assert eng.launch_info()["kernel"] == "lane"
        eng.reset()
        eng.step(60)
        eng.set_env_params(_dicts(SETS5_B))
        assert eng.launch_info()["kernel"] == "lane"
        mid = _snapshot(eng)
        eng.step(60)
        got = _snapshot(eng)
    finally:
        eng.close()
    (wmid, want), _ = _oracle(12, 12, 32, nbh, E, SETS5,
                              (("step", 60), ("snap",), ("sets", SETS5_B), ("step", 60), ("snap",)))
    _assert_same(mid, wmid, "before the change (the call moves nothing)")
    assert (want["eps"] > wmid["eps"]).any(), "oracle: no placement after the change"
    _assert_same(got, want, "after the change")


# 10. reset_envs: masked envs get their own N, the others are untouched
def test_reset_envs_places_own_n():
    E, nbh = 135, "neumann"
    mask = tuple(int(v) for v in (np.random.RandomState(7).rand(E) < 1 / 3))
    assert 0 < sum(mask) < E
    eng = _engine(12, 12, 32, nbh, E, SETS5[0])
    try:
        eng.set_env_params(_dicts(SETS5))
        assert eng.launch_info()["kernel"] == "lane"
        eng.reset()
        eng.step(10)
        eng.reset_envs(np.asarray(mask, np.uint8))
        at = _snapshot(eng)
        eng.step(30)
        got = _snapshot(eng)
    finally:
        eng.close()
    (wat, want), _ = _oracle(12, 12, 32, nbh, E, SETS5,
                             (("step", 10), ("reset_envs", mask), ("snap",), ("step", 30), ("snap",)))
    _assert_same(at, wat, "right after reset_envs")
    _assert_same(got, want, "30 steps later")


# 11. the episode log carries every env's own evacuation times
@pytest.mark.parametrize("epb,after", [(0, "lane"), (6, "block")])
def test_episode_log_records(epb, after):
    E, T, nbh = 135, 120, "neumann"
    eng = _engine(12, 12, 32, nbh, E, SETS5[0], epb)
    try:
        eng.set_env_params(_dicts(SETS5))
        assert eng.launch_info()["kernel"] == after
        eng.set_episode_log(capacity=E * T)
        eng.reset()
        eng.step(T)
        rec = eng.drain_episodes()
    finally:
        eng.close()
    _, want = _oracle(12, 12, 32, nbh, E, SETS5, (("step", T), ("snap",)))
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    assert len(want) > 0 and np.array_equal(rec, want)


def test_run_episodes_returns_per_env_lengths():
    E, nbh = 40, "moore"          # Moore: every set, the k_D-dominated one included, ends episodes
    eng = _engine(12, 12, 32, nbh, E, SETS5[0])
    try:
        eng.set_env_params(_dicts(SETS5))
        assert eng.launch_info()["kernel"] == "lane"
        eng.reset()
        steps = eng.run_episodes(per_env=2, max_steps=4000, chunk=16)
    finally:
        eng.close()
    _, want = _oracle(12, 12, 32, nbh, E, SETS5, (("step", int(steps.sum(axis=1).max())), ("snap",)))
    for e in range(E):
        mine = want[want[:, 0] == e]
        assert np.array_equal(steps[e], mine[:2, 2]), f"env {e}"


# 12. update_dff() with each env's own diffuse / decay
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_update_dff_per_env(nbh):
    E = 23
    eng = _engine(12, 12, 32, nbh, E, SETS5[0])
    try:
        eng.set_env_params(_dicts(SETS5))
        assert eng.launch_info()["kernel"] == "lane"
        eng.reset()
        eng.step(20)
        eng.update_dff()
        got = _snapshot(eng)
    finally:
        eng.close()
    (want,), _ = _oracle(12, 12, 32, nbh, E, SETS5, (("step", 20), ("update_dff",), ("snap",)))
    assert want["dff"].any()
    _assert_same(got, want, "update_dff")


# 13. errors leave the engine as it was
def test_errors_leave_engine_unchanged():
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    E, st = 16, SETS5[0]
    eng = _engine(12, 12, 32, "neumann", E, st)
    try:
        eng.set_env_params(_dicts(SETS5[:2]))
        info, (sets, soe) = eng.launch_info(), eng.env_params()
        assert info["kernel"] == "lane"
        for bad, soe_bad in (([{"n_agents": 0}], None), ([{"n_agents": 33}], None), ([{"k_S": float("nan")}], None),
                             (_dicts(SETS5[:2]), np.full(E, 2, np.int32)), (_dicts(SETS5[:2]), np.full(E, -1, np.int32))):
            with pytest.raises(ValueError):
                eng.set_env_params(bad, soe_bad)
            assert eng.launch_info() == info
            s2, soe2 = eng.env_params()
            assert s2 == sets and np.array_equal(soe2, soe)
        with pytest.raises(ValueError):                      # more sets than envs
            eng.set_env_params(_dicts([st] * (E + 1)), np.zeros(E, np.int32))
    finally:
        eng.close()
    m = make_room(5, 6)                                      # 12 free cells, fewer than the 16 agent slots
    small = Engine(m, l1_sff(m), n_envs=4, n_agents=4, agent_capacity=16, params=_params(st, "neumann"), seed=SEED)
    try:
        with pytest.raises(ValueError):
            small.set_env_params([{"n_agents": 13}])
        assert small.env_params() == ([], None)
        small.set_env_params([{"n_agents": 12}])
    finally:
        small.close()
    mt = _engine(12, 12, 32, "neumann", 2, st, rng="mt")
    try:
        with pytest.raises(NotImplementedError):
            mt.set_env_params(_dicts(SETS5[:2]))
        assert mt.env_params() == ([], None)
    finally:
        mt.close()
