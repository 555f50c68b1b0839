"""The group kernel's single-group form (core_group_kernel<.., ONE>): plain parity runs.

A launch whose grid gives every wave at most one group (4 * blocks >= groups) takes the
single-group form; FFM_GROUP_ONE=0 at create keeps the loop form on every grid.  Both must leave
the same bits as the oracle (oracle.Core.step_philox_batch from reset_philox): positions up to
each env's count, counts, DFF as uint32, episodes and all four counters, and the same episode-log
records.  Every case is the 12x12 default room, Philox seed 42, 60 steps, and first asserts
through launch_info() which form runs.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS", "FFM_GROUP_ONE")
SEED, T = 42, 60
E_REF = 1027


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
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _params(nbh, k_D):
    return {"k_S": 3, "k_D": k_D, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


def _room():
    from ffm_amd.data import make_room, l1_sff
    m = make_room(12, 12)
    return m, l1_sff(m)


@functools.lru_cache(maxsize=None)
def _oracle(nbh, k_D, N, auto=True):
    """E_REF envs from reset() through T steps, once per input point (envs are keyed by their
    global id, so the first E envs of the batch are the batch of E envs).  Per env: the final
    state, the agent-steps and exits, and the episode count after every step."""
    from oracle import oracle as O
    m, s = _room()
    core = O.Core(m, s, _params(nbh, k_D))
    E = E_REF
    pos = np.stack([core.reset_philox(N, SEED, 0, e) for e in range(E)])
    cnt = np.full(E, N, np.int32)
    dff = np.zeros((E,) + m.shape, np.float32)
    eps = np.zeros(E, np.int32)
    agent_steps = np.zeros(E, np.int64)
    exits = np.zeros(E, np.int64)
    eps_hist = np.zeros((T + 1, E), np.int32)
    for t in range(1, T + 1):
        before, e0 = cnt.astype(np.int64), eps.copy()
        core.step_philox_batch(pos, cnt, dff, eps, SEED, t, auto, N, 0, 16)
        agent_steps += before
        exits += np.where(eps > e0, before, before - cnt)     # a re-placed env lost all it had
        eps_hist[t] = eps
    out = {"pos": pos, "cnt": cnt, "dff": dff, "eps": eps, "agent_steps": agent_steps, "exits": exits,
           "eps_hist": eps_hist}
    for a in out.values():
        a.setflags(write=False)
    return out


def _episodes(eng):
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


def _steps_at_once(eng):
    eng.step(T)


def _run(monkeypatch, E, N, nbh, k_D, want_one, auto=True, drive=_steps_at_once, log=False, want=None, **env):
    """One engine under the switches in `env`: reset(), drive(eng); its final state.  The form
    (and whatever else `want` names in launch_info()) is asserted before anything is compared."""
    from ffm_amd.engine import Engine
    _setenv(monkeypatch, **env)
    m, s = _room()
    eng = Engine(m, s, n_envs=E, n_agents=N, params=_params(nbh, k_D), rng="philox", seed=SEED, auto_reset=auto)
    try:
        if log:
            eng.set_episode_log(None, 0)
        li = eng.launch_info()
        assert li["kernel"] == "group" and li["group_one"] == want_one, li
        for k, v in (want or {}).items():
            assert li[k] == v, (k, li)
        eng.reset()
        drive(eng)
        pos, cnt, dff = eng.get_state()
        out = {"pos": pos, "cnt": cnt, "dff": dff, "eps": _episodes(eng), "ctr": eng.counters(),
               "t": eng.step_index, "li": li}
        if log:
            out["rec"] = eng.drain_episodes()
        return out
    finally:
        eng.close()


def _assert_same(a, b):
    assert np.array_equal(a["cnt"], b["cnt"]), "counts"
    for e in range(len(a["cnt"])):
        assert np.array_equal(a["pos"][e, :a["cnt"][e]], b["pos"][e, :b["cnt"][e]]), f"env {e} positions"
    assert np.array_equal(a["dff"].view(np.uint32), b["dff"].view(np.uint32)), "DFF bits"
    assert np.array_equal(a["eps"], b["eps"]), "episodes"
    assert a["ctr"] == b["ctr"], (a["ctr"], b["ctr"])
    assert a["t"] == b["t"]


def _assert_oracle(got, ref, E):
    cnt = ref["cnt"][:E]
    assert np.array_equal(got["cnt"], cnt), "counts vs oracle"
    for e in range(E):
        assert np.array_equal(got["pos"][e, :cnt[e]], ref["pos"][e, :cnt[e]]), f"env {e} positions vs oracle"
    assert np.array_equal(got["dff"].view(np.uint32), ref["dff"][:E].view(np.uint32)), "DFF bits vs oracle"
    assert np.array_equal(got["eps"], ref["eps"][:E]), "episodes vs oracle"
    assert got["ctr"] == {"agent_steps": int(ref["agent_steps"][:E].sum()), "exits": int(ref["exits"][:E].sum()),
                          "resets": int(ref["eps"][:E].sum()), "steps": T}
    assert got["t"] == T + 1


# E < G, a partial last group, and 4 * blocks - groups in {0, 1, 2, 3}: waves without a group
E_CASES = (1, 3, 5, 16, 1027)


def test_cases_cover_the_idle_waves():
    idle = {4 * -(-(-(-E // G)) // 4) - -(-E // G) for E in E_CASES for G in (2, 4)}
    assert idle == {0, 1, 2, 3}
    assert any(E < G for E in E_CASES for G in (2, 4)) and any(E % 4 for E in E_CASES)


@pytest.mark.parametrize("N", [2, 32])
@pytest.mark.parametrize("k_D", [1, 2])
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("E", E_CASES)
def test_one_equals_oracle_and_loop(monkeypatch, E, G, nbh, k_D, N):
    groups = -(-E // G)
    geo = {"group_g": G, "blocks": -(-groups // 4), "step_shards": 1}
    one = _run(monkeypatch, E, N, nbh, k_D, True, want=geo, FFM_GROUP_ENVS=G)
    loop = _run(monkeypatch, E, N, nbh, k_D, False, want=geo, FFM_GROUP_ENVS=G, FFM_GROUP_ONE=0)
    _assert_same(one, loop)
    _assert_oracle(one, _oracle(nbh, k_D, N), E)


@pytest.mark.parametrize("G", [2, 4])
def test_placements_from_the_step_ballot(monkeypatch, G):
    """N = 2 agents per env: envs empty every few steps, and some step re-places two or more envs
    of one group (asserted on the oracle's episode counts), so a wave runs several placements
    after one step, in env order."""
    E, N = 64, 2
    ref = _oracle("neumann", 1, N)
    replaced = np.diff(ref["eps_hist"][:, :E], axis=0) > 0                # [T, E]
    per_group = replaced.reshape(T, E // G, G).sum(axis=2)
    assert per_group.max() >= 2, "no step re-placed two envs of one group"
    one = _run(monkeypatch, E, N, "neumann", 1, True, FFM_GROUP_ENVS=G)
    assert one["ctr"]["resets"] > 0
    _assert_oracle(one, ref, E)
    loop = _run(monkeypatch, E, N, "neumann", 1, False, FFM_GROUP_ENVS=G, FFM_GROUP_ONE=0)
    _assert_same(one, loop)


def test_no_placements_without_auto_reset(monkeypatch):
    E, N = 64, 2
    ref = _oracle("neumann", 1, N, auto=False)
    assert (ref["cnt"][:E] == 0).any(), "no env emptied"
    one = _run(monkeypatch, E, N, "neumann", 1, True, auto=False, FFM_GROUP_ENVS=4)
    assert one["ctr"]["resets"] == 0
    _assert_oracle(one, ref, E)
    loop = _run(monkeypatch, E, N, "neumann", 1, False, auto=False, FFM_GROUP_ENVS=4, FFM_GROUP_ONE=0)
    _assert_same(one, loop)


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("G", [2, 4])
def test_episode_log_records_equal_the_loop_forms(monkeypatch, G, auto):
    E, N = 67, 2
    one = _run(monkeypatch, E, N, "neumann", 1, True, auto=auto, log=True, FFM_GROUP_ENVS=G)
    loop = _run(monkeypatch, E, N, "neumann", 1, False, auto=auto, log=True, FFM_GROUP_ENVS=G, FFM_GROUP_ONE=0)
    assert len(loop["rec"]) > 0
    if auto:
        assert len(loop["rec"]) == int(_oracle("neumann", 1, N)["eps"][:E].sum())
    assert np.array_equal(one["rec"], loop["rec"])
    _assert_same(one, loop)
    _assert_oracle(one, _oracle("neumann", 1, N, auto), E)


@pytest.mark.parametrize("S", [2, 4])
def test_shards_take_the_single_group_form(monkeypatch, S):
    def by_twelve(eng):
        for _ in range(T // 12):
            eng.step(12)

    E, N = 1027, 32
    got = _run(monkeypatch, E, N, "neumann", 1, True, drive=by_twelve, want={"step_shards": S}, FFM_STEP_SHARDS=S)
    one = _run(monkeypatch, E, N, "neumann", 1, True, drive=by_twelve, want={"step_shards": 1}, FFM_STEP_SHARDS=1)
    _assert_same(got, one)
    _assert_oracle(got, _oracle("neumann", 1, N), E)


def test_the_launcher_picks_by_the_grid(monkeypatch):
    """One block for 16 groups: the loop form, whatever FFM_GROUP_ONE says; the default grid of
    the same engine: the single-group form."""
    E, N = 64, 32
    loop = _run(monkeypatch, E, N, "neumann", 1, False, want={"blocks": 1, "group_g": 4}, FFM_WAVE_BLOCKS=1,
                FFM_GROUP_ENVS=4)
    one = _run(monkeypatch, E, N, "neumann", 1, True, want={"blocks": 4, "group_g": 4}, FFM_GROUP_ENVS=4)
    _assert_same(one, loop)
    _assert_oracle(one, _oracle("neumann", 1, N), E)
