"""Env-sharded step launches (FFM_STEP_SHARDS) of the group kernel: plain parity runs.

step(n > 1) of a group-kernel engine may step S disjoint env shards with launches of their own
on streams of their own.  Whatever S or the group size,
the state after any step(n) must be the same bits: positions (up to each env's count), counts,
DFF, episodes and all four counters are compared with the same engine created with
FFM_STEP_SHARDS=1, and for one case per group size with the oracle.  Every case is the 12x12
default room with auto-reset, Philox seed 42 and 150 steps (episodes take about 100).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS")
SEED, T = 42, 150


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


def _params(nbh):
    return {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


def _engine(E, N, nbh):
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    m = make_room(12, 12)
    return Engine(m, l1_sff(m), n_envs=E, n_agents=N, params=_params(nbh), rng="philox", seed=SEED,
                  auto_reset=True)


def _episodes(eng):
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


def _snapshot(eng, stream=None):
    pos, cnt, dff = eng.get_state(stream=stream)
    return {"pos": pos, "cnt": cnt, "dff": dff, "eps": _episodes(eng), "ctr": eng.counters(stream),
            "t": eng.step_index}


def _default_script(eng):
    eng.reset()
    eng.step(T)


def _run(monkeypatch, E, N, nbh, script=_default_script, want_shards=None, want_blocks=None, **env):
    """One engine under the switches in `env`, driven by script(eng); its final state."""
    _setenv(monkeypatch, **env)
    eng = _engine(E, N, nbh)
    li = eng.launch_info()
    assert li["kernel"] == "group", li
    if want_shards is not None:
        assert li["step_shards"] == want_shards, li
    if want_blocks is not None:
        assert li["shard_blocks"] == want_blocks, li
    script(eng)
    out = _snapshot(eng)
    out["li"] = eng.launch_info()
    eng.close()
    return out


def _assert_same(a, b):
    assert np.array_equal(a["cnt"], b["cnt"]), "counts"
    for e in range(len(a["cnt"])):
        assert np.array_equal(a["pos"][e, :a["cnt"][e]], b["pos"][e, :b["cnt"][e]]), f"env {e} positions"
    assert np.array_equal(a["dff"].view(np.uint32), b["dff"].view(np.uint32)), "DFF bits"
    assert np.array_equal(a["eps"], b["eps"]), "episodes"
    assert a["ctr"] == b["ctr"], (a["ctr"], b["ctr"])
    assert a["t"] == b["t"]


E_REF = 1027


@functools.lru_cache(maxsize=None)
def _oracle(N, nbh, E=E_REF):
    """The oracle from reset() for T steps, once per input point (envs are keyed by their global
    id, so the first E envs of the batch are the batch of E envs)."""
    from ffm_amd.data import make_room, l1_sff
    from oracle import oracle as O
    m = make_room(12, 12)
    core = O.Core(m, l1_sff(m), _params(nbh))
    pos = np.stack([core.reset_philox(N, SEED, 0, e) for e in range(E)])
    cnt = np.full(E, N, np.int32)
    dff = np.zeros((E,) + m.shape, np.float32)
    eps = np.zeros(E, np.int32)
    agent_steps = np.zeros(E, np.int64)
    exits = np.zeros(E, np.int64)
    for t in range(1, T + 1):
        before, e0 = cnt.astype(np.int64), eps.copy()
        core.step_philox_batch(pos, cnt, dff, eps, SEED, t, True, N, 0, 16)
        agent_steps += before
        exits += np.where(eps > e0, before, before - cnt)     # a re-placed env lost all it had
    for a in (pos, cnt, dff, eps, agent_steps, exits):
        a.setflags(write=False)
    return pos, cnt, dff, eps, agent_steps, exits


def _assert_oracle(got, N, nbh, E, ref_E=E_REF):
    pos, cnt, dff, eps, agent_steps, exits = (a[:E] for a in _oracle(N, nbh, ref_E))
    assert np.array_equal(got["cnt"], cnt), "counts vs oracle"
    for e in range(E):
        assert np.array_equal(got["pos"][e, :cnt[e]], pos[e, :cnt[e]]), f"env {e} positions vs oracle"
    assert np.array_equal(got["dff"].view(np.uint32), dff.view(np.uint32)), "DFF bits vs oracle"
    assert np.array_equal(got["eps"], eps), "episodes vs oracle"
    assert got["ctr"] == {"agent_steps": int(agent_steps.sum()), "exits": int(exits.sum()),
                          "resets": int(eps.sum()), "steps": T}
    return int(eps.sum())


# (E, S asked, shards in effect): 16 / 16 / 8 envs; 8 + 5 (the partial group in the last shard
# only); one shard left (empty shards are skipped) twice; 264 / 264 / 264 / 235
SHAPES = [(40, 3, 3), (13, 2, 2), (7, 2, 1), (8, 4, 1), (1027, 4, 4)]


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("N", [32, 12])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("E,S,eff", SHAPES)
def test_sharded_equals_unsharded(monkeypatch, E, S, eff, G, N, nbh):
    one = _run(monkeypatch, E, N, nbh, want_shards=1, FFM_STEP_SHARDS=1, FFM_GROUP_ENVS=G)
    assert one["ctr"]["steps"] == T and one["t"] == T + 1
    got = _run(monkeypatch, E, N, nbh, want_shards=eff, FFM_STEP_SHARDS=S, FFM_GROUP_ENVS=G)
    assert got["li"]["group_g"] == G
    _assert_same(got, one)
    if E == E_REF and N == 32 and nbh == "neumann":     # one case per group size: the oracle too
        assert _assert_oracle(got, N, nbh, E) > 0


def test_default_is_one_shard_at_small_sizes(monkeypatch):
    got = _run(monkeypatch, 1027, 32, "neumann", want_shards=1)
    assert got["li"]["shard_blocks"] == got["li"]["blocks"]
    assert _assert_oracle(got, 32, "neumann", 1027) > 0


def test_default_is_two_shards_at_the_headline_size(monkeypatch):
    """65,536 envs (a wave steps 2.67 groups): two shards of 32,768 envs with the full persistent
    grid each; 16,384 envs (one group per wave at most): one launch per step."""
    def script(eng):
        eng.reset()
        eng.step(12)

    got = _run(monkeypatch, 65536, 32, "neumann", script, want_shards=2)
    assert got["li"]["shard_blocks"] == got["li"]["blocks"]
    one = _run(monkeypatch, 65536, 32, "neumann", script, want_shards=1, FFM_STEP_SHARDS=1)
    _assert_same(got, one)
    small = _run(monkeypatch, 16384, 32, "neumann", script, want_shards=1)
    assert small["ctr"]["steps"] == 12


def test_one_block_per_shard_loops_sixteen_groups(monkeypatch):
    """FFM_WAVE_BLOCKS=1, S = 2, E = 512 at G = 4: each shard's single block steps 64 groups, 16
    per wave, and its waves place many deferred envs."""
    kw = dict(FFM_GROUP_ENVS=4, FFM_WAVE_BLOCKS=1)
    one = _run(monkeypatch, 512, 32, "neumann", want_shards=1, FFM_STEP_SHARDS=1, **kw)
    got = _run(monkeypatch, 512, 32, "neumann", want_shards=2, want_blocks=1, FFM_STEP_SHARDS=2, **kw)
    _assert_same(got, one)
    assert _assert_oracle(got, 32, "neumann", 512) > 0


def test_ordering_on_a_caller_stream(monkeypatch):
    """step / reset_envs / step / get_state on a non-default stream: the fork and the join order
    the shards' streams with everything else the caller's stream holds."""
    E = 1027
    mask = (np.arange(E) % 3 == 0).astype(np.uint8)

    def script(eng):
        st = torch.cuda.Stream()
        eng.reset(st)
        eng.step(7, st)
        eng.reset_envs(mask, st)
        eng.step(5, st)
        script.state = eng.get_state(stream=st)

    one = _run(monkeypatch, E, 32, "neumann", script, FFM_STEP_SHARDS=1)
    first = script.state
    got = _run(monkeypatch, E, 32, "neumann", script, want_shards=4, FFM_STEP_SHARDS=4)
    for a, b in zip(first, script.state):     # what get_state(stream) itself returned
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    _assert_same(got, one)
    assert got["ctr"]["steps"] == 12 and got["t"] == 14


def test_sharding_off_and_on_between_calls(monkeypatch):
    """step(1), step(3), step(1): one launch, sharded launches, one launch; t stays continuous."""
    def script(eng):
        eng.reset()
        eng.step(1)
        eng.step(3)
        eng.step(1)

    def five(eng):
        eng.reset()
        eng.step(5)

    one = _run(monkeypatch, 1027, 32, "neumann", five, FFM_STEP_SHARDS=1)
    got = _run(monkeypatch, 1027, 32, "neumann", script, want_shards=4, FFM_STEP_SHARDS=4)
    _assert_same(got, one)
    assert got["ctr"]["steps"] == 5 and got["t"] == 6


def test_capture_and_fused_steps_run_one_shard(monkeypatch):
    one = _run(monkeypatch, 1027, 32, "neumann", FFM_STEP_SHARDS=1)

    def with_capture(eng):
        eng.set_trajectory_capture([0, 5, 300], capacity_rows=3 * (T + 1))
        assert eng.launch_info()["step_shards"] == 1
        _default_script(eng)
        assert len(eng.drain_trajectories()) > 0

    def fused(eng):
        eng.set_fused_steps(4)
        assert eng.launch_info()["step_shards"] == 1
        _default_script(eng)

    for script in (with_capture, fused):
        got = _run(monkeypatch, 1027, 32, "neumann", script, want_shards=4, FFM_STEP_SHARDS=4)
        _assert_same(got, one)


@pytest.mark.parametrize("G,E", [(4, 256), (2, 128)])
def test_many_deferred_placements_in_one_block(monkeypatch, G, E):
    """One shard, one block, 16 groups per wave and N = 2 agents per env: many envs of the block
    empty on the same step, so every wave has several deferred placements after its last group."""
    got = _run(monkeypatch, E, 2, "neumann", want_shards=1, want_blocks=1, FFM_STEP_SHARDS=1,
               FFM_GROUP_ENVS=G, FFM_WAVE_BLOCKS=1)
    assert _assert_oracle(got, 2, "neumann", E, ref_E=256) > 0
