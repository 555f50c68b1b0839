"""The single-group form's compaction without the kept-prefix array (core_group_kernel<.., ONE>).

The form takes the kept prefix at an env's start from the lane that holds it (the popcount of the
resolve ballots below that packed index), not from an LDS array.  Two measured builds also took an
agent's position from the register of the lane that loaded its dword and read the free list from
global memory; they were retired from the source (profiles/lds_fit/README.md names their define
and the commit, 2113d5c, that rebuilds them), and these cases cover their boundaries too.  The cases inject counts and positions with Engine.set_state
so that the packed prefix S meets every boundary of those paths, then compare exactly, after
every case's precondition has been asserted on the oracle's own run:

  * against the oracle (oracle.Core.step_philox_batch from the injected state), and
  * against the same engine with FFM_GROUP_ONE=0 (the loop form, which keeps both arrays).

12x12 default room, Philox seed 42, at most 20 steps, E <= 1,027.  The only cell next to the exit
(0, 6) in the Neumann neighbourhood is (1, 6), so in a Neumann run the agent that left an env is
the one that stood there.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS", "FFM_GROUP_ONE", "FFM_RESET_CANDIDATES")
SEED, T = 42, 12
W = 12
DOOR = 1 * W + 6          # the cell below the exit
NONE = 0xFFFF

P4 = ((32, 32, 32, 32), (32, 31, 2, 32), (0, 32, 0, 32), (32, 0, 0, 0), (1, 1, 1, 1))
P2 = ((32, 32), (0, 32), (31, 1))
REPS = 12


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


@functools.lru_cache(maxsize=None)
def _room():
    from ffm_amd.data import make_room, l1_sff, free_cells
    m = make_room(12, 12)
    return m, l1_sff(m), free_cells(m)


def _rows(counts, A, rng, door=0.8):
    """Positions for the given counts: distinct free cells in random order; with probability
    `door` one of the env's agents, at a random index, stands on the cell next to the exit."""
    free = _room()[2]
    pos = np.full((len(counts), A), NONE, np.uint16)
    for e, c in enumerate(counts):
        cells = rng.permutation(free)[:c]
        if c and rng.random() < door and DOOR not in cells:
            cells[rng.integers(c)] = DOOR
        pos[e, :c] = cells
    return pos


@functools.lru_cache(maxsize=None)
def _pattern_state(G):
    """REPS copies of every count pattern, group after group, then G - 1 envs more: a partial last
    group, and (groups % 4 != 0) waves that hold no group."""
    rng = np.random.default_rng(1000 + G)
    pats = P4 if G == 4 else P2
    counts = [c for _ in range(REPS) for p in pats for c in p] + [int(c) for c in rng.integers(0, 33, G - 1)]
    cnt = np.array(counts, np.int32)
    assert len(cnt) % G != 0 and -(-len(cnt) // G) % 4 != 0 and len(cnt) <= 1027
    pos = _rows(counts, 32, rng)
    pos.setflags(write=False)
    cnt.setflags(write=False)
    return pos, cnt


@functools.lru_cache(maxsize=None)
def _random_state(E, A, seed=7):
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in rng.integers(0, A + 1, E)]
    pos, cnt = _rows(counts, A, rng), np.array(counts, np.int32)
    pos.setflags(write=False)
    cnt.setflags(write=False)
    return pos, cnt


@functools.lru_cache(maxsize=None)
def _oracle(state, nbh, k_D, N, auto=True):
    """T steps (t = 1..T) from the injected state `state` = (maker, *args), once per input point.
    Per step: the counts and positions before it and the episode counts after it."""
    from oracle import oracle as O
    m, s, _ = _room()
    core = O.Core(m, s, _params(nbh, k_D))
    pos0, cnt0 = state[0](*state[1:])
    pos, cnt = pos0.copy(), cnt0.copy()
    E = len(cnt)
    dff = np.zeros((E,) + m.shape, np.float32)
    eps = np.zeros(E, np.int32)
    agent_steps = exits = 0
    pre_pos, pre_cnt, eps_hist = [], [], [eps.copy()]
    for t in range(1, T + 1):
        before, e0 = cnt.astype(np.int64), eps.copy()
        pre_pos.append(pos.copy())
        pre_cnt.append(cnt.copy())
        core.step_philox_batch(pos, cnt, dff, eps, SEED, t, auto, N, 0, 16)
        agent_steps += int(before.sum())
        exits += int(np.where(eps > e0, before, before - cnt).sum())     # a re-placed env lost all it had
        eps_hist.append(eps.copy())
    out = {"pos": pos, "cnt": cnt, "dff": dff, "eps": eps, "agent_steps": agent_steps, "exits": exits,
           "pre_pos": np.stack(pre_pos), "pre_cnt": np.stack(pre_cnt), "eps_hist": np.stack(eps_hist)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _episodes(eng):
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


def _run(monkeypatch, state, N, nbh, k_D, want_one, auto=True, log=False, want=None, **env):
    """One engine under the switches in `env`: reset(), the injected state, step(T); its final
    state.  The form (and whatever else `want` names in launch_info()) is asserted first."""
    from ffm_amd.engine import Engine
    _setenv(monkeypatch, **env)
    m, s, _ = _room()
    pos0, cnt0 = state[0](*state[1:])
    E, A = pos0.shape
    eng = Engine(m, s, n_envs=E, n_agents=N, agent_capacity=A, params=_params(nbh, k_D), rng="philox", seed=SEED,
                 auto_reset=auto)
    try:
        if log:
            eng.set_episode_log(None, 0)
        li = eng.launch_info()
        assert li["kernel"] == "group" and li["group_one"] == want_one, li
        for k, v in (want or {}).items():
            assert li[k] == v, (k, li)
        eng.reset()
        eng.set_state(0, pos0, cnt0, np.zeros((E,) + m.shape, np.float32))
        eng.step(T)
        pos, cnt, dff = eng.get_state()
        out = {"pos": pos, "cnt": cnt, "dff": dff, "eps": _episodes(eng), "ctr": eng.counters(), "t": eng.step_index}
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
    if "rec" in a or "rec" in b:
        assert np.array_equal(a["rec"], b["rec"]), "episode-log records"


def _assert_oracle(got, ref):
    cnt = ref["cnt"]
    assert np.array_equal(got["cnt"], cnt), "counts vs oracle"
    for e in range(len(cnt)):
        assert np.array_equal(got["pos"][e, :cnt[e]], ref["pos"][e, :cnt[e]]), f"env {e} positions vs oracle"
    assert np.array_equal(got["dff"].view(np.uint32), ref["dff"].view(np.uint32)), "DFF bits vs oracle"
    assert np.array_equal(got["eps"], ref["eps"]), "episodes vs oracle"
    assert got["ctr"] == {"agent_steps": ref["agent_steps"], "exits": ref["exits"], "resets": int(ref["eps"].sum()),
                          "steps": T}
    assert got["t"] == T + 1


def _exit_lanes(ref, G):
    """Per (step, group) of a Neumann run: the packed indices S[s] + al of the agents that left,
    and the prefix S of the counts the step started from."""
    out = []
    for t in range(T):
        pos, cnt = ref["pre_pos"][t], ref["pre_cnt"][t]
        after = ref["pre_cnt"][t + 1] if t + 1 < T else ref["cnt"]
        gone = (after < cnt) | (ref["eps_hist"][t + 1] > ref["eps_hist"][t])   # its last agent: re-placed
        for g in range(len(cnt) // G):
            S = np.concatenate(([0], np.cumsum(cnt[g * G:(g + 1) * G])))
            js = []
            for s in range(G):
                e = g * G + s
                if gone[e] and cnt[e] > 0:
                    al = np.flatnonzero(pos[e, :cnt[e]] == DOOR)
                    assert len(al) == 1, "an env lost an agent that did not stand next to the exit"
                    js.append((int(S[s] + al[0]), s))
            out.append((t, g, S, js))
    return out


def _both(monkeypatch, state, N, nbh, k_D, G, auto=True, log=False, **env):
    ref = _oracle(state, nbh, k_D, N, auto)
    one = _run(monkeypatch, state, N, nbh, k_D, True, auto=auto, log=log, want={"group_g": G}, FFM_GROUP_ENVS=G, **env)
    loop = _run(monkeypatch, state, N, nbh, k_D, False, auto=auto, log=log, want={"group_g": G}, FFM_GROUP_ENVS=G,
                FFM_GROUP_ONE=0, **env)
    _assert_oracle(one, ref)
    _assert_same(one, loop)
    return ref, one


def test_prefix_boundaries_g4(monkeypatch):
    """S = 0, 32, 64, 96, 128; an env straddling lane 63; empty envs first, middle and last; one
    agent per env.  Exits before lane 63, after lane 64 and in the straddling env in one step."""
    state = (_pattern_state, 4)
    _, cnt0 = _pattern_state(4)
    ref = _oracle(state, "neumann", 1, 32)
    first = {tuple(cnt0[g * 4:g * 4 + 4]) for g in range(len(cnt0) // 4)}
    assert first == set(P4)
    ev = _exit_lanes(ref, 4)
    assert any(tuple(S) == (0, 32, 64, 96, 128) for _, _, S, _ in ev)
    both_sides = straddle = False
    for _, _, S, js in ev:
        lo, hi = any(j < 63 for j, _ in js), any(j > 64 for j, _ in js)
        mid = any(S[s] < 64 < S[s + 1] for _, s in js)    # the env holds packed indices 63 and 64
        both_sides |= lo and hi
        straddle |= lo and hi and mid
    assert both_sides, "no step with exits on both sides of lane 63 in one group"
    assert straddle, "no such step with an exit in an env that straddles lane 63 as well"
    assert any(j == 63 for *_, js in ev for j, _ in js) and any(j == 64 for *_, js in ev for j, _ in js)
    _both(monkeypatch, state, 32, "neumann", 1, 4)


def test_prefix_boundaries_g2(monkeypatch):
    state = (_pattern_state, 2)
    _, cnt0 = _pattern_state(2)
    ref = _oracle(state, "neumann", 1, 32)
    assert {tuple(cnt0[g * 2:g * 2 + 2]) for g in range(len(cnt0) // 2)} == set(P2)
    ev = _exit_lanes(ref, 2)
    assert any(len(js) == 2 for *_, js in ev), "no step with exits in both envs of a group"
    assert any(tuple(S) == (0, 31, 32) and any(s == 1 for _, s in js) for _, _, S, js in ev)
    _both(monkeypatch, state, 32, "neumann", 1, 2)


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("A", [13, 31])
def test_odd_rows(monkeypatch, G, A):
    """Odd agent capacity: the row of an odd env starts in the high half of a position dword.
    E = 67: a partial last group, and waves without a group."""
    E = 67
    state = (_random_state, E, A)
    assert E % G != 0 and -(-E // G) % 4 != 0
    ref, _ = _both(monkeypatch, state, A, "neumann", 1, G)
    assert ref["exits"] > 0 and int(ref["eps"].sum()) > 0


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("k_D", [1, 2.5])
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("G", [2, 4])
def test_every_single_group_build(monkeypatch, G, nbh, k_D, log):
    """The 16 instantiations of the form; with the episode log on, its records equal the loop
    form's (and there are some)."""
    state = (_pattern_state, G)
    ref, one = _both(monkeypatch, state, 32, nbh, k_D, G, log=log)
    assert ref["exits"] > 0
    if log:
        # an env that was injected empty is placed by its first step without ending an episode
        ended = int(((np.diff(ref["eps_hist"], axis=0) > 0) & (ref["pre_cnt"] > 0)).sum())
        assert len(one["rec"]) == ended > 0


@pytest.mark.parametrize("cand", [None, 0])
def test_placements_of_several_envs_of_one_group(monkeypatch, cand):
    """Several envs of one group empty in one step: the wave places them one after the other,
    every placed lane reading its cell from the free list (the retired 20 KB-carve build, rebuilt
    from commit 2113d5c as profiles/lds_fit/README.md says, read it from the image in global
    memory).  The default candidate pass, and FFM_RESET_CANDIDATES=0 (the full ranking)."""
    state = (_pattern_state, 4)
    ref = _oracle(state, "neumann", 1, 32)
    placed = np.diff(ref["eps_hist"], axis=0) > 0                                    # [T, E]
    n = placed.shape[1] // 4 * 4
    assert placed[:, :n].reshape(T, n // 4, 4).sum(axis=2).max() >= 2, "no step re-placed two envs of one group"
    _, one = _both(monkeypatch, state, 32, "neumann", 1, 4, FFM_RESET_CANDIDATES=cand)
    assert one["ctr"]["resets"] >= 2


def test_nothing_is_placed_without_auto_reset(monkeypatch):
    state = (_pattern_state, 4)
    ref = _oracle(state, "neumann", 1, 32, auto=False)
    _, cnt0 = _pattern_state(4)
    assert ((ref["cnt"] == 0) & (cnt0 > 0)).any(), "no env emptied"
    assert not ref["eps"].any()
    _, one = _both(monkeypatch, state, 32, "neumann", 1, 4, auto=False)
    assert one["ctr"]["resets"] == 0


def test_two_shards_equal_one_launch(monkeypatch):
    E = 1027
    state = (_random_state, E, 32)
    ref = _oracle(state, "neumann", 1, 32)
    two = _run(monkeypatch, state, 32, "neumann", 1, True, want={"step_shards": 2}, FFM_STEP_SHARDS=2)
    one = _run(monkeypatch, state, 32, "neumann", 1, True, want={"step_shards": 1}, FFM_STEP_SHARDS=1)
    _assert_same(two, one)
    _assert_oracle(two, ref)


def test_resident_blocks_per_cu(monkeypatch):
    """hipOccupancyMaxActiveBlocksPerMultiprocessor of the Neumann G = 4 kernels at their own LDS
    sizes.  The single-group form keeps the common carve (22,400 B: the 20,432 B carve that fits
    eight blocks measured slower and is not the product build, profiles/lds_fit/), so 7 blocks of
    its 56 VGPRs fit a CU's 160 KB; the loop form's registers hold 6, as before."""
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    if arch != "gfx950":
        pytest.skip(f"{arch}: the 160 KB of LDS per CU this counts with are gfx950's")
    from ffm_amd.engine import Engine
    _setenv(monkeypatch, FFM_GROUP_ENVS=4)
    m, s, _ = _room()
    eng = Engine(m, s, n_envs=64, n_agents=32, params=_params("neumann", 1), rng="philox", seed=SEED)
    try:
        assert eng.launch_info()["group_g"] == 4
        assert eng.group_occupancy(one=True) == 7
        assert eng.group_occupancy(one=False) == 6
    finally:
        eng.close()
