"""Per-env parameters on the group kernel's own per-env form (Engine.set_env_params(..., kernel="group")).

The contract is that of tests/test_gpu_env_params.py (its oracle mirror and helpers are used here):
env e of an engine with per-env parameters evolves bit for bit like the env with the same global
id of a homogeneous engine created with its set.  Here the 12x12 engine stays on the group kernel
while the feature is on, in both of its forms (one group per wave, and the loop), both group
sizes, both neighbourhoods, with and without the episode log, and with step shards.  Every case
asserts the kernel, the envs per group, the form and the shard count through launch_info()
before it compares anything.  Compared exactly: positions of the live agents, counts, DFF bits,
episodes, the agent_steps / resets counters and the episode-log records.

The base workload is the other file's: 12x12, 32 agent slots, 135 envs (odd, no multiple of 4),
the five sets of SETS5 (5 is coprime to 2 and 4: every set meets every position of a group; the
k_D values 1, 0, 2.5, 1, 4 and the N values 32, 5, 17, 1, 24 sit inside one group), 120 steps.
"""
import numpy as np
import pytest

from test_gpu_env_params import _oracle, _engine, _dicts, _snapshot, _assert_same, _assert_resets, SETS5, SETS5_B, SEED
from test_gpu_env_params import SETS3

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_GROUP_ENVS", "FFM_GROUP_ONE", "FFM_WAVE_BLOCKS", "FFM_STEP_SHARDS")
E, T = 135, 120


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _setenv(monkeypatch, G=None, one=True, blocks=None, shards=None):
    """The switches are read when the engine is created and when the per-env form's geometry is taken."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("FFM_GROUP_ENVS", G), ("FFM_GROUP_ONE", None if one else 0), ("FFM_WAVE_BLOCKS", blocks),
                 ("FFM_STEP_SHARDS", shards)):
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _group_engine(nbh, n_envs=E, create=SETS5[0], env_base=0):
    eng = _engine(12, 12, 32, nbh, n_envs, create, 0, env_base=env_base)
    assert eng.launch_info()["kernel"] == "group"
    return eng


def _assert_group(eng, G, one, shards=1, blocks=None):
    info = eng.launch_info()
    assert info["kernel"] == "group", info
    assert info["group_g"] == G and info["group_one"] == one and info["step_shards"] == shards, info
    if blocks is not None:
        assert info["blocks"] == blocks, info
    return info


def _run_group(monkeypatch, nbh, G, one, n_envs=E, steps=T, blocks=None, sets=SETS5, log=False):
    _setenv(monkeypatch, G=G, one=one, blocks=blocks)
    eng = _group_engine(nbh, n_envs)
    try:
        eng.set_env_params(_dicts(sets), kernel="group")
        _assert_group(eng, G, one, blocks=blocks)
        if log:
            eng.set_episode_log(capacity=n_envs * steps)
        eng.reset()
        eng.step(steps)
        got = _snapshot(eng)
        rec = eng.drain_episodes() if log else None
    finally:
        eng.close()
    return got, rec


# 1. against the oracle: both neighbourhoods, both group sizes, both forms
@pytest.mark.parametrize("one", [True, False], ids=["one", "loop"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_group_path_matches_oracle(monkeypatch, nbh, G, one):
    got, _ = _run_group(monkeypatch, nbh, G, one)
    (want,), _ = _oracle(12, 12, 32, nbh, E, SETS5, (("step", T), ("snap",)))
    _assert_resets(want["eps"], SETS5, (0, 1, 2, 3))
    _assert_same(got, want, f"{nbh} G={G} {'one' if one else 'loop'}")


# the loop form on one block: 34 groups on 4 waves, up to 9 iterations per wave -- prefetched
# records, and the deferred placement tail with per-env N
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_loop_form_many_iterations(monkeypatch, nbh):
    got, _ = _run_group(monkeypatch, nbh, 4, False, blocks=1)
    (want,), _ = _oracle(12, 12, 32, nbh, E, SETS5, (("step", T), ("snap",)))
    _assert_resets(want["eps"], SETS5, (0, 1, 2, 3))
    _assert_same(got, want, f"{nbh} loop, 1 block")


# fewer envs than a group, and a partial only / last group
@pytest.mark.parametrize("one", [True, False], ids=["one", "loop"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("n_envs", [1, 3, 7])
def test_partial_groups(monkeypatch, n_envs, G, one):
    sets = SETS5[:n_envs] if n_envs < 5 else SETS5
    got, _ = _run_group(monkeypatch, "neumann", G, one, n_envs=n_envs, steps=40, sets=sets)
    (want,), _ = _oracle(12, 12, 32, "neumann", n_envs, sets, (("step", 40), ("snap",)))
    _assert_same(got, want, f"E={n_envs} G={G}")


# 2. the same engine on the lane path, and homogeneous group engines with the same global ids
@pytest.mark.parametrize("env_base", [0, 1000])
def test_equal_to_lane_path_and_homogeneous_engines(monkeypatch, env_base):
    nbh = "neumann"
    _setenv(monkeypatch, G=4)
    snaps = {}
    for kernel in ("group", "lane"):
        het = _group_engine(nbh, env_base=env_base)
        try:
            het.set_env_params(_dicts(SETS5), kernel=kernel)
            if kernel == "group":
                _assert_group(het, 4, True)
            else:
                assert het.launch_info()["kernel"] == "lane" and het.launch_info()["step_shards"] == 1
            het.reset()
            het.step(T)
            snaps[kernel] = _snapshot(het)
        finally:
            het.close()
    _assert_same(snaps["group"], snaps["lane"], "group path against lane path")
    got = snaps["group"]
    for p, st in enumerate(SETS5):
        hom = _group_engine(nbh, create=st, env_base=env_base)
        try:
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


# 3. step shards: each shard's launch takes its own slice of the records
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("S", [2, 3])
def test_step_shards(monkeypatch, S, G):
    nbh = "neumann"
    runs = {}
    for shards in (1, S):
        _setenv(monkeypatch, G=G, shards=shards)
        eng = _group_engine(nbh)
        try:
            eng.set_env_params(_dicts(SETS5), kernel="group")
            _assert_group(eng, G, True, shards=shards)
            eng.reset()
            for _ in range(10):
                eng.step(12)
            runs[shards] = _snapshot(eng)
        finally:
            eng.close()
    (want,), _ = _oracle(12, 12, 32, nbh, E, SETS5, (("step", T), ("snap",)))
    _assert_same(runs[S], runs[1], f"{S} shards against one launch")
    _assert_same(runs[S], want, f"{S} shards against the oracle")


# 4. switches: lane -> group -> lane -> off, mid-run; identity
def test_switches_mid_run(monkeypatch):
    nbh = "neumann"
    _setenv(monkeypatch, G=4)
    eng = _group_engine(nbh)
    got = []
    try:
        created = eng.launch_info()
        eng.set_env_params(_dicts(SETS5))
        assert eng.launch_info()["kernel"] == "lane" and eng.launch_info()["step_shards"] == 1
        eng.reset()
        eng.step(30)
        got.append(_snapshot(eng))
        eng.set_env_params(_dicts(SETS5), kernel="group")
        _assert_group(eng, 4, True)
        eng.step(30)
        got.append(_snapshot(eng))
        eng.set_env_params(_dicts(SETS5), kernel="lane")
        assert eng.launch_info()["kernel"] == "lane"
        eng.step(30)
        got.append(_snapshot(eng))
        eng.set_env_params(None)
        assert eng.launch_info() == created
        assert eng.env_params() == ([], None)
        eng.step(30)
        got.append(_snapshot(eng))
    finally:
        eng.close()
    ops = (("step", 30), ("snap",), ("step", 30), ("snap",), ("step", 30), ("snap",), ("sets", (SETS5[0],)), ("step", 30),
           ("snap",))
    want, _ = _oracle(12, 12, 32, nbh, E, SETS5, ops)
    for i, what in enumerate(("lane", "group", "lane again", "off")):
        _assert_same(got[i], want[i], what)


def test_identity_on_group_path(monkeypatch):
    nbh, st = "neumann", SETS5[0]
    _setenv(monkeypatch, G=4)
    a, b = _group_engine(nbh), _group_engine(nbh)
    try:
        created = a.launch_info()
        a.set_env_params(_dicts([st, st]), kernel="group")
        _assert_group(a, 4, True)
        for eng in (a, b):
            eng.reset()
            eng.step(60)
        _assert_same(_snapshot(a), _snapshot(b), "identity")
        a.set_env_params(None)
        assert a.launch_info() == created
        for eng in (a, b):
            eng.step(60)
        _assert_same(_snapshot(a), _snapshot(b), "after the off switch")
    finally:
        a.close()
        b.close()


# 5. new sets mid-run (parameters at once, N at the next placement) and reset_envs
@pytest.mark.parametrize("one", [True, False], ids=["one", "loop"])
def test_mid_run_change(monkeypatch, one):
    nbh = "neumann"
    _setenv(monkeypatch, G=4, one=one)
    eng = _group_engine(nbh)
    try:
        eng.set_env_params(_dicts(SETS5), kernel="group")
        _assert_group(eng, 4, one)
        eng.reset()
        eng.step(60)
        eng.set_env_params(_dicts(SETS5_B))
        _assert_group(eng, 4, one)
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


def test_reset_envs_places_own_n(monkeypatch):
    nbh = "neumann"
    mask = tuple(int(v) for v in (np.random.RandomState(7).rand(E) < 1 / 3))
    assert 0 < sum(mask) < E
    _setenv(monkeypatch, G=4)
    eng = _group_engine(nbh)
    try:
        eng.set_env_params(_dicts(SETS5), kernel="group")
        _assert_group(eng, 4, True)
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


# 6. the episode log through the EPL x PEP builds
@pytest.mark.parametrize("one", [True, False], ids=["one", "loop"])
@pytest.mark.parametrize("G", [2, 4])
def test_episode_log_records(monkeypatch, G, one):
    nbh = "neumann"
    got, rec = _run_group(monkeypatch, nbh, G, one, log=True)
    (want,), wrec = _oracle(12, 12, 32, nbh, E, SETS5, (("step", T), ("snap",)))
    _assert_same(got, want, "state with the log on")
    rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
    assert len(wrec) > 0 and np.array_equal(rec, wrec)


def test_run_episodes_returns_per_env_lengths(monkeypatch):
    n_envs, nbh = 40, "moore"          # Moore: every set, the k_D-dominated one included, ends episodes
    _setenv(monkeypatch, G=4)
    eng = _group_engine(nbh, n_envs)
    try:
        eng.set_env_params(_dicts(SETS5), kernel="group")
        _assert_group(eng, 4, True)
        eng.reset()
        steps = eng.run_episodes(per_env=2, max_steps=4000, chunk=16)
    finally:
        eng.close()
    _, want = _oracle(12, 12, 32, nbh, n_envs, SETS5, (("step", int(steps.sum(axis=1).max())), ("snap",)))
    for e in range(n_envs):
        mine = want[want[:, 0] == e]
        assert np.array_equal(steps[e], mine[:2, 2]), f"env {e}"


# 7. update_dff() on a group-path engine
@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_update_dff_per_env(monkeypatch, nbh):
    n_envs = 23
    _setenv(monkeypatch, G=4)
    eng = _group_engine(nbh, n_envs)
    try:
        eng.set_env_params(_dicts(SETS5), kernel="group")
        _assert_group(eng, 4, True)
        eng.reset()
        eng.step(20)
        eng.update_dff()
        got = _snapshot(eng)
    finally:
        eng.close()
    (want,), _ = _oracle(12, 12, 32, nbh, n_envs, SETS5, (("step", 20), ("update_dff",), ("snap",)))
    assert want["dff"].any()
    _assert_same(got, want, "update_dff")


# 8. refusals leave the engine as it was
def test_errors_leave_engine_unchanged(monkeypatch):
    _setenv(monkeypatch)
    st = SETS5[0]
    lane = _engine(12, 12, 32, "neumann", 16, st, -2)
    block = _engine(20, 20, 24, "neumann", 8, SETS3[0], 0)
    mt = _engine(12, 12, 32, "neumann", 2, st, rng="mt")
    try:
        assert lane.launch_info()["kernel"] == "lane" and block.launch_info()["kernel"] == "block"
        for eng, sets in ((lane, SETS5[:2]), (block, SETS3[:2]), (mt, SETS5[:2])):
            info, params = eng.launch_info(), eng.env_params()
            assert params == ([], None)
            with pytest.raises(NotImplementedError):
                eng.set_env_params(_dicts(sets), kernel="group")
            assert eng.launch_info() == info and eng.env_params() == ([], None)
        # ... also with the feature on
        lane.set_env_params(_dicts(SETS5[:2]))
        info, (sets, soe) = lane.launch_info(), lane.env_params()
        with pytest.raises(NotImplementedError):
            lane.set_env_params(_dicts(SETS5[2:4]), kernel="group")
        assert lane.launch_info() == info
        s2, soe2 = lane.env_params()
        assert s2 == sets and np.array_equal(soe2, soe)
        with pytest.raises(ValueError):
            lane.set_env_params(_dicts(SETS5[:2]), kernel="wave")
        assert lane.launch_info() == info
    finally:
        lane.close()
        block.close()
        mt.close()
    # a group engine: bad tables with kernel="group" leave the kernel setting alone too
    _setenv(monkeypatch, G=4)
    eng = _group_engine("neumann", 16)
    try:
        eng.set_env_params(_dicts(SETS5[:2]))
        info = eng.launch_info()
        assert info["kernel"] == "lane"
        with pytest.raises(ValueError):
            eng.set_env_params([{"n_agents": 0}], kernel="group")
        assert eng.launch_info() == info
        eng.set_env_params(_dicts(SETS5[:2]))          # kernel=None: the setting (lane) stays
        assert eng.launch_info() == info
    finally:
        eng.close()


# 9. the evac driver: the same files on either kernel (summary.txt but for its wall-clock rate)
def test_evac_outputs_do_not_depend_on_sweep_kernel(monkeypatch, tmp_path, capsys):
    from ffm_amd import evac
    _setenv(monkeypatch)
    out = {}
    for kernel in ("lane", "group", None):
        d = tmp_path / str(kernel)
        argv = ["--room", "12", "12", "--envs", "40", "--episodes", "2", "--sweep", "N=5,17", "--sweep", "k_D=0,2.5",
                "--out", str(d)] + (["--sweep-kernel", kernel] if kernel else [])
        evac.main(argv)
        files = {}
        for name in ("steps_per_episode.csv", "sweep_summary.csv", "summary.txt"):
            text = (d / name).read_text()
            files[name] = "\n".join(ln for ln in text.splitlines() if not ln.startswith("steps_per_second"))
        out[kernel] = files
    capsys.readouterr()
    assert len(out["lane"]["steps_per_episode.csv"].splitlines()) == 1 + 40 * 2
    assert out["group"] == out["lane"] and out[None] == out["lane"]
