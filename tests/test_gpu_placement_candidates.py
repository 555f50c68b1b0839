"""The placement's candidate pass (wave_reset.h, free lists of <= 128 cells).

A placement ranks only the (key, j) pairs whose key is below a threshold fixed at create,
thr = floor(M * 2^32 / F) with M = min(F, N + max(8, (N + 1) / 2)), when N <= C <= 64 of them
are; otherwise it ranks all F pairs as before.  FFM_RESET_CANDIDATES=<M> (read at create)
overrides M, which makes every branch reachable with the product library:

  * unset: the product rule, nearly always the candidate pass;
  * 1:     about one candidate, so C < N and the full ranking (N = 2 now and then gets C >= 2);
  * F:     every key is a candidate: C = F > 64 in the plain and obstacle rooms (full ranking),
           and the candidate pass ranking everything in the walled room (F = 47: an odd count,
           so the ~0 pad word is read; the product rule gives M == F there for N = 32 too);
  * 0:     no candidate pass.

Every setting must give the oracle's positions, counts and DFF bit for bit, and the getter must
report the M and thr in effect.  The fused multi-step kernel is built without the candidate pass
(it costs that kernel a VGPR); its case checks that it still places as the oracle does.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS", "FFM_RESET_CANDIDATES")
SEED = 42
SETTINGS = ("unset", "1", "F", "0")
SHAPES = ((37, 2, 60), (37, 5, 60), (64, 32, 250))      # (E, N, T)


def _params():
    return {"k_S": 3, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}


@functools.lru_cache(maxsize=None)
def _room(room):
    from ffm_amd.data import make_room, l1_sff
    if room == "lane8":          # 8x8: the lane kernel (the group kernel steps 12x12 rooms only)
        m = make_room(8, 8)
    else:
        m = make_room(12, 12)
    if room == "obstacle":       # as test_gpu_decide_exact._room: an inner wall, a pillar, two exits
        m[6, 1:9] = 2
        m[3:5, 4:6] = 2
        m[8, 0] = 3
    if room == "walled":         # the lower half walled off and three more cells: F = 47
        m[6:11, 1:11] = 2
        m[5, 1:4] = 2
    s = l1_sff(m)
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


def _free(room):
    return int((_room(room)[0] == 0).sum())


def _expected(setting, N, F):
    """(M, thr) the engine must report."""
    M = min(F, N + max(8, (N + 1) // 2))
    if setting != "unset":
        M = max(0, min(F, F if setting == "F" else int(setting)))
    thr = 0 if M == 0 else 0xFFFFFFFF if M == F else (M << 32) // F
    return M, thr


@functools.lru_cache(maxsize=None)
def _oracle_reset(room, E, N):
    from oracle import oracle as O
    m, s = _room(room)
    core = O.Core(m, s, _params())
    pos = np.stack([core.reset_philox(N, SEED, 0, e) for e in range(E)])
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def _oracle(room, E, N, T):
    from oracle import oracle as O
    m, s = _room(room)
    H, W = m.shape
    core = O.Core(m, s, _params())
    pos = _oracle_reset(room, E, N).copy()
    cnt = np.full(E, N, np.int32)
    dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    for t in range(1, 1 + T):
        core.step_philox_batch(pos, cnt, dff, eps, SEED, t, True, N, 0, 16)
    for a in (pos, cnt, dff, eps):
        a.setflags(write=False)
    return pos, cnt, dff, eps


def _engine(monkeypatch, room, E, N, setting, G=None, wave_blocks=None, envs_per_block=0):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ffm_amd.engine import Engine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    F = _free(room)
    if setting != "unset":
        monkeypatch.setenv("FFM_RESET_CANDIDATES", str(F) if setting == "F" else setting)
    if G:
        monkeypatch.setenv("FFM_GROUP_ENVS", str(G))
    if wave_blocks:
        monkeypatch.setenv("FFM_WAVE_BLOCKS", str(wave_blocks))
    m, s = _room(room)
    eng = Engine(m, s, n_envs=E, n_agents=N, params=_params(), rng="philox", seed=SEED, auto_reset=True,
                 envs_per_block=envs_per_block)
    M, thr = _expected(setting, N, F)
    assert eng.reset_candidates() == {"M": M, "thr": thr}
    return eng


def _check_steps(eng, room, E, N, T):
    eng.reset()
    eng.step(T)
    gpos, gcnt, gdff = eng.get_state()
    eng.close()
    pos, cnt, dff, eps = _oracle(room, E, N, T)
    # (the obstacle room's inner wall traps agents, the SFF being plain L1 distance: with 32 of
    # them no env empties, and that case checks the first placement and the stepping only)
    assert int(eps.sum()) >= E or room == "obstacle", "the run must re-place envs"
    assert np.array_equal(gcnt, cnt), f"counts differ in envs {np.flatnonzero(gcnt != cnt)[:8].tolist()}"
    for e in range(E):
        assert np.array_equal(gpos[e, :cnt[e]], pos[e, :cnt[e]]), f"env {e} positions"
    bad = np.argwhere(gdff.view(np.uint32) != dff.view(np.uint32))
    assert not bad.size, f"DFF bits differ at (env, x, y) {bad[:8].tolist()}"


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("E,N,T", SHAPES)
@pytest.mark.parametrize("room", ["plain", "obstacle", "walled"])
def test_group_kernel(monkeypatch, room, E, N, T, G, setting):
    eng = _engine(monkeypatch, room, E, N, setting, G=G)
    li = eng.launch_info()
    assert (li["kernel"], li["group_g"]) == ("group", G), li
    _check_steps(eng, room, E, N, T)


@pytest.mark.parametrize("setting", SETTINGS)
def test_one_block_many_pending(monkeypatch, setting):
    """One block of four waves steps all 64 envs: a wave carries several deferred placements."""
    eng = _engine(monkeypatch, "plain", 64, 32, setting, G=4, wave_blocks=1)
    li = eng.launch_info()
    assert (li["kernel"], li["group_g"], li["blocks"]) == ("group", 4, 1), li
    _check_steps(eng, "plain", 64, 32, 250)


@pytest.mark.parametrize("setting", SETTINGS)
def test_lane_kernel(monkeypatch, setting):
    eng = _engine(monkeypatch, "lane8", 37, 5, setting)
    assert eng.launch_info()["kernel"] == "lane"
    _check_steps(eng, "lane8", 37, 5, 60)


@pytest.mark.parametrize("setting", SETTINGS)
def test_wave_kernel(monkeypatch, setting):
    eng = _engine(monkeypatch, "plain", 37, 5, setting, envs_per_block=-1)
    assert eng.launch_info()["kernel"] == "wave"
    _check_steps(eng, "plain", 37, 5, 60)


@pytest.mark.parametrize("setting", SETTINGS)
def test_fused_steps(monkeypatch, setting):
    eng = _engine(monkeypatch, "plain", 37, 5, setting)
    assert eng.launch_info()["multi"]
    eng.set_fused_steps(5)
    _check_steps(eng, "plain", 37, 5, 60)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("N", [5, 32])
@pytest.mark.parametrize("room", ["plain", "obstacle", "walled"])
def test_reset_alone(monkeypatch, room, N, setting):
    """reset() places every env by core_reset_kernel: the oracle's reset_philox at t = 0."""
    E = 64
    eng = _engine(monkeypatch, room, E, N, setting)
    eng.reset()
    gpos, gcnt, gdff = eng.get_state()
    eng.close()
    assert np.array_equal(gcnt, np.full(E, N, np.int32))
    assert np.array_equal(gpos[:, :N], _oracle_reset(room, E, N))
    assert not gdff.any()
