"""The group kernel's Neumann stencil, bit for bit, where a rework of it would go wrong.

update_dff (model/ffm_core.py:106-117) is B = c0 * D, A = B + sum over the neighbours of
c1 * B[nb], clamped below 1e-4.  The group kernel reads the neighbours from the wave's LDS tile
and forms the two products per operand.  A variant that forms B and C = c1 * B once per cell,
writes C over D in the tile and reads the neighbours' C back was measured and not landed
(profiles/decide_stencil/); these cases were written for it and hold for
any stencil that writes the tile or changes who computes what: a value left in a tile that a
partial group re-stages (E = 17 on one block: a full group, then the group of env 16 alone), a
neighbour read across the map's edge or into the next env's tile (large values on the border
rows and columns), the 1e-4 clamp (a patch of values that straddle it after one step), other
c0 / c1, and the zeroing of an env that ends and is re-placed in the stepped window.  Every case
is a 12x12 room.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS")
SEED, T0 = 42, 500
H = W = 12
E_REF, A = 17, 32
STEPS = (1, 2, 5)
RATES = ((0.2, 0.2), (0.05, 0.5))          # diffuse, decay


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _params(diffuse, decay):
    return {"k_S": 3, "k_D": 1, "diffuse": diffuse, "decay": decay, "neighborhood": "neumann"}


def _room():
    from ffm_amd.data import make_room, l1_sff
    m = make_room(H, W)
    return m, l1_sff(m)


CLAMP = (slice(4, 8), slice(6, 10))         # the patch of values around the clamp


@functools.lru_cache(maxsize=None)
def _start(kind):
    """"field": 32 agents per env on a random DFF of order 1 with values of 50..500 on the four
    border rows and columns and a 4x4 patch that straddles the 1e-4 clamp after one step.
    "ending": the same, but two envs of every three hold one or two agents next to the exit."""
    rng = np.random.default_rng(11)
    inner = np.array([x * W + y for x in range(1, H - 1) for y in range(1, W - 1)], np.uint16)
    dff0 = (rng.random((E_REF, H, W)) * 2).astype(np.float32)
    border = np.zeros((H, W), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    dff0[:, border] = (50 + 450 * rng.random((E_REF, int(border.sum())))).astype(np.float32)
    # c0 is 0.64 and 0.475 at the two settings: 0.4e-4 .. 4e-4 lands on both sides of 1e-4; the
    # patch lies in a zone of such values one cell wider, so its neighbours add a few 1e-5 only
    dff0[:, 3:9, 5:11] = (0.4e-4 + 3.6e-4 * rng.random((E_REF, 6, 6))).astype(np.float32)
    pos0 = np.stack([rng.permutation(inner)[:A] for _ in range(E_REF)]).astype(np.uint16)
    cnt0 = np.full(E_REF, A, np.int32)
    if kind == "ending":                    # every third env stays full
        few = np.arange(E_REF) % 3 != 2
        pos0[few, :2] = np.array([1 * W + 6, 2 * W + 6], np.uint16)      # below the exit at (0, 6)
        cnt0[few] = 1 + np.arange(E_REF)[few] % 2
    for a in (pos0, cnt0, dff0):
        a.setflags(write=False)
    return pos0, cnt0, dff0


@functools.lru_cache(maxsize=None)
def _reference(kind, diffuse, decay):
    """The oracle's state after each of STEPS steps from _start(kind), computed once."""
    from oracle import oracle as O
    m, s = _room()
    core = O.Core(m, s, _params(diffuse, decay))
    pos0, cnt0, dff0 = _start(kind)
    pos, cnt, dff = pos0.copy(), cnt0.copy(), dff0.copy()
    eps = np.zeros(E_REF, np.int32)
    out = {}
    for i in range(1, max(STEPS) + 1):
        core.step_philox_batch(pos, cnt, dff, eps, SEED, T0 + i - 1, True, A, 0, 8)
        if i in STEPS:
            out[i] = tuple(a.copy() for a in (pos, cnt, dff, eps))
            for a in out[i]:
                a.setflags(write=False)
    return out


def _run(monkeypatch, kind, G, E, diffuse, decay, steps):
    from ffm_amd.engine import Engine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FFM_GROUP_ENVS", str(G))
    monkeypatch.setenv("FFM_WAVE_BLOCKS", "1")
    m, s = _room()
    eng = Engine(m, s, n_envs=E, n_agents=A, params=_params(diffuse, decay), rng="philox", seed=SEED,
                 auto_reset=True)
    li = eng.launch_info()
    assert (li["kernel"], li["group_g"], li["blocks"]) == ("group", G, 1), li
    pos0, cnt0, dff0 = (a[:E] for a in _start(kind))
    eng.set_state(0, positions=pos0, counts=cnt0, dff=dff0)
    eng.step_index = T0
    eng.step(steps)
    gpos, gcnt, gdff = eng.get_state()
    resets = eng.counters()["resets"]
    eng.close()
    pos, cnt, dff, eps = (a[:E] for a in _reference(kind, diffuse, decay)[steps])
    assert np.array_equal(gcnt, cnt), "counts"
    for e in range(E):
        assert np.array_equal(gpos[e, :cnt[e]], pos[e, :cnt[e]]), f"env {e} positions"
    bad = np.argwhere(gdff.view(np.uint32) != dff.view(np.uint32))
    assert bad.size == 0, f"DFF bits differ at (env, x, y) {bad[:8].tolist()}"
    assert resets == int(eps.sum())
    return dff, eps


def test_start_straddles_the_clamp():
    """The inputs do what the docstring says: after one step the patch holds clamped zeros and
    kept values at both settings, and the border values stay large."""
    for diffuse, decay in RATES:
        dff = _reference("field", diffuse, decay)[1][2]
        patch = dff[(slice(None),) + CLAMP]
        assert (patch == 0).any() and (patch >= 1e-4).any()
        assert dff[:, 0, :].min() > 10 and dff[:, :, -1].min() > 10


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("diffuse,decay", RATES)
@pytest.mark.parametrize("E", [9, 17])
@pytest.mark.parametrize("G", [2, 4])
def test_stencil_bits(monkeypatch, G, E, diffuse, decay, steps):
    """One block: E = 9 is three groups (G = 4: two full, one of one env) on three waves, E = 17
    five groups on four waves (G = 4) or nine (G = 2): wave 0 re-stages its tile."""
    _run(monkeypatch, "field", G, E, diffuse, decay, steps)


@pytest.mark.parametrize("G", [2, 4])
def test_ended_envs_start_at_zero(monkeypatch, G):
    """Envs that end inside the window are re-placed and their DFF zeroed by the stencil's
    stores; their neighbours in the group keep theirs."""
    dff, eps = _run(monkeypatch, "ending", G, E_REF, 0.2, 0.2, max(STEPS))
    assert 0 < int((eps > 0).sum()) and (eps == 0).any(), "the window holds ended and running envs"
