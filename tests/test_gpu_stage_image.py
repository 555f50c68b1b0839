"""The group kernel's engine-constant stage image and the prologue that reads it.

At create a group-kernel engine builds one device buffer with the bytes every workgroup used to
stage per launch (the padded map, f32(-k_S) * SFF, the padded free list, the widened map) and
the per-lane slot geometry of both group sizes; the kernel's prologue copies the first part to
LDS, initialises each wave's grids from it and clears only the tile halos.
Here: the image's bytes against a NumPy rebuild, the step against the oracle bit for bit over a
pairwise-covering set of shapes and switches, and a start from large DFF values on the border
rows and columns, where a halo that is not zero or a tile that leaks into its neighbour shows.
Every case is a 12x12 room.
"""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS")
SEED, T = 42, 120
H = W = 12
PW, PHW = W + 2, (H + 2) * (W + 2)
TS = 4 + (H + 2) * W + 4          # floats of one env's DFF tile


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


def _params(nbh, k_S=3, k_D=1):
    return {"k_S": k_S, "k_D": k_D, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


def _a16(n):
    return (n + 15) & ~15


# ---------------------------------------------------------------------------
# Image bytes
# ---------------------------------------------------------------------------
def _geom_table(G):
    """The per-lane geometry of a group of G envs (core_group.hip group_lane_geom): three arrays of
    one uint4 per lane, uint32 [3, 64, 4]."""
    Q4 = H * W // 4
    Q = G * Q4
    NS, NSF, HQ = -(-Q // 64), Q // 64, (4 + W) // 4
    out = np.zeros((3, 64, 4), np.int64)
    for lane in range(64):
        toff, lo, ro = [-1, -1, -1], [0, 0, 0], [0, 0, 0]
        yfl = senv = tail = tlo = tro = 0
        for k in range(NS):
            q = k * 64 + lane
            s = q // Q4
            c = 4 * (q - s * Q4)
            y = c % W
            ok = q < Q
            toff[k] = s * TS + 4 + W + c if ok else -1
            yfl |= (1 if ok and y == 0 else 0) << (2 * k)
            yfl |= (2 if ok and y == W - 4 else 0) << (2 * k)
            senv |= (s if ok else 15) << (4 * k)
            lo[k] = toff[k] - 1 if ok and y != 0 else 0          # 0: a zero word of the tile's halo
            ro[k] = toff[k] + 4 if ok and y != W - 4 else 0
        if Q % 64 != 0 and (Q % 64) * 4 == 64:                    # the scalar tail: one cell per lane
            q = 4 * 64 * NSF + lane
            s, c = divmod(q, H * W)
            y = c % W
            off = s * TS + 4 + W + c
            tail = (1 if y == 0 else 0) | (2 if y == W - 1 else 0)
            tlo = off - 1 if y != 0 else 0
            tro = off + 1 if y != W - 1 else 0
        s, j = divmod(lane, 2 * HQ)
        halo = s * (TS // 4) + (j if j < HQ else TS // 4 - 2 * HQ + j) if lane < G * 2 * HQ else 255
        out[0, lane] = toff + [yfl | senv << 8 | tail << 20 | halo << 24]
        out[1, lane] = [lo[0], ro[0], lo[1], ro[1]]
        out[2, lane] = [tlo, tro, lo[2], ro[2]]
    return (out & 0xFFFFFFFF).astype(np.uint32)


def _check_image(m, k_S):
    from ffm_amd.data import l1_sff
    from ffm_amd.engine import Engine
    sff = l1_sff(m)
    assert sff.dtype == np.float32
    eng = Engine(m, sff, n_envs=4, n_agents=8, params=_params("neumann", k_S=k_S), rng="philox", seed=SEED)
    assert eng.launch_info()["kernel"] == "group"
    img = eng.stage_image()
    eng.close()
    free = np.flatnonzero(m.reshape(-1) == 0)
    F = len(free)
    sizes = [_a16(PHW), _a16(PHW * 4), _a16(max(F, 1) * 2), _a16(PHW * 2)]
    shared = sum(sizes)
    assert shared % 16 == 0 and shared // 16 <= 256      # one 16-byte load per thread of the block
    assert len(img) == shared + 2 * 3 * 64 * 16
    o = np.concatenate([[0], np.cumsum(sizes)])
    pmap = np.full((H + 2, W + 2), 2, np.uint8)
    pmap[1:-1, 1:-1] = np.where(m == 0, 0, np.where(m == 3, 3, 2))
    psff = np.zeros((H + 2, W + 2), np.float32)
    psff[1:-1, 1:-1] = sff
    term = np.float32(-k_S) * psff.astype(np.float32)
    assert term.dtype == np.float32
    fpad = ((free // W + 1) * PW + free % W + 1).astype(np.uint16)     # the engine's own formula
    want = [pmap.reshape(-1), term.reshape(-1).view(np.uint32), fpad, pmap.reshape(-1).astype(np.uint16)]
    for i, w in enumerate(want):
        nb = w.size * w.itemsize
        got = img[o[i]:o[i] + nb].view(w.dtype)
        assert np.array_equal(got, w), f"region {i}"
        assert not img[o[i] + nb:o[i + 1]].any(), f"pad bytes of region {i}"
    tabs = img[shared:].view(np.uint32).reshape(2, 3, 64, 4)
    assert np.array_equal(tabs[0], _geom_table(2)), "geometry table, G = 2"
    assert np.array_equal(tabs[1], _geom_table(4)), "geometry table, G = 4"
    return F


@pytest.mark.parametrize("k_S", [3, 10, 0.37])
def test_image_bytes_default_room(k_S):
    from ffm_amd.data import make_room
    assert _check_image(make_room(H, W), k_S) == 100


def test_image_bytes_odd_free_list():
    """Interior obstacles: 93 free cells, an odd count (the free list's pad is 10 bytes)."""
    from ffm_amd.data import make_room
    m = make_room(H, W)
    m[5, 3:9] = 2
    m[8, 8] = 2
    F = _check_image(m, 3)
    assert F == 93 and F % 2 == 1 and F < 100


def test_other_kernels_have_no_image():
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    m = make_room(H, W)
    eng = Engine(m, l1_sff(m), n_envs=4, n_agents=8, params=_params("neumann"), envs_per_block=-2)
    assert eng.launch_info()["kernel"] == "lane"
    assert eng.stage_image().size == 0
    eng.close()


# ---------------------------------------------------------------------------
# Parity with the oracle, bit for bit
# ---------------------------------------------------------------------------
E_REF = 24
DIMS = [(1, 3, 8, 9, 17, 21),            # E
        (1, 7, 32),                      # N
        (2, 4),                          # FFM_GROUP_ENVS
        ("neumann", "moore"),
        (1, 2.5),                        # k_D (the KD1 = true / false builds)
        (3, 10),                         # k_S
        (None, 1)]                       # FFM_WAVE_BLOCKS


def _pairwise(dims):
    """A greedy pairwise-covering subset of the product (deterministic)."""
    pairs = {(i, a, j, b) for i, j in itertools.combinations(range(len(dims)), 2) for a in dims[i] for b in dims[j]}
    covers = lambda c: {(i, c[i], j, c[j]) for i, j in itertools.combinations(range(len(dims)), 2)}
    cases, todo = [], set(pairs)
    product = list(itertools.product(*dims))
    while todo:
        best = max(product, key=lambda c: len(covers(c) & todo))
        cases.append(best)
        todo -= covers(best)
    return cases


MATRIX = _pairwise(DIMS)


def test_matrix_covers_every_pair():
    assert len(MATRIX) <= 60
    for i, j in itertools.combinations(range(len(DIMS)), 2):
        want = {(a, b) for a in DIMS[i] for b in DIMS[j]}
        assert want <= {(c[i], c[j]) for c in MATRIX}, (i, j)


@functools.lru_cache(maxsize=None)
def _oracle(N, nbh, k_D, k_S):
    """The oracle from reset() for T steps, once per input point (envs are keyed by their global
    id, so the first E envs of the batch are the batch of E envs)."""
    from ffm_amd.data import make_room, l1_sff
    from oracle import oracle as O
    m = make_room(H, W)
    core = O.Core(m, l1_sff(m), _params(nbh, k_S, k_D))
    E = E_REF
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


def _episodes(eng):
    from ffm_amd.engine import _DevArray
    torch.cuda.synchronize()
    ptr = eng.device_buffers()["episodes"]
    return torch.as_tensor(_DevArray(ptr, eng.n_envs, "<i4"), device=f"cuda:{eng.device}").cpu().numpy().copy()


def _parity_case(monkeypatch, E, N, G, nbh, k_D, k_S, wave_blocks, shards=None):
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    _setenv(monkeypatch, FFM_GROUP_ENVS=G, FFM_WAVE_BLOCKS=wave_blocks, FFM_STEP_SHARDS=shards)
    m = make_room(H, W)
    eng = Engine(m, l1_sff(m), n_envs=E, n_agents=N, params=_params(nbh, k_S, k_D), rng="philox", seed=SEED,
                 auto_reset=True)
    li = eng.launch_info()
    groups = -(-E // G)
    blocks = 1 if wave_blocks else -(-groups // 4)
    assert (li["kernel"], li["group_g"], li["blocks"], li["block_size"]) == ("group", G, blocks, 256), li
    assert li["step_shards"] == (shards or 1), li
    eng.reset()
    eng.step(T)
    gpos, gcnt, gdff = eng.get_state()
    geps, ctr = _episodes(eng), eng.counters()
    eng.close()
    pos, cnt, dff, eps, agent_steps, exits = (a[:E] for a in _oracle(N, nbh, k_D, k_S))
    assert int(eps.sum()) > 0, "no placement ran: the image's free list was not used"
    assert np.array_equal(gcnt, cnt), "counts"
    for e in range(E):
        assert np.array_equal(gpos[e, :cnt[e]], pos[e, :cnt[e]]), f"env {e} positions"
    assert np.array_equal(gdff.view(np.uint32), dff.view(np.uint32)), "DFF bits"
    assert np.array_equal(geps, eps), "episodes"
    assert ctr == {"agent_steps": int(agent_steps.sum()), "exits": int(exits.sum()), "resets": int(eps.sum()),
                   "steps": T}
    return li


@pytest.mark.parametrize("E,N,G,nbh,k_D,k_S,wave_blocks", MATRIX)
def test_parity_matrix(monkeypatch, E, N, G, nbh, k_D, k_S, wave_blocks):
    _parity_case(monkeypatch, E, N, G, nbh, k_D, k_S, wave_blocks)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_full_group_then_one_env_partial_group(monkeypatch, nbh):
    """E = 17, G = 4, one block: wave 0 steps a full group, then the group of env 16 alone --
    where a halo-only clear or a stale tile would show."""
    li = _parity_case(monkeypatch, 17, 32, 4, nbh, 1, 3, 1)
    assert li["blocks"] == 1 and -(-17 // 4) == 5      # 5 groups on 4 waves


@pytest.mark.parametrize("G", [2, 4])
def test_two_shards(monkeypatch, G):
    """E = 24 as two env shards (16 + 8 envs), each a launch with its own prologue."""
    _parity_case(monkeypatch, 24, 32, G, "neumann", 1, 3, None, shards=2)


# ---------------------------------------------------------------------------
# Halo
# ---------------------------------------------------------------------------
HALO_E, HALO_T, HALO_T0 = 17, 3, 1000


@functools.lru_cache(maxsize=None)
def _halo_reference(nbh):
    """Large DFF values on all four border rows and columns of every env, agents on the cells
    next to them; the oracle's state HALO_T steps later."""
    from ffm_amd.data import make_room, l1_sff
    from oracle import oracle as O
    m = make_room(H, W)
    rng = np.random.default_rng(5)
    E, A = HALO_E, 32
    ring = np.array([x * W + y for x in range(1, H - 1) for y in range(1, W - 1)
                     if x in (1, H - 2) or y in (1, W - 2)], np.uint16)       # 36 cells
    pos0 = np.stack([rng.permutation(ring)[:A] for _ in range(E)]).astype(np.uint16)
    cnt0 = np.full(E, A, np.int32)
    dff0 = (rng.random((E, H, W)) * 2).astype(np.float32)
    border = np.zeros((H, W), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    dff0[:, border] = (50 + 450 * rng.random((E, int(border.sum())))).astype(np.float32)
    core = O.Core(m, l1_sff(m), _params(nbh))
    pos, cnt, dff = pos0.copy(), cnt0.copy(), dff0.copy()
    eps = np.zeros(E, np.int32)
    agent_steps = 0
    for t in range(HALO_T0, HALO_T0 + HALO_T):
        agent_steps += core.step_philox_batch(pos, cnt, dff, eps, SEED, t, True, A, 0, 16)
    for a in (pos0, cnt0, dff0, pos, cnt, dff, eps):
        a.setflags(write=False)
    return (pos0, cnt0, dff0), (pos, cnt, dff, eps, agent_steps)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("G", [2, 4])
def test_halo_with_large_border_dff(monkeypatch, G, nbh):
    """One block, so its waves step several groups each (G = 4: wave 0 a full group and the
    one-env partial group): the DFF bits change if a tile's halo is not zero or a staged
    tile reaches into the next env's."""
    from ffm_amd.data import make_room, l1_sff
    from ffm_amd.engine import Engine
    _setenv(monkeypatch, FFM_GROUP_ENVS=G, FFM_WAVE_BLOCKS=1)
    m = make_room(H, W)
    eng = Engine(m, l1_sff(m), n_envs=HALO_E, n_agents=32, params=_params(nbh), rng="philox", seed=SEED,
                 auto_reset=True)
    li = eng.launch_info()
    assert (li["kernel"], li["group_g"], li["blocks"]) == ("group", G, 1), li
    (pos0, cnt0, dff0), (pos, cnt, dff, eps, agent_steps) = _halo_reference(nbh)
    eng.set_state(0, positions=pos0, counts=cnt0, dff=dff0)
    eng.step_index = HALO_T0
    eng.step(HALO_T)
    gpos, gcnt, gdff = eng.get_state()
    ctr = eng.counters()
    eng.close()
    assert np.array_equal(gcnt, cnt), "counts"
    for e in range(HALO_E):
        assert np.array_equal(gpos[e, :cnt[e]], pos[e, :cnt[e]]), f"env {e} positions"
    assert np.array_equal(gdff.view(np.uint32), dff.view(np.uint32)), "DFF bits"
    assert ctr["agent_steps"] == agent_steps and ctr["resets"] == int(eps.sum()) and ctr["steps"] == HALO_T
