"""The step's no-request branch on every kernel form, in Philox mode.

model/ffm_core.py:82 reads `if np.isfinite(probs_sum) and probs_sum != 0:`; an agent that fails it
takes no draw, makes no request and adds nothing to the DFF.  A kernel without the branch lets the
agent "stay", which is a granted request for its own cell: the DFF there gains 1 every step, leaks
into the room through update_dff and changes what the other agents decide.  Three families reach
the branch (tests/no_request_util.py):

  pocket     six free cells that reach no exit, inf in the geodesic SFF: -inf - (-inf), and with
             k_S = 0 the product 0 * inf; with auto-reset on, placements put agents there again;
  overflow   one DFF cell at 3e38 with k_D = 8: the product is +inf in float32, +inf - (+inf);
  diag       a cell that diagonal moves alone reach, inf in the Neumann field under Moore movement:
             a -inf score beside finite ones is a candidate of probability exactly 0 and the sum
             stays finite -- the branch must NOT be taken (a test for "some score is not finite"
             would freeze these agents).

Every case compares positions, counts, DFF bits, episodes and counters with the oracle mirror bit
for bit.  tests/test_no_request_fixtures.py shows on the CPU that every case below takes the branch
as often as FLOORS asks; the tables here are what it reads.
"""
import functools

import numpy as np
import pytest

import no_request_util as U
import rare_philox_util as R
from test_gpu_rare_philox import BASE_FORMS, FORMS, _case, _layout

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x5DEECE66D1234567
T0 = 77                     # the step index of the reset() that places every env
N = 32
_id = lambda v: v if isinstance(v, str) else None


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


# ---------------------------------------------------------------------------
# Pocket and diagonal cell: from reset(), auto-reset on
# ---------------------------------------------------------------------------
ROOM_FORMS = ("group_room", "lane_room", "block_room")
POCKET_FORMS = BASE_FORMS + ("group_loop", "group_pep", "lane_pep") + ROOM_FORMS
# (form, neighbourhood, k_S, E, T): about two pocket agents per env and step at N = 32 (fewer under
# the per-env sets' own N of the pep forms, and in one env of three of the room forms), so E * T is
# sized for the floor of 1,000; the fused form's T is a multiple of its 4 steps
_SHAPES = {"group_g2": (129, 12), "group_g4": (513, 8), "lane": (257, 8), "wave": (64, 40), "block3": (130, 12),
           "fused4": (257, 8), "group_loop": (129, 16), "group_pep": (257, 16), "lane_pep": (513, 8),
           "group_room": (513, 16), "lane_room": (385, 24), "block_room": (257, 40)}
POCKET_CASES = [(f, nbh, 3) + _SHAPES[f] for f in POCKET_FORMS for nbh in ("neumann", "moore")] + \
               [(f, nbh, 0) + _SHAPES[f] for f, nbh in (("group_g4", "neumann"), ("lane", "moore"), ("wave", "neumann"),
                                                        ("block3", "moore"), ("fused4", "neumann"))]
DIAG_CASES = [(f, 64, 16) for f in BASE_FORMS]


def pocket_rooms(nbh, dtype="float32"):
    """The pocket room first; the room forms put a plain and an obstacle room beside it."""
    from ffm_amd.data import l1_sff, make_room
    from test_gpu_geometry import obstacle_room
    m1, m2 = make_room(12, 12), obstacle_room(12, 12)
    return [U.pocket_room(nbh, dtype), (m1, l1_sff(m1)), (m2, l1_sff(m2))]


def pocket_args(form_id, nbh, k_S, E, dtype="float32"):
    return (form_id, pocket_rooms(nbh, dtype), U.params(nbh, k_S), E, N, 0, 0, SEED)


def diag_args(form_id, E):
    return (form_id, [U.diag_room()], U.params("moore"), E, N, 0, 0, SEED)


@functools.lru_cache(maxsize=None)
def branch_counts(kind, *case):
    """(no-request, boxed-in, non-finite-candidate) agent-steps of a case's oracle run."""
    if kind == "overflow":
        return _overflow_mirror(*case)[1]
    args = pocket_args(*case[:4]) if kind == "pocket" else pocket_args(*case[:4], dtype="float64") \
        if kind == "pocket_f64" else diag_args(*case[:2])
    mir = _layout(*args)[4]
    mir.reset(T0)
    return U.count_mirror(mir, T0 + 1, case[-1])


def _from_reset(eng, mir, form_id, T):
    try:
        eng.step_index = T0
        eng.reset()
        mir.reset(T0)
        R.assert_engine_equals(eng, mir, "reset()")
        mir.step(T0 + 1, T)
        if FORMS[form_id]["fused"] > 1:
            eng.set_fused_steps(FORMS[form_id]["fused"])
        eng.step(T)
        R.assert_engine_equals(eng, mir, f"{T} steps after reset()")
        assert eng.step_index == T0 + 1 + T
    finally:
        eng.close()


@pytest.mark.parametrize("form_id,nbh,k_S,E,T", POCKET_CASES, ids=_id)
def test_pocket_agents_make_no_request(monkeypatch, form_id, nbh, k_S, E, T):
    """Every candidate of an agent in the pocket scores -inf (k_S = 0: NaN): it stays without a
    request, its cell's DFF gains nothing, and the env's episode never ends."""
    assert branch_counts("pocket", form_id, nbh, k_S, E, T)[0] >= U.FLOORS["pocket"]
    eng, mir = _case(monkeypatch, *pocket_args(form_id, nbh, k_S, E))
    _from_reset(eng, mir, form_id, T)


F64_CASE = ("block3", "neumann", 3, 129, 12)


def test_pocket_float64_sff_block_kernel(monkeypatch):
    """The float64 arm of decide(): main.py's SFF dtype, on the block kernel."""
    form_id, nbh, k_S, E, T = F64_CASE
    assert branch_counts("pocket_f64", *F64_CASE)[0] >= U.FLOORS["pocket"]
    eng, mir = _case(monkeypatch, *pocket_args(form_id, nbh, k_S, E, dtype="float64"))
    assert mir.cores[0].sff64 is not None
    _from_reset(eng, mir, form_id, T)


@pytest.mark.parametrize("form_id,E,T", DIAG_CASES, ids=_id)
def test_zero_probability_candidates_still_request(monkeypatch, form_id, E, T):
    """A -inf score beside finite ones: the candidate has probability exactly 0 (the agent on the
    cell moves off it at once, nobody moves onto it), and nobody takes the branch."""
    nr, _, nonfinite = branch_counts("diag", form_id, E, T)
    assert nr == 0 and nonfinite >= U.FLOORS["diag"]
    eng, mir = _case(monkeypatch, *diag_args(form_id, E))
    _from_reset(eng, mir, form_id, T)


# ---------------------------------------------------------------------------
# Overflow: injected with set_state, as test_gpu_geometry's injected states
# ---------------------------------------------------------------------------
OVERFLOW_E, OVERFLOW_T = 129, 8
OVERFLOW_CASES = [(f, nbh) for f in BASE_FORMS for nbh in ("neumann", "moore")]


def _overflow_states(nbh, E):
    """Env e: the ring around the hot cell (every fourth env: an agent on it), its own shuffle."""
    from ffm_amd.data import make_room
    m = make_room(12, 12)
    pos = np.full((E, R.A), 0xFFFF, np.uint16)
    dff = np.zeros((E,) + m.shape, np.float32)
    for e in range(E):
        pos[e, :N], dff[e] = U.overflow_state(m, 4 if nbh == "neumann" else 8, e % 4 == 3, 5000 + e, n=N)
    return pos, np.full(E, N, np.int32), dff


def overflow_args(form_id, nbh):
    from ffm_amd.data import l1_sff, make_room
    m = make_room(12, 12)
    return (form_id, [(m, l1_sff(m))], U.params(nbh, 3, 8), OVERFLOW_E, N, 0, 0, SEED)


@functools.lru_cache(maxsize=None)
def _overflow_mirror(form_id, nbh):
    """(mirror after the run, its branch counts): every env starts from an injected state.  Shared, read only."""
    mir = _layout(*overflow_args(form_id, nbh))[4]
    mir.reset(T0)
    pos, cnt, dff = _overflow_states(nbh, OVERFLOW_E)
    for e in range(OVERFLOW_E):
        mir.set_env(e, pos[e], int(cnt[e]), dff[e])
    return mir, U.count_mirror(mir, T0 + 1, OVERFLOW_T)


@pytest.mark.parametrize("form_id,nbh", OVERFLOW_CASES, ids=_id)
def test_dff_product_overflow(monkeypatch, form_id, nbh):
    """k_D * DFF = +inf on one candidate: no request from the agents around the cell (or on it)
    while the cell stays above f32 max / 8 (four steps at decay = diffuse = 0.2), then ordinary
    steps on a DFF of 1e36 and more; the fused form takes the 8 steps as two launches of 4."""
    assert branch_counts("overflow", form_id, nbh)[0] >= U.FLOORS["overflow"]
    eng, _ = _case(monkeypatch, *overflow_args(form_id, nbh))
    mir, _ = _overflow_mirror(form_id, nbh)
    try:
        eng.step_index = T0
        eng.reset()
        pos, cnt, dff = _overflow_states(nbh, OVERFLOW_E)
        eng.set_state(0, positions=pos, counts=cnt, dff=dff)
        if FORMS[form_id]["fused"] > 1:
            eng.set_fused_steps(FORMS[form_id]["fused"])
        eng.step(OVERFLOW_T)
        R.assert_engine_equals(eng, mir, f"{OVERFLOW_T} steps from the injected state")
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Observers: a frozen agent is inside, and never exits
# ---------------------------------------------------------------------------
OBS_CASE = ("group_g2", "neumann", 3, 129, 24)
OBS_BINS = 16


def test_observers_count_frozen_agents_inside(monkeypatch):
    """Field statistics and exit flow on, one class: the occupancy map holds the pocket's agents at
    every observed step, `remaining` counts them, and the doors count only the agents that left."""
    from exit_flow_mirror import default_doors, door_from, leavers
    from test_gpu_field_stats import KEYS, _want
    form_id, nbh, k_S, E, T = OBS_CASE
    eng, mir = _case(monkeypatch, *pocket_args(form_id, nbh, k_S, E))
    m = mir.cores[0].map
    W = m.shape[1]
    dfrom = door_from(m, default_doors(m), nbh).reshape(-1)
    try:
        eng.set_field_stats(None, 1, OBS_BINS)
        eng.set_exit_flow(None, None, 1, OBS_BINS)
        eng.step_index = T0
        eng.reset()
        mir.reset(T0)
        obs, exited, outflow = [], 0, np.zeros(OBS_BINS, np.uint64)
        for k in range(T):
            t = T0 + 1 + k
            before = [(mir.pos[e, :mir.cnt[e]].astype(np.int64), int(mir.eps[e]), int(mir.start[e])) for e in range(E)]
            mir.step(t, 1)
            obs.append((mir.pos.copy(), mir.cnt.copy(), t - mir.start))      # an env re-placed in this step: tau = 0
            for e, (P, k0, start) in enumerate(before):
                n = int(mir.cnt[e])
                gone = leavers(P, mir.pos[e, :n].astype(np.int64), dfrom, W, nbh, len(P) > 0 and mir.eps[e] != k0)
                exited += len(gone)
                outflow[min(t - start, OBS_BINS - 1)] += np.uint64(len(gone))    # by the ending episode's clock
        eng.step(T)
        R.assert_engine_equals(eng, mir, "with both observers on")
        want = _want(obs, [0] * E, 1, OBS_BINS, m.size)
        got = eng.field_stats()
        for key in KEYS:
            assert np.array_equal(got[key].reshape(want[key].shape), want[key]), key
        pocket = (np.isinf(np.asarray(mir.cores[0].sff32)) & (m == 0)).reshape(-1)
        inside = int(want["occupancy"][0][pocket].sum())
        assert inside >= U.FLOORS["pocket"], "the pocket's agents were observed inside"
        flow = eng.exit_flow()
        assert int(flow["exited"].sum()) == exited > 0
        assert np.array_equal(flow["outflow"].reshape(-1), outflow)
        # agents inside at the end + agents that left = agents ever placed: nobody frozen is counted out
        placed = N * (E + int(mir.eps.sum()))
        assert int(mir.cnt.sum()) + exited == placed
    finally:
        eng.close()
