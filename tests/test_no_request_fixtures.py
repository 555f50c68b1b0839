"""The no-request branch (model/ffm_core.py:82) is taken where the tests say it is.  No GPU.

A fixture or a GPU case that never reaches the branch pins nothing.  no_request_util.count_branches
restates lines :52-82 in NumPy and counts, from a state alone, the agents that fail :82, apart from
those that fail :63 (boxed in).  Here it runs over the oracle's replay of every new golden fixture
and over the oracle mirror of every case of tests/test_gpu_no_request.py, against the floors of
no_request_util.FLOORS:

  pocket     >= 1,000 no-request agent-steps per fixture and per GPU case;
  overflow   >= 1,000 per GPU case.  An injected fixture is one env of 60 agents for 6 steps, 360
             agent-steps in all, and only the agents beside the one hot cell (4 or 8), or the one on
             it, can fail :82, while it stays above f32 max / 8 (five steps): at most 20 (Neumann) or
             40 (Moore) per ring fixture, 5 per fixture with an agent on the cell, and by
             construction the whole ring, or the agent on the cell, in the first step.  The fixtures
             must lie between the two; the floor of 1,000 is the GPU cases', which have E to grow;
  diag       >= 50 agent-steps with a non-finite score among the candidates, and not one of them fails
             :82: a -inf beside a finite score has probability exactly 0 and leaves the sum finite.
"""
import numpy as np
import pytest

import no_request_util as U
from golden_util import load_case, load_inject
from oracle import oracle as O

POCKET = ("pocket_neumann_12x12_N40", "pocket_moore_12x12_N40", "pocket_neumann_f64_12x12_N40",
          "pocket_moore_kS0_12x12_N40")
DIAG = ("diag_moore_12x12_N60", "diag_moore_f64_12x12_N60")
# fixture: the least and the most no-request agent-steps its construction allows (see above)
OVERFLOW = {"overflow_neumann_ring60_kS3_kD8": (4, 20), "overflow_moore_ring60_kS3_kD8": (8, 40),
            "overflow_neumann_on60_kS3_kD8": (1, 5), "overflow_moore_on60_kS3_kD8": (1, 5)}


def _replay(name):
    c = load_case(name)
    assert c.max_steps <= 60 and c.map.shape == (12, 12)
    core = O.Core(c.map, c.sff, c.params)
    return c, U.count_replay_mt(core, c.N, [ep.seed for ep in c.episodes], c.max_steps)


def test_count_branches_on_hand_made_states():
    """Four agents in the pocket room, by hand: one in the pocket beside a free cell (:82), one boxed
    in by it and the walls (:63)... and two in the open, of which one stands below the exit."""
    m, s = U.pocket_room("neumann")
    W = 12
    pos = np.full((1, 8), 0xFFFF, np.uint16)
    # (1, 1) has the neighbours (2, 1) [agent] and (1, 2) [agent]: boxed in.  (2, 1): (2, 2) is free: :82.
    # (1, 2): (1, 3) and (2, 2) free: :82.  (1, 6) below the exit: exit forcing.  (6, 6): ordinary.
    cells = [1 * W + 1, 2 * W + 1, 1 * W + 2, 1 * W + 6, 6 * W + 6]
    pos[0, :5] = cells
    dff = np.zeros((1, 12, 12), np.float32)
    for k_S in (3, 0):
        nr, bx, nf = U.count_branches(m, s, U.params("neumann", k_S), pos, np.array([5]), dff)
        assert (int(nr[0]), int(bx[0]), int(nf[0])) == (2, 1, 2)
    # the diagonal cell: the agent on (5, 5) and the one beside it at (4, 4) see a -inf score, and request
    m, s = U.diag_room()
    pos[0, :2] = [5 * W + 5, 4 * W + 4]
    nr, bx, nf = U.count_branches(m, s, U.params("moore"), pos, np.array([2]), dff)
    assert (int(nr[0]), int(bx[0]), int(nf[0])) == (0, 0, 1)      # (4, 4) sees (5, 5) occupied: no candidate
    pos[0, :1] = [4 * W + 4]
    nr, bx, nf = U.count_branches(m, s, U.params("moore"), pos, np.array([1]), dff)
    assert (int(nr[0]), int(bx[0]), int(nf[0])) == (0, 0, 1)
    # one hot DFF cell with k_D = 8: its four neighbours fail :82, the agent two cells away does not
    from ffm_amd.data import l1_sff, make_room
    m = make_room(12, 12)
    pos[0, :5] = [5 * W + 6, 7 * W + 6, 6 * W + 5, 6 * W + 7, 8 * W + 6]
    nr, bx, nf = U.count_branches(m, l1_sff(m), U.params("neumann", 3, 8), pos, np.array([5]), U.huge_dff(m)[None])
    assert (int(nr[0]), int(bx[0]), int(nf[0])) == (4, 0, 4)


@pytest.mark.parametrize("name", POCKET)
def test_pocket_fixtures_meet_the_floor(name):
    c, (nr, bx, nf) = _replay(name)
    assert nr >= U.FLOORS["pocket"], (nr, bx)
    assert nf == nr          # every non-finite score there fails :82
    assert bx > 0            # and :63 is taken beside it: the two are told apart
    # the first seed's DFF is stored in full
    assert len(c.episodes[0].full) == len(c.episodes[0].counts)


@pytest.mark.parametrize("name", DIAG)
def test_diag_fixtures_never_take_the_branch(name):
    c, (nr, bx, nf) = _replay(name)
    assert c.params["neighborhood"] == "moore"
    assert nf >= U.FLOORS["diag"] and nr == 0, (nr, nf)
    assert len(c.episodes[0].full) == len(c.episodes[0].counts)


@pytest.mark.parametrize("name", sorted(OVERFLOW))
def test_overflow_fixtures_take_the_branch(name):
    c = load_inject(name)
    assert c.params["k_D"] == 8 and (c.dff0 == U.DFF_HUGE).sum() == 1 and c.dff0[U.HUGE_CELL] == U.DFF_HUGE
    core = O.Core(c.map, c.sff, c.params)
    nr, bx, nf = U.count_replay_mt(core, len(c.pos0), [c.seed], len(c.counts), pos0=c.pos0, dff0=c.dff0)
    print(name, nr, bx, nf)
    assert nr == nf and OVERFLOW[name][0] <= nr <= OVERFLOW[name][1], (nr, nf)


def _gpu_cases():
    pytest.importorskip("torch")
    import test_gpu_no_request as G
    return G


def test_gpu_tables_cover_the_forms():
    G = _gpu_cases()
    import test_gpu_rare_philox as P
    twelve = {f for f in P.FORMS if not f[-1].isdigit() or f in P.BASE_FORMS}      # the forms that take a 12x12 room
    assert twelve == set(G.POCKET_FORMS) and len(twelve) == 12
    assert {(f, n) for f, n, k, _, _ in G.POCKET_CASES if k == 3} == {(f, n) for f in twelve for n in ("neumann", "moore")}
    assert any(k == 0 for _, _, k, _, _ in G.POCKET_CASES)
    Es = {c[3] for c in G.POCKET_CASES}
    assert min(Es) >= 64 and max(Es) <= 513 and any(e % 2 for e in Es)
    assert all(8 <= c[4] <= 40 for c in G.POCKET_CASES)
    assert {f for f, _ in G.OVERFLOW_CASES} == set(P.BASE_FORMS)


def test_gpu_pocket_cases_meet_the_floor():
    G = _gpu_cases()
    for case in G.POCKET_CASES + [G.OBS_CASE]:
        nr, bx, _ = G.branch_counts("pocket", *case)
        assert nr >= U.FLOORS["pocket"], (case, nr)
    assert G.branch_counts("pocket_f64", *G.F64_CASE)[0] >= U.FLOORS["pocket"]


def test_gpu_overflow_cases_meet_the_floor():
    G = _gpu_cases()
    for case in G.OVERFLOW_CASES:
        nr, _, nf = G.branch_counts("overflow", *case)
        assert nr >= U.FLOORS["overflow"], (case, nr)


def test_gpu_diag_cases_never_take_the_branch():
    G = _gpu_cases()
    for case in G.DIAG_CASES:
        nr, _, nf = G.branch_counts("diag", *case)
        assert nr == 0 and nf >= U.FLOORS["diag"], (case, nr, nf)
