"""The motion statistics' oracle mirror alone (no GPU): every case tests/test_gpu_motion_stats.py
runs is not vacuous on the oracle, the sequential walks' own assertions hold in every env-step, the
identities between the tables hold, and the NumPy direction table is what the rule says."""
import numpy as np
import pytest

import exit_flow_mirror as X
import motion_mirror as M
from env_sweep_util import SETS5
from motion_mirror import BINS, ENGINES, M32, PAR

# dir_from of three(12, 12), written by hand: exits at (0, 6), (5, 0) and (11, 3); '.' is none.
# Neumann codes: 0 up, 1 down, 2 left, 3 right.  Moore codes: row-major, 0 .. 7.
HAND = {
    "neumann": ("............",
                "......0.....",
                "............",
                "............",
                "............",
                ".2..........",
                "............",
                "............",
                "............",
                "............",
                "...1........",
                "............"),
    "moore": ("............",
              ".....210....",
              "............",
              "............",
              ".5..........",
              ".3..........",
              ".0..........",
              "............",
              "............",
              "............",
              "..765.......",
              "............"),
}


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_direction_table(nbh):
    want = np.array([[-1 if ch == "." else int(ch) for ch in row] for row in HAND[nbh]], np.int32)
    m = X.three(12, 12)
    got = M.dir_from(m, nbh)
    assert np.array_equal(got, want)
    # a door exactly where a direction is, and the direction points at an exit cell
    assert np.array_equal(got >= 0, X.door_from(m, X.default_doors(m), nbh) >= 0)
    for x, y in np.argwhere(got >= 0):
        dx, dy = M.NEIGHBOURS[nbh][got[x, y]]
        assert m[x + dx, y + dy] == 3


def test_directions_of_the_engine_are_the_mirrors():
    from ffm_amd.engine import motion_directions
    assert tuple(motion_directions(4)) == M.NEIGHBOURS["neumann"] + ((0, 0),)
    assert tuple(motion_directions(8)) == M.NEIGHBOURS["moore"] + ((0, 0),)


def test_walk_finds_the_successors():
    assert M.successors(4, [], 4) == [0, 1, 2, 3]
    assert M.successors(4, [0, 2], 2) == [None, 0, None, 1]
    assert M.successors(3, [0, 1, 2], 0) == [None, None, None]
    with pytest.raises(AssertionError):
        M.successors(4, [1], 4)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_every_engine_case(name, nbh):
    (w,), eps, _ = M.plain(name, nbh)
    NB = len(M.NEIGHBOURS[nbh])
    H = 12 if ENGINES[name][0] == "T12" else 14
    assert w["flux"].shape == (3, H, H, NB + 1) and w["present"].shape == (3, BINS)
    M.assert_not_vacuous(w, eps, ENGINES[name][0])
    M.assert_identities(w)
    assert int(w["egress_count"].sum()) == w["events"] == int(w["exited"].sum())
    assert np.array_equal(w["egress_count"].sum(axis=(1, 2)), w["exited"].sum(axis=1))
    # the flow's tables of the same pass are the flow mirror's own
    (x,), _, _ = X.plain(name, nbh)
    assert np.array_equal(w["exited"], x["exited"]) and np.array_equal(w["outflow"], x["outflow"])


@pytest.mark.parametrize("name", ["group", "block"])
def test_no_auto_reset_case(name):
    rm, A, N, E, T = ENGINES[name][:5]
    (first, last), _, _ = M.plain(name, "moore", (("step", T), ("mark",), ("step", 10)), auto=False)
    assert int(first["egress_count"].sum()) == E * N and last["events"] == 0
    assert not last["flux"].any() and not last["present"].any()
    M.assert_identities(first)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_snapshot_and_origin_cases(nbh):
    E = 37
    every = (1,) * E
    third = tuple(int(e % 3 == 0) for e in range(E))
    for mask in (every, third):
        ops = (("step", 30), ("reset_envs", mask), ("mark",), ("step", 1), ("mark",), ("step", 29))
        (_, w1, w2), _, _ = M.plain("group", nbh, ops)
        assert w1["tau1"] > 0, "mirror: no event with tau = 1 right after the reset"
        assert w2["events"] > 0 and w2["shifted"] > 0
        M.assert_identities(w1)
    # two reset_envs in a row: leavers of envs whose first step after the placement has tau = 2
    other = tuple(int(e % 3 == 1) for e in range(E))
    ops = (("step", 30), ("reset_envs", third), ("reset_envs", other), ("mark",), ("step", 1), ("mark",), ("step", 29))
    (_, w1, _), _, _ = M.plain("group", nbh, ops)
    assert w1["late_first"] > 0 and w1["tau1"] > 0, "mirror: no leaver in a first step with tau != 1"
    ops = (("step", 30), ("mark",), ("set_state", X.ring_state(E, 32)), ("step", 30))
    (w0, w), _, _ = M.plain("group", nbh, ops)
    assert w0["events"] > 0 and w["events"] > 0 and w["flux"].any()


def test_mid_run_cases():
    for on in (("on",), ("on", "keep")):
        ops = (("step", 20), on, ("mark",), ("step", 100), ("mark",), ("step", 60), ("mark",), ("step", 20),
               on, ("mark",), ("step", 60))
        ws, _, _ = M.plain("group", "moore", ops)
        assert all(ws[k]["events"] > 0 and ws[k]["shifted"] > 0 for k in (1, 2, 4))
    # the two differ: with ep_start kept, the agents in flight carry their episode's tau
    a, _, _ = M.plain("group", "moore", (("step", 20), ("on",), ("mark",), ("step", 100)))
    b, _, _ = M.plain("group", "moore", (("step", 20), ("on", "keep"), ("mark",), ("step", 100)))
    assert np.array_equal(a[1]["flux"], b[1]["flux"]) and not np.array_equal(a[1]["present"], b[1]["present"])
    assert not np.array_equal(a[1]["egress_steps"], b[1]["egress_steps"])


@pytest.mark.parametrize("rooms,A,N", [(("X1", "X2", "X3", "X4"), 32, 32), (("Y1", "Y2", "Y3", "Y4"), 16, 10)])
def test_env_rooms_cases(rooms, A, N):
    E, T = 36, 300
    roe = tuple(e % 4 for e in range(E))
    (w,), eps, _ = M.motion(rooms, roe, A, "moore", (PAR + (N,),), (0,) * E, (("step", T),), roe, 4)
    assert (eps >= 2).all() and w["shifted"] > 0
    M.assert_identities(w)
    # class r is room r: a wider exit gives leavers more cells, and more directions, to leave from
    leaving = [set(map(tuple, np.argwhere(M.dir_from(M.room(r)[0], "moore") >= 0))) for r in rooms]
    assert all(len(leaving[r]) < len(leaving[r + 1]) for r in range(3))


def test_env_rooms_with_params_case():
    E, T = 40, 400
    roe = tuple(e % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    (wa, wb), eps, _ = M.motion(("X1", "X2", "X3", "X4"), roe, 32, "moore", SETS5, soe,
                                (("step", 250), ("mark",), ("step", T - 250)), roe, 4)
    assert (eps >= 2).all() and wa["events"] > 0 and wb["events"] > 0
    M.assert_identities(wa)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_wrap_case(nbh):
    t0 = (1 << 32) - 20
    (w,), _, _ = M.plain("group", nbh, (("step", 60),), t0=t0, E=7)
    assert w["before_wrap"] > 0 and w["after_wrap"] > 0
    assert t0 + 1 + 60 > M32
    M.assert_identities(w)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_many_agents_case(nbh):
    E = 3
    (w,), _, _ = M.motion(("R64",), (0,) * E, 512, nbh, (PAR + (512,),), (0,) * E, (("step", 120),), X.cls3(E), 3,
                          False)
    assert w["chunk_shift"] > 0, "mirror: no survivor at an index >= 64 with a leaver in an earlier chunk"
    assert w["events"] > 0 and w["flux"].shape[1:3] == (64, 64)
    M.assert_identities(w)
