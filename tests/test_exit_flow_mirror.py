"""The exit flow's oracle mirror alone (no GPU): every case tests/test_gpu_exit_flow.py runs is not
vacuous on the oracle, the sequential walk's own assertions hold in every env-step, and the
NumPy door tables are what the rule says."""
import numpy as np
import pytest

import exit_flow_mirror as X
from env_sweep_util import SETS5
from exit_flow_mirror import BINS, ENGINES, M32, PAR


def test_door_tables():
    m = X.three(12, 12)
    doors = X.default_doors(m)
    assert doors[0, 6] == 0 and doors[5, 0] == 1 and doors[11, 3] == 2 and (doors >= 0).sum() == 3
    for nbh, near in (("neumann", {(1, 6): 0, (5, 1): 1, (10, 3): 2}),
                      ("moore", {(1, 5): 0, (1, 6): 0, (1, 7): 0, (4, 1): 1, (5, 1): 1, (6, 1): 1,
                                 (10, 2): 2, (10, 3): 2, (10, 4): 2})):
        df = X.door_from(m, doors, nbh)
        got = {(int(x), int(y)): int(df[x, y]) for x, y in np.argwhere(df >= 0)}
        assert got == near, nbh
    # a 4-wide exit: a cell next to two exit cells takes the first in neighbour order
    w4 = X.room("X4")[0]
    d4 = X.default_doors(w4)
    assert [int(d4[0, y]) for y in range(4, 8)] == [0, 1, 2, 3]
    assert [int(v) for v in X.door_from(w4, d4, "neumann")[1, 3:9]] == [-1, 0, 1, 2, 3, -1]
    assert [int(v) for v in X.door_from(w4, d4, "moore")[1, 3:9]] == [0, 0, 0, 1, 2, 3]


def test_walk_finds_the_leavers():
    m = X.three(12, 12)
    df = X.door_from(m, X.default_doors(m), "neumann").reshape(-1)
    P = np.array([18, 30, 61, 100])             # (1, 6) and (5, 1) have doors
    assert X.leavers(P, np.array([18, 31, 61, 101]), df, 12, "neumann", False) == []
    assert X.leavers(P, np.array([31, 61, 101]), df, 12, "neumann", False) == [0]
    assert X.leavers(P, np.array([18, 31, 101]), df, 12, "neumann", False) == [2]
    assert X.leavers(P[[0, 2]], np.array([], np.int64), df, 12, "neumann", True) == [0, 1]
    with pytest.raises(AssertionError):          # an agent without a door cannot vanish
        X.leavers(P, np.array([18, 61, 101]), df, 12, "neumann", False)


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_every_engine_case(name, nbh):
    (w,), eps, doors = X.plain(name, nbh)
    assert doors.shape[0] == 1 and w["exited"].shape == (3, 3)
    X.assert_not_vacuous(w, eps)
    assert w["exited"].sum() == w["outflow"].sum() == w["events"]
    assert not w["outflow"][:, :, 0].any()       # tau >= 1 always


@pytest.mark.parametrize("name", ["group", "block"])
def test_no_auto_reset_case(name):
    rm, A, N, E, T = ENGINES[name][:5]
    (first, last), eps, _ = X.plain(name, "moore", (("step", T), ("mark",), ("step", 10)), auto=False)
    assert int(first["exited"].sum()) == E * N and last["events"] == 0
    if name == "group":
        assert E * N == 1184


def test_door_label_case():
    E, T = 37, 300
    args = (("X4",), (0,) * E, 32, "moore", (PAR + (32,),), (0,) * E, (("step", T),), X.cls3(E), 3)
    (w4,), eps, doors = X.flow(*args)
    (w1,), _, doors1 = X.flow(*args, labels=((0,) * 144,))
    assert w4["exited"].shape == (3, 4) and w1["exited"].shape == (3, 1)
    assert (w4["exited"] > 0).all() and (eps >= 2).all()
    assert np.array_equal(w4["exited"].sum(axis=1, keepdims=True), w1["exited"])
    assert np.array_equal(w4["outflow"].sum(axis=1, keepdims=True), w1["outflow"])
    assert (doors1[doors >= 0] == 0).all() and (doors1[doors < 0] == -1).all()


@pytest.mark.parametrize("rooms,A,N", [(("X1", "X2", "X3", "X4"), 32, 32), (("Y1", "Y2", "Y3", "Y4"), 16, 10)])
def test_env_rooms_case(rooms, A, N):
    E, T = 36, 300
    roe = tuple(e % 4 for e in range(E))
    (w,), eps, doors = X.flow(rooms, roe, A, "moore", (PAR + (N,),), (0,) * E, (("step", T),), roe, 4)
    assert doors.shape[0] == 4 and w["exited"].shape == (4, 4)
    for r in range(4):                            # class r is room r: doors it does not have stay zero
        assert (w["exited"][r, :r + 1] > 0).all() and not w["exited"][r, r + 1:].any()
    assert (eps >= 2).all()


def test_env_rooms_with_params_case():
    E, T = 40, 400
    roe = tuple(e % 4 for e in range(E))
    soe = tuple(e % 5 for e in range(E))
    (w,), eps, _ = X.flow(("X1", "X2", "X3", "X4"), roe, 32, "moore", SETS5, soe, (("step", T),), roe, 4)
    for r in range(4):
        assert (w["exited"][r, :r + 1] > 0).all() and not w["exited"][r, r + 1:].any()
    assert (eps >= 2).all()


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_snapshot_refresh_cases(nbh):
    E = 37
    every = (1,) * E
    third = tuple(int(e % 3 == 0) for e in range(E))
    for mask in (every, third):
        ops = (("step", 30), ("reset_envs", mask), ("mark",), ("step", 1), ("mark",), ("step", 29))
        (_, w1, _), _, _ = X.plain("group", nbh, ops)
        # agents placed next to a door leave in the step right after the reset, with tau = 1
        assert w1["tau1"] > 0, "mirror: no event with tau = 1 right after the reset"
        if mask is every:
            assert w1["tau1"] == w1["events"]
    ops = (("step", 30), ("set_state", X.ring_state(E, 32)), ("mark",), ("step", 30))
    (_, w), _, _ = X.plain("group", nbh, ops)
    assert w["events"] > 0 and w["exited"][:, 0].all()


def test_mid_run_case():
    ops = (("step", 20), ("on",), ("mark",), ("step", 100), ("mark",), ("step", 60), ("mark",), ("step", 20),
           ("on",), ("mark",), ("step", 60))
    ws, eps, _ = X.plain("group", "moore", ops)
    assert all(ws[k]["events"] > 0 for k in (1, 2, 4))


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_wrap_case(nbh):
    t0 = (1 << 32) - 20
    (w,), _, _ = X.plain("group", nbh, (("step", 60),), t0=t0, E=7)
    assert w["before_wrap"] > 0 and w["after_wrap"] > 0
    assert t0 + 1 + 60 > M32


@pytest.mark.parametrize("nbh", ["neumann", "moore"])
def test_many_agents_case(nbh):
    E = 3
    (w,), _, _ = X.flow(("R64",), (0,) * E, 512, nbh, (PAR + (512,),), (0,) * E, (("step", 120),), X.cls3(E), 3,
                        False)
    assert w["idx64"] > 0, "mirror: no leaver with an agent index >= 64"
    assert w["exited"].shape == (3, 1) and w["events"] > 0 and BINS == 16
