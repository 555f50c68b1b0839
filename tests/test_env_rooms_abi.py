"""CPU-side checks of per-env rooms: the two ABI symbols, make_room's exit width, and the pure
functions the evac driver builds a room sweep from (the product with a room axis, the env
assignment, both CSV texts with the room column).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ffm_engine_set_env_rooms", "ffm_engine_get_env_rooms")


@pytest.fixture(scope="module")
def lib():
    from ffm_amd import build as B
    B.build()
    from ffm_amd.engine import load_library
    return load_library()


def test_symbols_resolve_and_are_declared(lib):
    from ffm_amd.engine import EXPORTED
    header = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    so = ctypes.CDLL(os.path.join(ROOT, "ffm_amd", "_lib", "libffm_amd.so"))
    for n in NAMES:
        assert hasattr(so, n), n
        assert re.search(r"^int " + n + r"\(ffm_engine\*", header, re.M), n
        assert n in EXPORTED


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID
    m = np.zeros(144, np.uint8)
    s = np.zeros(144, np.float32)
    roe = np.zeros(1, np.int32)
    n = ctypes.c_int32(7)
    P = ctypes.c_void_p
    assert lib.ffm_engine_set_env_rooms(None, m.ctypes.data_as(P), s.ctypes.data_as(P), 1, roe.ctypes.data_as(P),
                                        None) == E_INVALID
    assert lib.ffm_engine_set_env_rooms(None, None, None, 0, None, None) == E_INVALID
    assert lib.ffm_engine_get_env_rooms(None, None, None, 0, ctypes.byref(n), None) == E_INVALID
    assert b"null" in lib.ffm_last_error()


def test_abi_version_is_still_2(lib):
    from ffm_amd.engine import ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert lib.ffm_abi_version() == ABI_VERSION == 2
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", header)


# ---- make_room's exit width ---------------------------------------------------------------------
def test_make_room_default_width_is_todays_room():
    from ffm_amd.data import make_room
    assert np.array_equal(make_room(12, 12, exit_width=1), make_room(12, 12))
    assert np.array_equal(make_room(12, 12, exit_pos=(6, 0), exit_width=1), make_room(12, 12, exit_pos=(6, 0)))
    assert np.array_equal(make_room(5, 8, exit_pos=(4, 3), exit_width=1), make_room(5, 8, exit_pos=(4, 3)))


def test_make_room_two_wide_and_side_wall():
    from ffm_amd.data import make_room
    assert make_room(4, 6, exit_pos=(0, 2), exit_width=2).tolist() == [
        [2, 2, 3, 3, 2, 2],
        [2, 0, 0, 0, 0, 2],
        [2, 0, 0, 0, 0, 2],
        [2, 2, 2, 2, 2, 2]]
    assert make_room(6, 4, exit_pos=(1, 3), exit_width=3).tolist() == [
        [2, 2, 2, 2],
        [2, 0, 0, 3],
        [2, 0, 0, 3],
        [2, 0, 0, 3],
        [2, 0, 0, 2],
        [2, 2, 2, 2]]
    assert make_room(4, 6, exit_width=2).tolist()[0] == [2, 2, 2, 3, 3, 2]      # from the default position (0, 3)


def test_make_room_refuses_a_corner():
    from ffm_amd.data import make_room
    for kw in (dict(exit_pos=(0, 4), exit_width=2),      # would reach (0, 5)
               dict(exit_pos=(0, 0), exit_width=2),      # starts in a corner
               dict(exit_pos=(3, 0), exit_width=3),      # the side wall, down to (5, 0)
               dict(exit_pos=(2, 2), exit_width=2),      # not on a wall
               dict(exit_width=0)):
        with pytest.raises(ValueError):
            make_room(6, 6, **kw)


# ---- the evac driver's pure functions, on a hand-written example --------------------------------
BASE = {"k_S": 3.0, "k_D": 1.0, "diffuse": 0.2, "decay": 0.2, "N": 32}


def test_parse_sweep_exit_width():
    from ffm_amd.evac import parse_sweep
    assert parse_sweep("exit_width=1,2,4") == ("exit_width", [1, 2, 4])
    assert parse_sweep("N=5,20") == ("N", [5, 20])


def test_product_with_a_room_axis_varies_the_room_slowest():
    from ffm_amd.evac import sweep_grid
    g = sweep_grid([("N", [5, 20]), ("k_D", [0.0, 4.0])], BASE, 3, [1, 2, 4])
    assert [(s["room"], s["exit_width"], s["N"], s["k_D"]) for s in g] == [
        (0, 1, 5, 0.0), (0, 1, 5, 4.0), (0, 1, 20, 0.0), (0, 1, 20, 4.0),
        (1, 2, 5, 0.0), (1, 2, 5, 4.0), (1, 2, 20, 0.0), (1, 2, 20, 4.0),
        (2, 4, 5, 0.0), (2, 4, 5, 4.0), (2, 4, 20, 0.0), (2, 4, 20, 4.0)]
    # rooms from files: no exit_width; a room sweep alone: one set per room with the base parameters
    g = sweep_grid([], BASE, 2)
    assert g == [{**BASE, "room": 0}, {**BASE, "room": 1}]
    # no room axis: the sets of before
    assert sweep_grid([("N", [5])], BASE) == [{**BASE, "N": 5}]
    with pytest.raises(ValueError):
        sweep_grid([], BASE, 2, [1, 2, 4])


def test_env_assignment_with_rooms_is_e_mod_p():
    from ffm_amd.evac import env_assignment, sweep_grid
    g = sweep_grid([("N", [5, 20])], BASE, 2, [1, 2])            # (r0,5) (r0,20) (r1,5) (r1,20)
    soe = env_assignment(6, len(g))
    assert soe.tolist() == [0, 1, 2, 3, 0, 1]
    assert [g[p]["room"] for p in soe] == [0, 0, 1, 1, 0, 0]
    assert (soe % 2).tolist() == [0, 1, 0, 1, 0, 1]             # the parameter set of each env


def test_steps_csv_has_the_room_columns():
    from ffm_amd.evac import env_assignment, steps_csv, sweep_grid
    g = sweep_grid([("N", [5, 20])], BASE, 2, [1, 2])
    soe = env_assignment(6, 4)
    rec = np.array([[5, 0, 4, 0], [2, 1, 3, 0], [2, 0, 11, 0], [0, 0, 9, 0], [3, 0, 6, 0]])
    assert steps_csv(rec, 2, 32, g, soe) == (
        "episode_num,env,N,steps,k_S,k_D,diffuse,decay,room,exit_width\n"
        "1,0,5,9,3,1,0.2,0.2,0,1\n"
        "5,2,5,11,3,1,0.2,0.2,1,2\n"
        "6,2,5,3,3,1,0.2,0.2,1,2\n"
        "7,3,20,6,3,1,0.2,0.2,1,2\n"
        "11,5,20,4,3,1,0.2,0.2,0,1\n")
    g = sweep_grid([], BASE, 2)                                  # --rooms: the room column alone
    assert steps_csv(rec[:2], 2, 32, g, env_assignment(6, 2)) == (
        "episode_num,env,N,steps,k_S,k_D,diffuse,decay,room\n"
        "6,2,32,3,3,1,0.2,0.2,0\n"
        "11,5,32,4,3,1,0.2,0.2,1\n")


def test_sweep_summary_has_the_room_columns():
    from ffm_amd.evac import env_assignment, sweep_grid, sweep_summary_csv
    g = sweep_grid([("N", [5, 20])], BASE, 2, [1, 2])
    soe = env_assignment(6, 4)
    steps = np.array([[9, 11], [7, 7], [11, 13], [20, 30], [1, 3], [4, 3]])   # envs 0, 4: set 0; 1, 5: set 1
    assert sweep_summary_csv(steps, g, soe) == (
        "set,k_S,k_D,diffuse,decay,N,room,exit_width,count,mean,std,min,max\n"
        "0,3,1,0.2,0.2,5,0,1,4,6.000000,4.123106,1,11\n"
        "1,3,1,0.2,0.2,20,0,1,4,5.250000,1.785357,3,7\n"
        "2,3,1,0.2,0.2,5,1,2,2,12.000000,1.000000,11,13\n"
        "3,3,1,0.2,0.2,20,1,2,2,25.000000,5.000000,20,30\n")
