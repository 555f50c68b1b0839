"""CPU-side checks of per-env parameters: the two ABI symbols, and the pure functions the evac
driver builds a sweep from (set grid, env assignment, both CSV texts).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ffm_engine_set_env_params", "ffm_engine_get_env_params")


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
    assert re.search(r"double k_S, k_D, diffuse, decay;\s*int32_t n_agents;\s*int32_t reserved;\s*} ffm_env_params;", header)


def test_env_params_struct_matches_header_layout():
    from ffm_amd.engine import EnvParams
    assert ctypes.sizeof(EnvParams) == 40
    assert [f[0] for f in EnvParams._fields_] == ["k_S", "k_D", "diffuse", "decay", "n_agents", "reserved"]
    assert EnvParams.n_agents.offset == 32


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID, EnvParams
    one = (EnvParams * 1)()
    soe = np.zeros(1, np.int32)
    n = ctypes.c_int32(7)
    assert lib.ffm_engine_set_env_params(None, one, 1, soe.ctypes.data_as(ctypes.c_void_p), None) == E_INVALID
    assert lib.ffm_engine_set_env_params(None, None, 0, None, None) == E_INVALID
    assert lib.ffm_engine_get_env_params(None, one, 1, ctypes.byref(n), None) == E_INVALID
    assert b"null" in lib.ffm_last_error()


def test_abi_version_is_still_2(lib):
    from ffm_amd.engine import ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert lib.ffm_abi_version() == ABI_VERSION == 2
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", header)


# ---- the evac driver's pure functions, on a hand-written example --------------------------------
BASE = {"k_S": 3.0, "k_D": 1.0, "diffuse": 0.2, "decay": 0.2, "N": 32}


def test_parse_sweep():
    from ffm_amd.evac import parse_sweep
    assert parse_sweep("N=5,10,32") == ("N", [5, 10, 32])
    assert parse_sweep("k_D=0,1.5,4") == ("k_D", [0.0, 1.5, 4.0])
    for bad in ("k_A=1,2", "N", "N=", "=3"):
        with pytest.raises(ValueError):
            parse_sweep(bad)


def test_sweep_grid_is_the_product_in_argument_order():
    from ffm_amd.evac import sweep_grid
    g = sweep_grid([("N", [5, 10]), ("k_D", [0.0, 1.5, 4.0])], BASE)
    assert [(s["N"], s["k_D"]) for s in g] == [(5, 0.0), (5, 1.5), (5, 4.0), (10, 0.0), (10, 1.5), (10, 4.0)]
    assert all(s["k_S"] == 3.0 and s["diffuse"] == 0.2 and s["decay"] == 0.2 for s in g)
    g = sweep_grid([("k_D", [0.0, 4.0]), ("N", [5, 10])], BASE)
    assert [(s["N"], s["k_D"]) for s in g] == [(5, 0.0), (10, 0.0), (5, 4.0), (10, 4.0)]
    with pytest.raises(ValueError):
        sweep_grid([("N", [1]), ("N", [2])], BASE)


def test_env_assignment_is_e_mod_p():
    from ffm_amd.evac import env_assignment
    a = env_assignment(8, 3)
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 2, 0, 1, 2, 0, 1]
    with pytest.raises(ValueError):
        env_assignment(2, 3)


def test_steps_csv_with_sets_carries_each_envs_n_and_parameters():
    from ffm_amd.evac import env_assignment, steps_csv, sweep_grid
    g = sweep_grid([("N", [5, 10]), ("k_D", [0.0, 1.5])], BASE)       # (5,0) (5,1.5) (10,0) (10,1.5)
    soe = env_assignment(6, 4)
    rec = np.array([[5, 1, 3, 0], [1, 0, 7, 0], [0, 0, 9, 0], [2, 0, 11, 0], [5, 0, 4, 0]])
    assert steps_csv(rec, 2, 32, g, soe) == (
        "episode_num,env,N,steps,k_S,k_D,diffuse,decay\n"
        "1,0,5,9,3,0,0.2,0.2\n"
        "3,1,5,7,3,1.5,0.2,0.2\n"
        "5,2,10,11,3,0,0.2,0.2\n"
        "11,5,5,4,3,1.5,0.2,0.2\n"
        "12,5,5,3,3,1.5,0.2,0.2\n")
    # records carry global env ids
    assert steps_csv(rec + np.array([100, 0, 0, 0]), 2, 32, g, soe, env_base=100).splitlines()[3] == \
        "205,102,10,11,3,0,0.2,0.2"


def test_steps_csv_old_call_gives_its_old_text():
    from ffm_amd.evac import steps_csv
    rec = np.array([[1, 0, 7, 0], [0, 0, 9, 0], [7, 1, 3, 0]])
    assert steps_csv(rec, 2, 32) == "episode_num,env,N,steps\n1,0,32,9\n3,1,32,7\n16,7,32,3\n"


def test_sweep_summary_rows():
    from ffm_amd.evac import env_assignment, sweep_grid, sweep_summary_csv
    g = sweep_grid([("N", [5, 10]), ("k_D", [0.0, 1.5])], BASE)
    soe = env_assignment(6, 4)
    steps = np.array([[9, 11], [7, 7], [11, 13], [20, 30], [1, 3], [4, 3]])   # envs 0, 4: set 0; 1, 5: set 1
    assert sweep_summary_csv(steps, g, soe) == (
        "set,k_S,k_D,diffuse,decay,N,count,mean,std,min,max\n"
        "0,3,0,0.2,0.2,5,4,6.000000,4.123106,1,11\n"
        "1,3,1.5,0.2,0.2,5,4,5.250000,1.785357,3,7\n"
        "2,3,0,0.2,0.2,10,2,12.000000,1.000000,11,13\n"
        "3,3,1.5,0.2,0.2,10,2,25.000000,5.000000,20,30\n")
