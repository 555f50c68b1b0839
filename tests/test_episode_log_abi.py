"""CPU-side checks of the episode log's C ABI and of the evacuation driver's CSV (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffm_engine_set_episode_log", "ffm_engine_drain_episodes", "ffm_engine_get_episode_stats")


@pytest.fixture(scope="module")
def lib():
    from ffm_amd import build as B
    B.build()
    from ffm_amd.engine import load_library
    return load_library()


def test_symbols_resolve_and_are_declared(lib):
    so = C.CDLL(os.path.join(ROOT, "ffm_amd", "_lib", "libffm_amd.so"))
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    from ffm_amd.engine import EXPORTED
    for n in SYMBOLS:
        assert hasattr(so, n), n
        assert re.search(r"^int\s+" + n + r"\s*\(", txt, re.M), n
        assert n in EXPORTED
    # the header names what the log restates
    assert "main.py:44-56" in txt and "model/ffm_core.py:119-133" in txt


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID
    n, dropped = C.c_int64(5), C.c_int64(5)
    buf = np.zeros((4, 4), np.int32)
    s = np.zeros(5, np.uint64)
    assert lib.ffm_engine_set_episode_log(None, 16, 8, None) == E_INVALID
    assert lib.ffm_last_error()
    assert lib.ffm_engine_drain_episodes(None, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n), C.byref(dropped),
                                         None) == E_INVALID
    assert lib.ffm_engine_get_episode_stats(None, None, 0, s.ctypes.data_as(C.c_void_p), 0, None) == E_INVALID


def test_abi_version_unchanged(lib):
    assert lib.ffm_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", txt)


def test_evac_csv_is_a_pure_function_of_the_records():
    from ffm_amd.evac import records_from_steps, steps_csv, summary_text
    rec = np.array([[1, 1, 40, 75], [0, 0, 97, 97], [1, 0, 35, 35], [0, 1, 23, 120]], np.int32)   # any order
    assert steps_csv(rec, episodes=2, N=12) == ("episode_num,env,N,steps\n"
                                                "1,0,12,97\n"
                                                "2,0,12,23\n"
                                                "3,1,12,35\n"
                                                "4,1,12,40\n")
    assert steps_csv(np.zeros((0, 4), np.int32), episodes=1, N=5) == "episode_num,env,N,steps\n"
    steps = np.array([[97, 23], [35, 40]], np.int32)
    assert steps_csv(records_from_steps(steps), 2, 12) == steps_csv(rec, 2, 12)
    assert np.array_equal(records_from_steps(steps, env_base=7)[:, 0], [7, 7, 8, 8])
    assert summary_text(steps, 1000, 2.0) == ("count 4\nmean 48.750000\nstd 28.533971\nmin 23\nmax 97\n"
                                              "steps_per_second 500.0\n")
