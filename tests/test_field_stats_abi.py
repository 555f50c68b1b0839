"""CPU-side checks of the field statistics' C ABI and of the evacuation driver's texts (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffm_engine_set_field_stats", "ffm_engine_get_field_stats")


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
    # the header names what the feature restates, and the limit of its tables
    assert "main.py:44-54" in txt
    assert re.search(r"#define\s+FFM_FIELD_STATS_MAX_BYTES\b", txt)


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID
    cls = np.zeros(4, np.int32)
    out = np.zeros(16, np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.ffm_engine_set_field_stats(None, cls.ctypes.data_as(C.c_void_p), 1, 0, None) == E_INVALID
    assert lib.ffm_last_error()
    assert lib.ffm_engine_set_field_stats(None, None, 0, 0, None) == E_INVALID
    assert lib.ffm_engine_get_field_stats(None, p, p, p, p, 0, None) == E_INVALID
    assert lib.ffm_engine_get_field_stats(None, None, None, None, None, 1, None) == E_INVALID


def test_abi_version_unchanged(lib):
    assert lib.ffm_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", txt)


def test_observer_is_built_from_its_own_source():
    from ffm_amd import build as B
    assert "core_observe.hip" in B.SOURCES
    assert os.path.exists(os.path.join(B.CSRC, "core_observe.hip"))


def test_driver_texts_are_pure_functions_of_the_arrays():
    from ffm_amd.evac import observed_csv, occupancy_csv, remaining_csv
    observed = np.array([7, 0, 2 ** 40 + 1], np.uint64)
    assert observed_csv(observed) == "set,observed\n0,7\n1,0\n2,1099511627777\n"
    assert observed_csv(np.zeros(0, np.uint64)) == "set,observed\n"

    occ = np.zeros((2, 3, 4), np.uint64)
    occ[0, 1, 2] = 5
    occ[0, 1, 1] = 2 ** 33
    occ[1, 2, 0] = 1
    assert occupancy_csv(occ) == "set,row,col,occupancy\n0,1,1,8589934592\n0,1,2,5\n1,2,0,1\n"
    assert occupancy_csv(np.zeros((1, 3, 3), np.uint64)) == "set,row,col,occupancy\n"

    remaining = np.array([[0, 9, 4], [0, 3, 2 ** 35]], np.uint64)
    alive = np.array([[0, 3, 2], [0, 1, 1]], np.uint64)
    assert remaining_csv(remaining, alive) == ("set,tau,remaining,alive\n"
                                               "0,0,0,0\n0,1,9,3\n0,2,4,2\n"
                                               "1,0,0,0\n1,1,3,1\n1,2,34359738368,1\n")
    assert remaining_csv(np.zeros((2, 0), np.uint64), np.zeros((2, 0), np.uint64)) == "set,tau,remaining,alive\n"
    with pytest.raises(ValueError):
        remaining_csv(remaining, alive[:, :2])


def test_fields_parsing():
    from ffm_amd.evac import build_parser
    ap = build_parser()
    base = ["--room", "12", "12", "--out", "x"]
    a = ap.parse_args(base)
    assert a.fields is False and a.curve_bins == 0
    a = ap.parse_args(base + ["--fields"])
    assert a.fields is True and a.curve_bins == 0
    a = ap.parse_args(base + ["--fields", "--curve-bins", "128"])
    assert a.fields is True and a.curve_bins == 128


@pytest.mark.parametrize("extra", [["--curve-bins", "16"], ["--fields", "--curve-bins", "-1"]])
def test_curve_bins_wants_fields_and_a_count(extra, capsys):
    """Refused by the argument check, before anything touches a device."""
    from ffm_amd.evac import main
    with pytest.raises(SystemExit) as ex:
        main(["--room", "12", "12", "--out", "x"] + extra)
    assert ex.value.code == 2
    assert "--curve-bins" in capsys.readouterr().err
