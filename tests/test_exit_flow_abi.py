"""CPU-side checks of the exit flow's C ABI and of the evacuation driver's texts (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffm_engine_set_exit_flow", "ffm_engine_get_exit_flow", "ffm_engine_get_exit_doors")


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
    assert hasattr(so, "ffm_debug_exit_flow_info")
    # the header names what the feature restates, the limit of its tables and the order of the setters
    assert "model/ffm_core.py:66-72, 100-102" in txt
    assert re.search(r"#define\s+FFM_EXIT_FLOW_MAX_BYTES\s+FFM_FIELD_STATS_MAX_BYTES\b", txt)
    assert "Rooms first, the flow after" in txt


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID
    cls = np.zeros(4, np.int32)
    out = np.zeros(16, np.uint64)
    doors = np.zeros(16, np.int32)
    p = out.ctypes.data_as(C.c_void_p)
    nd = C.c_int32()
    assert lib.ffm_engine_set_exit_flow(None, None, 0, cls.ctypes.data_as(C.c_void_p), 1, 0, None) == E_INVALID
    assert lib.ffm_last_error()
    assert lib.ffm_engine_set_exit_flow(None, doors.ctypes.data_as(C.c_void_p), 1, None, 0, 0, None) == E_INVALID
    assert lib.ffm_engine_get_exit_flow(None, p, p, 0, None) == E_INVALID
    assert lib.ffm_engine_get_exit_flow(None, None, None, 1, None) == E_INVALID
    assert lib.ffm_engine_get_exit_doors(None, doors.ctypes.data_as(C.c_void_p), C.byref(nd)) == E_INVALID
    assert lib.ffm_engine_get_exit_doors(None, None, None) == E_INVALID


def test_abi_version_unchanged(lib):
    assert lib.ffm_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", txt)


def test_flow_kernel_is_built_from_its_own_source():
    from ffm_amd import build as B
    assert "core_flow.hip" in B.SOURCES
    assert os.path.exists(os.path.join(B.CSRC, "core_flow.hip"))


def test_driver_texts_are_pure_functions_of_the_arrays():
    from ffm_amd.evac import doors_csv, exit_usage_csv, outflow_csv
    exited = np.array([[7, 0], [2 ** 40 + 1, 3]], np.uint64)
    assert exit_usage_csv(exited) == "set,door,exited\n0,0,7\n0,1,0\n1,0,1099511627777\n1,1,3\n"
    assert exit_usage_csv(np.zeros((0, 0), np.uint64)) == "set,door,exited\n"
    assert exit_usage_csv(np.zeros((2, 0), np.uint64)) == "set,door,exited\n"
    with pytest.raises(ValueError):
        exit_usage_csv(np.zeros(3, np.uint64))

    doc = np.full((2, 3, 4), -1, np.int32)
    doc[0, 0, 2] = 0
    doc[1, 0, 1] = 1
    doc[1, 0, 2] = 0
    doc[1, 2, 3] = 2
    assert doors_csv(doc) == "room,door,row,col\n0,0,0,2\n1,1,0,1\n1,0,0,2\n1,2,2,3\n"
    assert doors_csv(np.full((1, 3, 3), -1, np.int32)) == "room,door,row,col\n"
    assert doors_csv(np.zeros((0, 3, 3), np.int32)) == "room,door,row,col\n"

    out = np.zeros((2, 2, 3), np.uint64)
    out[0, 1, 1] = 9
    out[1, 0, 2] = 2 ** 35
    assert outflow_csv(out) == ("set,door,tau,exited\n"
                                "0,0,0,0\n0,0,1,0\n0,0,2,0\n0,1,0,0\n0,1,1,9\n0,1,2,0\n"
                                "1,0,0,0\n1,0,1,0\n1,0,2,34359738368\n1,1,0,0\n1,1,1,0\n1,1,2,0\n")
    assert outflow_csv(np.zeros((2, 1, 0), np.uint64)) == "set,door,tau,exited\n"
    with pytest.raises(ValueError):
        outflow_csv(np.zeros((2, 3), np.uint64))


def test_flow_parsing():
    from ffm_amd.evac import build_parser
    ap = build_parser()
    base = ["--room", "12", "12", "--out", "x"]
    a = ap.parse_args(base)
    assert a.flow is False and a.fields is False and a.curve_bins == 0
    a = ap.parse_args(base + ["--flow"])
    assert a.flow is True and a.fields is False and a.curve_bins == 0
    a = ap.parse_args(base + ["--flow", "--curve-bins", "128"])
    assert a.flow is True and a.curve_bins == 128
    a = ap.parse_args(base + ["--flow", "--fields", "--curve-bins", "8"])
    assert a.flow is True and a.fields is True and a.curve_bins == 8


@pytest.mark.parametrize("extra", [["--curve-bins", "16"], ["--flow", "--curve-bins", "-1"]])
def test_curve_bins_wants_fields_or_flow_and_a_count(extra, capsys):
    """Refused by the argument check, before anything touches a device."""
    from ffm_amd.evac import main
    with pytest.raises(SystemExit) as ex:
        main(["--room", "12", "12", "--out", "x"] + extra)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--curve-bins" in err and "--flow" in err
