"""CPU-side checks of the motion statistics' C ABI and of the evacuation driver's texts (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ffm_engine_set_motion_stats", "ffm_engine_get_motion_stats")


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
    assert hasattr(so, "ffm_debug_motion_stats_info")
    assert "ffm_debug_motion_stats_info" not in txt           # a diagnostic, outside the header
    # the header names what the feature relies on, the limit of its tables and the order of the setters
    assert "model/ffm_core.py:100-102" in txt
    assert re.search(r"#define\s+FFM_MOTION_STATS_MAX_BYTES\s+FFM_FIELD_STATS_MAX_BYTES\b", txt)
    assert "Rooms first, the motion statistics after" in txt


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID
    cls = np.zeros(4, np.int32)
    out = np.zeros(16, np.uint64)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.ffm_engine_set_motion_stats(None, cls.ctypes.data_as(C.c_void_p), 1, 0, None) == E_INVALID
    assert lib.ffm_last_error()
    assert lib.ffm_engine_set_motion_stats(None, None, 0, 0, None) == E_INVALID
    assert lib.ffm_engine_get_motion_stats(None, p, p, p, p, p, 0, None) == E_INVALID
    assert lib.ffm_engine_get_motion_stats(None, None, None, None, None, None, 1, None) == E_INVALID
    info = np.zeros(7, np.int32)
    fn = lib.ffm_debug_motion_stats_info
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int], C.c_int
    assert fn(None, info.ctypes.data_as(C.c_void_p), 7) == E_INVALID


def test_abi_version_unchanged(lib):
    assert lib.ffm_abi_version() == 2
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", txt)


def test_motion_kernel_is_built_from_its_own_source():
    from ffm_amd import build as B
    assert "core_motion.hip" in B.SOURCES
    src = open(os.path.join(B.CSRC, "core_motion.hip")).read()
    assert "core_motion_kernel" in src and "FFM_MOTION_MUTATE" in src


def test_directions():
    from ffm_amd.engine import motion_directions
    assert motion_directions(4) == [(-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)]
    assert motion_directions(8) == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1), (0, 0)]


def test_driver_texts_are_pure_functions_of_the_arrays():
    from ffm_amd.evac import egress_by_origin_csv, flux_csv, speed_csv
    flux = np.zeros((2, 2, 3, 5), np.uint64)
    flux[0, 1, 2, 4] = 7
    flux[0, 1, 2, 0] = 1
    flux[1, 0, 1, 3] = 2 ** 40 + 1
    assert flux_csv(flux) == "set,row,col,direction,count\n0,1,2,0,1\n0,1,2,4,7\n1,0,1,3,1099511627777\n"
    assert flux_csv(np.zeros((0, 3, 3, 9), np.uint64)) == "set,row,col,direction,count\n"
    assert flux_csv(np.zeros((2, 3, 3, 9), np.uint64)) == "set,row,col,direction,count\n"
    with pytest.raises(ValueError):
        flux_csv(np.zeros((2, 3, 3), np.uint64))

    present = np.array([[0, 9, 4], [0, 2 ** 35, 0]], np.uint64)
    moved = np.array([[0, 3, 4], [0, 1, 0]], np.uint64)
    assert speed_csv(present, moved) == ("set,tau,present,moved\n0,0,0,0\n0,1,9,3\n0,2,4,4\n"
                                         "1,0,0,0\n1,1,34359738368,1\n1,2,0,0\n")
    assert speed_csv(np.zeros((2, 0), np.uint64), np.zeros((2, 0), np.uint64)) == "set,tau,present,moved\n"
    with pytest.raises(ValueError):
        speed_csv(present, moved[:, :2])
    with pytest.raises(ValueError):
        speed_csv(present[0], moved[0])

    count = np.zeros((2, 3, 4), np.uint64)
    steps = np.zeros((2, 3, 4), np.uint64)
    count[0, 1, 1], steps[0, 1, 1] = 2, 31
    count[1, 2, 3], steps[1, 2, 3] = 1, 2 ** 33
    assert egress_by_origin_csv(count, steps) == "set,row,col,count,steps_sum\n0,1,1,2,31\n1,2,3,1,8589934592\n"
    assert egress_by_origin_csv(count * 0, steps * 0) == "set,row,col,count,steps_sum\n"
    with pytest.raises(ValueError):
        egress_by_origin_csv(count, steps[:1])


def test_motion_parsing():
    from ffm_amd.evac import build_parser
    ap = build_parser()
    base = ["--room", "12", "12", "--out", "x"]
    a = ap.parse_args(base)
    assert a.motion is False and a.flow is False and a.fields is False and a.curve_bins == 0
    a = ap.parse_args(base + ["--motion"])
    assert a.motion is True and a.flow is False and a.fields is False and a.curve_bins == 0
    a = ap.parse_args(base + ["--motion", "--curve-bins", "128"])
    assert a.motion is True and a.curve_bins == 128
    a = ap.parse_args(base + ["--motion", "--flow", "--fields", "--curve-bins", "8"])
    assert a.motion is True and a.flow is True and a.fields is True and a.curve_bins == 8


@pytest.mark.parametrize("extra", [["--curve-bins", "16"], ["--motion", "--curve-bins", "-1"]])
def test_curve_bins_wants_a_feature_and_a_count(extra, capsys):
    """Refused by the argument check, before anything touches a device."""
    from ffm_amd.evac import main
    with pytest.raises(SystemExit) as ex:
        main(["--room", "12", "12", "--out", "x"] + extra)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--curve-bins" in err and "--motion" in err
