"""CPU-side checks of the group kernel's room form: mode 2 of ffm_engine_set_env_rooms_kernel in the
header, the Python table of room kernels, the setter's argument check and the evac driver's
--room-kernel option.  No GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ffm_amd import build as B
    B.build()
    from ffm_amd.engine import load_library
    return load_library()


def test_header_documents_mode_2():
    header = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    doc = header[header.index("/* The kernel that steps the engine while rooms are on"):
                 header.index("int ffm_engine_set_env_rooms_kernel(")]
    assert re.search(r"mode 2 = group", doc)
    assert "Mode 2 is accepted on" in doc and "FFM_WAVE_BLOCKS" in doc
    assert re.search(r"^int ffm_engine_set_env_rooms_kernel\(ffm_engine\* eng, int32_t mode\);", header, re.M)
    assert re.search(r"^#define FFM_ABI_VERSION 2$", header, re.M)      # a new mode value: signature and version stay


def test_python_room_kernels():
    from ffm_amd.engine import Engine
    assert Engine._ENV_ROOMS_KERNELS["group"] == 2
    assert Engine._ENV_ROOMS_KERNELS["lane"] == 0 and Engine._ENV_ROOMS_KERNELS["block"] == 1
    assert "group" in Engine.set_env_rooms.__doc__ and "group" in Engine.launch_info.__doc__


def test_null_engine_and_unknown_mode_are_invalid(lib):
    from ffm_amd.engine import E_INVALID
    for mode in (3, -1, 2):
        assert lib.ffm_engine_set_env_rooms_kernel(None, mode) == E_INVALID


def test_evac_parser_room_kernel():
    from ffm_amd.evac import build_parser
    ap = build_parser()
    base = ["--room", "12", "12", "--out", "o"]
    assert ap.parse_args(base).room_kernel is None
    for k in ("lane", "group", "block"):
        assert ap.parse_args(base + ["--room-kernel", k]).room_kernel == k
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--room-kernel", "wave"])
