"""CPU-side checks of the per-env group path's public surface: the ABI entry
ffm_engine_set_env_params_kernel and the evac driver's --sweep-kernel switch (no GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffm_engine_set_env_params_kernel"


@pytest.fixture(scope="module")
def lib():
    from ffm_amd import build as B
    B.build()
    from ffm_amd.engine import load_library
    return load_library()


def test_symbol_is_exported_declared_and_bound(lib):
    so = ctypes.CDLL(os.path.join(ROOT, "ffm_amd", "_lib", "libffm_amd.so"))
    assert hasattr(so, NAME)
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert re.search(r"^int\s+" + NAME + r"\s*\(\s*ffm_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt, re.M)
    from ffm_amd.engine import EXPORTED
    assert NAME in EXPORTED
    assert getattr(lib, NAME).restype is ctypes.c_int


@pytest.mark.parametrize("mode", [0, 1, 2, -1])
def test_null_engine_is_invalid(lib, mode):
    from ffm_amd.engine import E_INVALID
    assert getattr(lib, NAME)(None, mode) == E_INVALID
    assert lib.ffm_last_error()


def test_abi_version_is_still_2(lib):
    from ffm_amd.engine import ABI_VERSION
    assert lib.ffm_abi_version() == ABI_VERSION == 2
    txt = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    assert re.search(r"#define\s+FFM_ABI_VERSION\s+2\b", txt)


def test_binding_rejects_a_bad_kernel_name_before_the_library():
    """Engine.set_env_params(kernel=...) validates the name first: no engine handle is touched."""
    from ffm_amd.engine import Engine
    eng = Engine.__new__(Engine)          # no device, no handle: the check must come first
    with pytest.raises(ValueError):
        Engine.set_env_params(eng, [{}], kernel="wave")


def test_evac_parser_sweep_kernel():
    from ffm_amd import evac
    ap = evac.build_parser()
    base = ["--room", "12", "12", "--out", "x"]
    assert ap.parse_args(base).sweep_kernel is None
    for k in ("lane", "group"):
        assert ap.parse_args(base + ["--sweep-kernel", k]).sweep_kernel == k
    for bad in ("wave", "block", "", "Group"):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--sweep-kernel", bad])
    assert evac.SWEEP_KERNEL_DEFAULT in ("lane", "group")
