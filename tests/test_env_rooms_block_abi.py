"""CPU-side checks of the block kernel's room form: the ABI symbol of its opt-in switch,
data.geodesic_sff (the obstacle-aware static floor field) and the evac driver's new pure pieces
(--sff parsing, the kernel choice from a launch_info dict).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffm_engine_set_env_rooms_kernel"


@pytest.fixture(scope="module")
def lib():
    from ffm_amd import build as B
    B.build()
    from ffm_amd.engine import load_library
    return load_library()


def test_symbol_resolves_and_is_declared(lib):
    from ffm_amd.engine import EXPORTED
    header = open(os.path.join(ROOT, "include", "ffm_amd.h")).read()
    so = ctypes.CDLL(os.path.join(ROOT, "ffm_amd", "_lib", "libffm_amd.so"))
    assert hasattr(so, NAME)
    assert re.search(r"^int " + NAME + r"\(ffm_engine\* eng, int32_t mode\);", header, re.M)
    assert NAME in EXPORTED
    assert re.search(r"^#define FFM_ABI_VERSION 2$", header, re.M)      # an added symbol: the version stays


def test_null_engine_is_invalid(lib):
    from ffm_amd.engine import E_INVALID
    for mode in (0, 1, 2):
        assert lib.ffm_engine_set_env_rooms_kernel(None, mode) == E_INVALID


# ---------------------------------------------------------------------------
# geodesic_sff
# ---------------------------------------------------------------------------
def _r2():
    from ffm_amd.data import make_room
    m = make_room(12, 12, exit_pos=(6, 0))
    m[1:3, 9:11] = 2
    m[9:11, 9:11] = 2
    return m


def _r3():
    from ffm_amd.data import make_room
    m = make_room(12, 12)
    m[11, 3] = 3
    m[1:3, 1:3] = 2
    return m


def _barrier20():
    from ffm_amd.data import make_room
    m = make_room(20, 20)
    m[4, 5:16] = 2
    return m


def _plain_rooms():
    from ffm_amd.data import make_room
    return {
        "12x12": make_room(12, 12),
        "12x12 side exit": make_room(12, 12, exit_pos=(6, 0)),
        "14x14": make_room(14, 14),
        "16x16 w2": make_room(16, 16, exit_pos=(0, 4), exit_width=2),
        "20x20 w4": make_room(20, 20, exit_pos=(0, 8), exit_width=4),
        "50x50": make_room(50, 50),
        "64x64": make_room(64, 64),
        "R2": _r2(),
        "R3": _r3(),
    }


@pytest.mark.parametrize("name", sorted(_plain_rooms()))
def test_geodesic_equals_l1_where_nothing_is_in_the_way(name):
    from ffm_amd.data import geodesic_sff, l1_sff
    m = _plain_rooms()[name]
    g, l = geodesic_sff(m), l1_sff(m)
    assert g.dtype == np.float32 and g.shape == m.shape
    assert np.array_equal(g.view(np.uint32), l.view(np.uint32))


def _no_lower_neighbour(m, f):
    """Free cells without a strictly lower passable Neumann neighbour: where agents get stuck."""
    H, W = m.shape
    out = []
    for x, y in np.argwhere(m == 0):
        nb = [(x + dx, y + dy) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1))]
        if not any(0 <= u < H and 0 <= v < W and m[u, v] in (0, 3) and f[u, v] < f[x, y] for u, v in nb):
            out.append((int(x), int(y)))
    return out


def test_geodesic_goes_round_the_barrier():
    from ffm_amd.data import geodesic_sff, l1_sff
    m = _barrier20()
    g, l = geodesic_sff(m), l1_sff(m)
    assert np.isfinite(g[m == 0]).all() and np.isinf(g[m == 2]).all() and (g[m == 3] == 0).all()
    assert int((g.view(np.uint32) != l.view(np.uint32)).sum()) == 154
    assert _no_lower_neighbour(m, g) == []
    assert len(_no_lower_neighbour(m, l)) == 1                           # the trap under the L1 field
    assert g.dtype == np.float32 and geodesic_sff(m, dtype=np.float64).dtype == np.float64


def test_unreachable_pocket():
    from ffm_amd.data import geodesic_sff, make_room
    m = make_room(12, 12)
    m[4:8, 4:8] = 2
    m[5:7, 5:7] = 0                                                      # a walled-off 2x2 pocket
    with pytest.raises(ValueError, match="cannot reach an exit"):
        geodesic_sff(m)
    g = geodesic_sff(m, unreachable="inf")
    assert np.isinf(g[5:7, 5:7]).all() and int(np.isinf(g[m == 0]).sum()) == 4
    with pytest.raises(ValueError):
        geodesic_sff(m, unreachable="zero")
    with pytest.raises(ValueError):
        geodesic_sff(m, neighborhood="hex")


def test_moore_is_chebyshev_on_a_plain_room():
    from ffm_amd.data import geodesic_sff, make_room
    m = make_room(16, 16)
    g = geodesic_sff(m, neighborhood="moore")
    ex, ey = np.argwhere(m == 3)[0]
    xs, ys = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    cheb = np.maximum(np.abs(xs - ex), np.abs(ys - ey)).astype(np.float32)
    passable = (m == 0) | (m == 3)
    assert np.array_equal(g[passable], cheb[passable]) and np.isinf(g[~passable]).all()


# ---------------------------------------------------------------------------
# the evac driver's pure pieces
# ---------------------------------------------------------------------------
def test_parse_sff():
    from ffm_amd.evac import parse_sff
    assert parse_sff(None, True) == ("l1", None)
    assert parse_sff("l1", True) == ("l1", None)
    assert parse_sff("geodesic", True) == ("geodesic", None)
    assert parse_sff(None, False) == (None, None)
    assert parse_sff("sff.npy", False) == (None, "sff.npy")
    with pytest.raises(ValueError):
        parse_sff("sff.npy", True)                                       # --room takes a kind, not a file
    with pytest.raises(ValueError):
        parse_sff("geodesic", False)                                     # --map takes a file


def test_parser_takes_sff_kinds_and_files():
    from ffm_amd.evac import build_parser
    ap = build_parser()
    assert ap.parse_args(["--room", "20", "20", "--sff", "geodesic", "--out", "o"]).sff == "geodesic"
    assert ap.parse_args(["--room", "20", "20", "--out", "o"]).sff is None
    assert ap.parse_args(["--map", "m.npy", "--sff", "s.npy", "--out", "o"]).sff == "s.npy"


def test_room_sff_kinds():
    from ffm_amd.data import geodesic_sff, l1_sff
    from ffm_amd.evac import room_sff
    m = _barrier20()
    assert np.array_equal(room_sff("l1", m, "neumann").view(np.uint32), l1_sff(m).view(np.uint32))
    assert np.array_equal(room_sff("geodesic", m, "moore").view(np.uint32),
                          geodesic_sff(m, neighborhood="moore").view(np.uint32))


def test_room_sweep_kernel_choice():
    from ffm_amd.evac import room_sweep_kernel
    assert room_sweep_kernel({"kernel": "wave"}) == "block"
    assert room_sweep_kernel({"kernel": "block"}) == "block"
    for k in ("lane", "group", "block_scratch"):                         # the plain call: its form, or its refusal
        assert room_sweep_kernel({"kernel": k}) is None
