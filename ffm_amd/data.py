"""Synthetic rooms and static floor fields.

Restates the recipe of the reference's ``create_12x12_map_and_sff.py:15-50``
(SoraKurihara/FFM) for any size: a one-cell wall border (value 2), one exit
(value 3) at ``(0, W // 2)``, free cells 0, and an L1 distance-to-exit static
floor field stored as float32 with ``inf`` on every non-passable cell.
``tests/test_data.py`` checks the 12x12 case against the files the reference's
own script writes (committed under ``tests/golden/``).  ``geodesic_sff`` is the field for rooms
with obstacles: the step count to the nearest exit along passable cells.
"""
from __future__ import annotations

import numpy as np

FREE, AGENT, WALL, EXIT = 0, 1, 2, 3


def make_room(H: int = 12, W: int = 12, exit_pos: tuple[int, int] | None = None,
              exit_width: int = 1) -> np.ndarray:
    """Map per ``create_12x12_map_and_sff.py:15-25`` scaled to H x W (uint8).

    ``exit_width`` adjacent exit cells lie along the wall that holds ``exit_pos``: they start at
    ``exit_pos`` and extend in +y on the top or bottom wall, in +x on a side wall.  A wider exit
    that is not on a wall, or that would reach a corner, raises ValueError."""
    if H < 3 or W < 3:
        raise ValueError("room needs at least 3x3 cells")
    if exit_width < 1:
        raise ValueError("exit_width must be >= 1")
    m = np.zeros((H, W), dtype=np.uint8)
    m[0, :] = WALL
    m[-1, :] = WALL
    m[:, 0] = WALL
    m[:, -1] = WALL
    ex, ey = exit_pos if exit_pos is not None else (0, W // 2)
    if exit_width == 1:
        m[ex, ey] = EXIT
        return m
    ex, ey = ex % H, ey % W
    if ex in (0, H - 1):      # top or bottom wall: along y
        if ey < 1 or ey + exit_width > W - 1:
            raise ValueError(f"a {exit_width}-wide exit at {(ex, ey)} would reach a corner of the {H}x{W} room")
        m[ex, ey:ey + exit_width] = EXIT
    elif ey in (0, W - 1):    # side wall: along x
        if ex + exit_width > H - 1:
            raise ValueError(f"a {exit_width}-wide exit at {(ex, ey)} would reach a corner of the {H}x{W} room")
        m[ex:ex + exit_width, ey] = EXIT
    else:
        raise ValueError(f"a {exit_width}-wide exit must start on a wall, not at {(ex, ey)}")
    return m


def l1_sff(map_array: np.ndarray, dtype=np.float32) -> np.ndarray:
    """L1 distance to the nearest exit per ``create_12x12_map_and_sff.py:36-50``."""
    m = np.asarray(map_array)
    exits = np.argwhere(m == EXIT)
    H, W = m.shape
    xs, ys = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.full((H, W), np.inf, dtype=np.float64)
    for ex, ey in exits:
        d = np.minimum(d, np.abs(xs - ex) + np.abs(ys - ey))
    passable = (m == FREE) | (m == EXIT)
    out = np.where(passable, d, np.inf).astype(dtype)
    return out


_MOVES = {"neumann": ((-1, 0), (1, 0), (0, -1), (0, 1)),
          "moore": ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def geodesic_sff(map_array: np.ndarray, neighborhood: str = "neumann", dtype=np.float32,
                 unreachable: str = "raise") -> np.ndarray:
    """Steps to the nearest exit along passable cells: the static floor field of a room with
    obstacles, where ``l1_sff`` can lead agents into a pocket that has no lower neighbour.

    A multi-source breadth-first search from the exit cells over the passable cells (free and
    exit), with the moves of ``neighborhood`` as the engine makes them (Moore: all eight, no
    corner rule).  Non-passable cells hold ``inf``, as in ``l1_sff``; on a room without obstacles
    the Neumann field equals ``l1_sff`` bit for bit.  A free cell that cannot reach an exit
    raises ValueError, or with ``unreachable="inf"`` holds ``inf``."""
    if neighborhood not in _MOVES:
        raise ValueError(f"neighborhood must be 'neumann' or 'moore', got {neighborhood!r}")
    if unreachable not in ("raise", "inf"):
        raise ValueError(f"unreachable must be 'raise' or 'inf', got {unreachable!r}")
    m = np.asarray(map_array)
    if m.ndim != 2:
        raise ValueError("map must be two-dimensional")
    H, W = m.shape
    passable = (m == FREE) | (m == EXIT)
    d = np.full((H, W), np.inf, dtype=np.float64)
    frontier = [(int(x), int(y)) for x, y in np.argwhere(m == EXIT)]
    for x, y in frontier:
        d[x, y] = 0.0
    step = 0
    while frontier:
        step += 1
        nxt = []
        for x, y in frontier:
            for dx, dy in _MOVES[neighborhood]:
                u, v = x + dx, y + dy
                if 0 <= u < H and 0 <= v < W and passable[u, v] and d[u, v] == np.inf:
                    d[u, v] = step
                    nxt.append((u, v))
        frontier = nxt
    lost = np.argwhere((m == FREE) & np.isinf(d))
    if len(lost) and unreachable == "raise":
        x, y = lost[0]
        raise ValueError(f"{len(lost)} free cell(s) cannot reach an exit (the first at {(int(x), int(y))}); "
                         "unreachable='inf' keeps them at inf")
    return d.astype(dtype)


def free_cells(map_array: np.ndarray) -> np.ndarray:
    """Row-major free-cell list, the order of ``np.argwhere(map == 0)``."""
    return np.flatnonzero(np.asarray(map_array).reshape(-1) == FREE)
