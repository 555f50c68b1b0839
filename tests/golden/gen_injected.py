#!/usr/bin/env python3
"""Generate the injected-state golden vectors by running the reference itself (container only).

    python tests/golden/gen_injected.py [--ref /root/reference]

Like gen_golden.py it imports ``model.ffm_core.FloorFieldModel`` from the reference
(SoraKurihara/FFM), but instead of stepping from the model's own placement it overwrites
``positions`` and ``dff`` with a state the dynamics do not produce by themselves (the families
of tests/test_gpu_geometry.py: packed blobs, rings of requesters around one cell, a large
DFF; and one DFF cell at 3e38 with k_D = 8, whose product overflows float32, so that the agents
around it fail model/ffm_core.py:82 and make no request), seeds both global generators, and records 6 steps.  Only the recorded arrays (inputs and
outputs) are written, as small ``inject_*.npz`` fixtures next to this script.

Fixture layout (one file per case):
  map [H,W] u8, sff [H,W] (f32 or f64), params json, seed
  pos0    [n] int16           injected agent cells (x*W+y), in agent order
  dff0    [H,W] float32       injected DFF
  counts  [T] int16           agents alive after each step
  cells   [sum(counts)] int16 agent cells after each step, in order
  dff     [T,H,W] float32     DFF after each step
  np_tail / py_tail [4] uint32  next raw 32-bit words of both RNG streams
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
STEPS = 6


def run_case(name, FloorFieldModel, map_array, sff, params, cells0, dff0, seed):
    H, W = map_array.shape
    with tempfile.TemporaryDirectory() as td:
        sff_path = os.path.join(td, "sff.npy")
        np.save(sff_path, sff)
        np.random.seed(seed)
        model = FloorFieldModel(map_array, sff_path, len(cells0), dict(params))
    c = np.asarray(cells0, dtype=np.int64)
    model.positions = np.stack([c // W, c % W], axis=1)
    model.dff = np.array(dff0, dtype=np.float32)
    np.random.seed(seed)
    random.seed(seed)
    counts, cells, dffs = [], [], []
    for _ in range(STEPS):
        model.step()
        p = model.positions
        counts.append(p.shape[0])
        cells.extend((p[:, 0] * W + p[:, 1]).astype(np.int16).tolist())
        assert model.dff.dtype == np.float32
        dffs.append(np.array(model.dff))
    np_tail = np.asarray(np.random.mtrand._rand._bit_generator.random_raw(4), dtype=np.uint32)
    py_tail = np.asarray([random.getrandbits(32) for _ in range(4)], dtype=np.uint32)
    path = os.path.join(HERE, f"inject_{name}.npz")
    np.savez_compressed(
        path, map=map_array.astype(np.uint8), sff=sff, params=json.dumps(params), seed=np.int64(seed),
        pos0=c.astype(np.int16), dff0=np.asarray(dff0, np.float32), counts=np.asarray(counts, np.int16),
        cells=np.asarray(cells, np.int16), dff=np.stack(dffs).astype(np.float32), np_tail=np_tail, py_tail=py_tail)
    print(f"{name}: n={len(c)} counts={counts} -> {os.path.getsize(path)} B")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default="", help="a prefix: (re)generate the cases whose names start with it")
    args = ap.parse_args()
    global run_case
    _run = run_case

    def run_case(name, *a, **kw):        # noqa: F811 -- filter by --only
        if name.startswith(args.only):
            _run(name, *a, **kw)

    sys.path.insert(0, args.ref)
    from model.ffm_core import FloorFieldModel  # the reference itself
    sys.path.insert(0, os.path.dirname(TESTS))
    sys.path.insert(0, TESTS)
    from ffm_amd.data import l1_sff
    from test_gpu_geometry import DFF_SCALES, ROOMS, injected_state, make_named_room

    kS, kD = (0, 3, 10), (0, 1, 2.5, 8)
    dd = ((0.2, 0.2), (0.01, 0.01), (0.5, 0.9))
    # per room and neighbourhood: (family, n)
    shapes = (("blob", 32), ("ring", 19), ("blob", 60), ("ring", 7))
    i = 0
    for room in ROOMS:
        for nbh in ("neumann", "moore"):
            m = make_named_room(room)
            for fam, n in shapes:
                rng = np.random.default_rng(1000 + i)
                # rings want their centre: k_S = 10; the other points cycle through every value
                p = {"k_S": 10 if fam == "ring" else kS[i % 3], "k_D": kD[(i // 2 + i) % 4],
                     "diffuse": dd[i % 3][0], "decay": dd[i % 3][1], "neighborhood": nbh}
                scale = DFF_SCALES[(i + i // 4) % 4]
                # every sixth case takes main.py's float64 SFF path
                sff = l1_sff(m, np.float64 if i % 6 == 5 else np.float32)
                cells, dff = injected_state(rng, m, n, 4 if nbh == "neumann" else 8, fam, scale)
                run_case(f"{room}_{nbh}_{fam}{n}_kS{p['k_S']}_kD{p['k_D']}_s{scale}", FloorFieldModel, m, sff, p,
                         cells, dff, 500 + i)
                i += 1
    # a full room: only the agents next to the exit have a valid neighbour
    m = make_named_room("plain")
    rng = np.random.default_rng(77)
    cells, dff = injected_state(rng, m, int((m == 0).sum()), 8, "blob", 20)
    run_case("plain_moore_full_kS3_kD2.5_s20", FloorFieldModel, m, l1_sff(m),
             {"k_S": 3, "k_D": 2.5, "diffuse": 0.2, "decay": 0.2, "neighborhood": "moore"}, cells, dff, 601)
    # a non-square room for the runtime-dimension kernels
    m = make_named_room("interior", 20, 24)
    rng = np.random.default_rng(78)
    cells, dff = injected_state(rng, m, 40, 4, "ring", 200)
    run_case("interior20x24_neumann_ring40_kS10_kD1_s200", FloorFieldModel, m, l1_sff(m),
             {"k_S": 10, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}, cells, dff, 602)
    # k_D * DFF overflows float32 around one cell: the agents beside it (or on it) make no request
    import no_request_util as U
    m = make_named_room("plain")
    i = 0
    for nbh in ("neumann", "moore"):
        for on_cell in (False, True):
            cells, dff = U.overflow_state(m, 4 if nbh == "neumann" else 8, on_cell, 900 + i)
            run_case(f"overflow_{nbh}_{'on' if on_cell else 'ring'}60_kS3_kD8", FloorFieldModel, m, l1_sff(m),
                     {"k_S": 3, "k_D": 8, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}, cells, dff, 700 + i)
            i += 1


if __name__ == "__main__":
    main()
