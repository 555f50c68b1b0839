#!/usr/bin/env python3
"""Find the Philox counters that land in the branches no random run takes, and write them to
tests/golden/rare_philox.json (settings only; tests/test_rare_philox_fixtures.py pins every
entry with the scalar Philox, tests/test_gpu_rare_philox.py puts engines there).

  friction  the owner's word w of a contested target is rejected (low32(w m) < 2^32 mod m) and the
            first word of the owner's friction stream picks another rank;
  tie       two equal placement keys at adjacent ranks r, r + 1 <= 31 among F free cells;
  short     fewer than N of F placement keys under the candidate threshold (the retry).

The search loops are the oracle library's (oracle/ffm_oracle.c, ffo_find_*), over global envs
[64, 72) and t ascending from 0 in fixed chunks; the first hit in (t, env) order that fits is
taken, so the result does not depend on the thread count.

    python tools/find_rare_philox.py            # search and write the file (a few minutes)
    python tools/find_rare_philox.py --check    # search again and compare with the file
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "rare_philox.json")

SEED = 0x9E3779B97F4A7C15            # both halves nonzero
ENVS = (64, 72)                      # a test puts the env at any local slot through env_base
T_END = 1 << 32
# (m, owner index): m = 2, 4, 8 never reject (2^32 mod m = 0)
FRICTION = ((3, 0), (3, 29), (5, 27), (6, 0), (6, 26), (7, 0), (7, 25))
RMAX = 31                            # N = r + 1 and r + 2 fit a capacity of 32
# (name, F, what the pair of j must satisfy): F = 100 the plain 12x12 room (j >= 64: the second of
# a lane's two keys), 47 the walled room, 196 a 16x16 room, 2304 50x50, 11664 110x110
TIES = (("tie_F100_low", 100, lambda j: max(j) < 64), ("tie_F100_high", 100, lambda j: max(j) >= 64),
        ("tie_F47", 47, None), ("tie_F196", 196, None), ("tie_F2304", 2304, None), ("tie_F11664", 11664, None))
SHORT = ((100, 1), (196, 1), (2304, 1))
HEADER = [
    "Philox counters that reach the rare branches of the step and placement kernels.",
    "Written by tools/find_rare_philox.py; `--check` searches again and compares.",
    "friction: the owner's word is rejected and the first word of its friction stream is not;",
    "a second rejection in a row has probability 2^-64 and is out of scope.",
]


def _first(find, chunk, ok=None):
    """The first row, in (t, env) order, of find((t0, t1)) over ascending chunks that ok() accepts."""
    for t0 in range(0, T_END, chunk):
        for row in find((t0, min(T_END, t0 + chunk))):
            if ok is None or ok(row):
                return [int(v) for v in row]
    raise SystemExit("no hit below t = 2^32: choose another seed")


def search(nthreads, log=print):
    from oracle import oracle as O
    fixtures = []
    for m, owner in FRICTION:
        t0 = time.time()
        r = _first(lambda ts: O.find_friction_reject(SEED, m, owner, ENVS, ts, nthreads=nthreads), 1 << 27)
        fixtures.append({"kind": "friction", "id": f"friction_m{m}_o{owner}", "seed": SEED, "t": r[0], "env": r[1],
                         "owner": owner, "m": m, "rank_unrejected": r[2], "rank_replacement": r[3], "w": r[4],
                         "w_replacement": r[5]})
        log(f"{fixtures[-1]['id']}: t = {r[0]} env {r[1]} ({time.time() - t0:.0f} s)")
    for name, F, pred in TIES:
        t0 = time.time()
        chunk = max(64, (1 << 26) // (F * (ENVS[1] - ENVS[0])))     # about 2^26 keys a call: few hits, far below cap
        r = _first(lambda ts: O.find_reset_tie(SEED, F, RMAX, ENVS, ts, nthreads=nthreads), chunk,
                   None if pred is None else lambda row: pred((int(row[3]), int(row[4]))))
        fixtures.append({"kind": "tie", "id": name, "seed": SEED, "t": r[0], "env": r[1], "F": F, "r": r[2],
                         "j": [r[3], r[4]], "key": r[5]})
        log(f"{name}: t = {r[0]} env {r[1]} r = {r[2]} j = {r[3]}, {r[4]} ({time.time() - t0:.0f} s)")
    for F, N in SHORT:
        t0 = time.time()
        r = _first(lambda ts: O.find_reset_short(SEED, F, N, ENVS, ts, nthreads=nthreads), 1 << 22)
        fixtures.append({"kind": "short", "id": f"short_F{F}_N{N}", "seed": SEED, "t": r[0], "env": r[1], "F": F,
                         "N": N, "count": r[2]})
        log(f"{fixtures[-1]['id']}: t = {r[0]} env {r[1]} ({time.time() - t0:.0f} s)")
    return fixtures


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="search again and compare with the file; writes nothing")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="OpenMP threads (at most 16)")
    a = ap.parse_args()
    nthreads = max(1, min(16, a.threads))
    t0 = time.time()
    fixtures = search(nthreads)
    wall = time.time() - t0
    if a.check:
        with open(OUT) as f:
            have = json.load(f)["fixtures"]
        if have != fixtures:
            raise SystemExit(f"{OUT} differs from this search")
        print(f"{OUT}: same {len(fixtures)} fixtures ({wall:.0f} s on {nthreads} threads)")
        return
    doc = {"header": HEADER + [f"Wall time of the run that wrote this file: {wall:.0f} s on {nthreads} threads."],
           "fixtures": fixtures}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(fixtures)} fixtures in {wall:.0f} s")


if __name__ == "__main__":
    main()
