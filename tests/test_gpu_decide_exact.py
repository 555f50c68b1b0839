"""The group kernel's exact decide (the NumPy arithmetic behind lane_decide's fast pass).

The fast pass hands an agent to the exact pass when its draw lies within kFastMargin = 1e-4 of
a cdf boundary: about 7e-4 of the drawn decisions.  The Neumann group kernels run that pass
wave-cooperatively (group_exact_coop, core_group.hip: candidate k on lane k, one pending agent
at a time), the Moore ones per lane.  Two halves, both bit for bit against the oracle:

  * forced: a variant library built with FFM_FAST_MARGIN=1.0f, where the fast pass never
    accepts, so every drawn decision takes the exact pass and a chunk carries up to 64 pending
    lanes.  The library is bound when ffm_amd.engine is imported, so the cases run in one
    fresh child process (this file with --child) and report one line each;
  * natural: the product library at 2,048 envs, where the exact pass runs on the order of a
    thousand times in 40 steps and now and then for two lanes of one chunk.

Every case is a 12x12 room.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_WAVE_BLOCKS")
SEED = 42
H = W = 12
T_FORCED = 30


def _params(nbh, k_S=3, k_D=1):
    return {"k_S": k_S, "k_D": k_D, "diffuse": 0.2, "decay": 0.2, "neighborhood": nbh}


def _room(room):
    from ffm_amd.data import make_room, l1_sff
    m = make_room(H, W)
    if room == "obstacle":      # an inner wall (a gap of two cells), a pillar and two exits
        m[H // 2, 1:W - 3] = 2
        m[H // 4:H // 4 + 2, W // 3:W // 3 + 2] = 2
        m[H - H // 3, 0] = 3
    return m, l1_sff(m)


# ---------------------------------------------------------------------------
# Cases: (id, kind, room, E, N, G, nbh, k_D, k_S, wave_blocks)
# ---------------------------------------------------------------------------
def _forced_cases():
    cases = []
    for G in (2, 4):
        for nbh in ("neumann", "moore"):
            for k_D in (1, 2):
                for k_S in (3, 0):
                    for E, N in ((37, 32), (3, 5)):
                        cases.append(("reset", "plain", E, N, G, nbh, k_D, k_S, None))
            cases.append(("reset", "obstacle", 37, 32, G, nbh, 1, 3, None))
        for k_D in (1, 2):       # sc - mx far below exp's underflow bound of -104
            cases.append(("blob", "plain", 9, 30, G, "neumann", k_D, 3, None))
    for nbh in ("neumann", "moore"):     # a full group, then a one-env group on the same wave
        cases.append(("reset", "plain", 17, 32, 4, nbh, 1, 3, 1))
    return [("-".join(str(x) for x in c), *c) for c in cases]


FORCED = _forced_cases()


def _blob_start(E, N):
    """A 6x5 blob of agents in the middle of the room on a DFF of up to a few hundred on and
    around it (the dynamics do not reach this from reset())."""
    rng = np.random.default_rng(3)
    cells = np.array([x * W + y for x in range(3, 9) for y in range(4, 9)], np.uint16)
    assert N == len(cells)
    pos0 = np.stack([rng.permutation(cells) for _ in range(E)]).astype(np.uint16)
    cnt0 = np.full(E, N, np.int32)
    dff0 = np.zeros((E, H, W), np.float32)
    dff0[:, 2:10, 3:10] = (400 * rng.random((E, 8, 7)) ** 3).astype(np.float32)
    return pos0, cnt0, dff0


@functools.lru_cache(maxsize=None)
def _oracle(kind, room, E, N, nbh, k_D, k_S, T, t0=1):
    from oracle import oracle as O
    m, s = _room(room)
    core = O.Core(m, s, _params(nbh, k_S, k_D))
    if kind == "blob":
        pos, cnt, dff = _blob_start(E, N)
    else:
        pos = np.stack([core.reset_philox(N, SEED, 0, e) for e in range(E)])
        cnt = np.full(E, N, np.int32)
        dff = np.zeros((E, H, W), np.float32)
    eps = np.zeros(E, np.int32)
    for t in range(t0, t0 + T):
        core.step_philox_batch(pos, cnt, dff, eps, SEED, t, True, N, 0, 16)
    for a in (pos, cnt, dff, eps):
        a.setflags(write=False)
    return pos, cnt, dff, eps


def _run_case(kind, room, E, N, G, nbh, k_D, k_S, wave_blocks, T, E_ref=None):
    """One engine run against the oracle; returns None or what differs."""
    from ffm_amd.engine import Engine
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ["FFM_GROUP_ENVS"] = str(G)
    if wave_blocks:
        os.environ["FFM_WAVE_BLOCKS"] = str(wave_blocks)
    m, s = _room(room)
    eng = Engine(m, s, n_envs=E, n_agents=N, params=_params(nbh, k_S, k_D), rng="philox", seed=SEED,
                 auto_reset=True)
    li = eng.launch_info()
    if (li["kernel"], li["group_g"]) != ("group", G) or (wave_blocks and li["blocks"] != wave_blocks):
        eng.close()
        return f"launch {li}"
    if kind == "blob":
        pos0, cnt0, dff0 = _blob_start(E, N)
        eng.set_state(0, positions=pos0, counts=cnt0, dff=dff0)
        eng.step_index = 1
    else:
        eng.reset()
    eng.step(T)
    gpos, gcnt, gdff = eng.get_state()
    eng.close()
    pos, cnt, dff, eps = (a[:E] for a in _oracle(kind, room, E_ref or E, N, nbh, k_D, k_S, T))
    if not np.array_equal(gcnt, cnt):
        return f"counts differ in envs {np.flatnonzero(gcnt != cnt)[:8].tolist()}"
    for e in range(E):
        if not np.array_equal(gpos[e, :cnt[e]], pos[e, :cnt[e]]):
            return f"env {e} positions"
    bad = np.argwhere(gdff.view(np.uint32) != dff.view(np.uint32))
    if bad.size:
        return f"DFF bits differ at (env, x, y) {bad[:8].tolist()}"
    return None


def _child_main():
    """Every forced case with the library in FFM_LIB_PATH; one JSON line per case."""
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    for cid, *c in FORCED:
        try:
            err = _run_case(*c, T_FORCED)
        except Exception as ex:     # reported as the case's failure
            err = f"{type(ex).__name__}: {ex}"
        print(json.dumps({"case": cid, "error": err}), flush=True)


# ---------------------------------------------------------------------------
# Forced fallback
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced_results(tmp_path_factory):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ffm_amd import build as B
    out = str(tmp_path_factory.mktemp("forced") / "libffm_forced.so")
    # one source file's compile time where the product build's objects are there to link with
    have_objs = all(os.path.exists(os.path.join(B.LIB_PATH + ".obj", s + ".o")) for s in B.SOURCES)
    B.build(out=out, defines=["FFM_FAST_MARGIN=1.0f"], only=["core_group.hip"] if have_objs else None)
    env = dict(os.environ, FFM_LIB_PATH=out)
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            res[d["case"]] = d["error"]
    return r.returncode, r.stderr[-2000:], res


@pytest.mark.parametrize("cid", [c[0] for c in FORCED])
def test_forced_fallback(forced_results, cid):
    rc, err, res = forced_results
    assert cid in res, f"the child did not reach this case (exit {rc}): {err}"
    assert res[cid] is None, res[cid]


# ---------------------------------------------------------------------------
# Product library, natural rate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 4])
def test_natural_rate(G):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        err = _run_case("reset", "plain", 2048, 32, G, "neumann", 1, 3, None, 40)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert err is None, err


if __name__ == "__main__" and "--child" in sys.argv:
    _child_main()
