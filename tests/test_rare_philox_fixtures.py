"""tests/golden/rare_philox.json pinned on the CPU (tools/find_rare_philox.py wrote it).

Every fixture names a Philox counter that lands in a branch no random run takes: a rejected friction
word, two equal placement keys, a threshold pass that comes up short.  Here each is recomputed from
the scalar O.philox, so a stale file fails without a GPU; tests/test_gpu_rare_philox.py then puts
engines on those counters.  The friction fixtures are also replayed in the oracle on the scenario
of rare_philox_util.py: the agent that moves into the contested cell is the one the replacement
word picks, not the one the rejected word would have picked -- what a kernel without the rejection
branch gets wrong.
"""
import collections

import numpy as np
import pytest

import rare_philox_util as R

FRICTION = R.fixtures("friction")
TIES = R.fixtures("tie")
SHORT = R.fixtures("short")
_id = lambda x: x["id"]


def _thr(m):
    return (1 << 32) % m


def test_counts_per_kind():
    """What the GPU tests rely on: the m, owners, F and N the file must hold at the least."""
    per_m = collections.Counter(x["m"] for x in FRICTION)
    assert per_m[3] >= 2 and per_m[5] >= 1 and per_m[6] >= 2 and per_m[7] >= 2, per_m
    assert {0, 29} <= {x["owner"] for x in FRICTION if x["m"] == 3}
    assert max(x["owner"] for x in FRICTION if x["m"] == 7) >= 16
    seeds = {x["seed"] for x in R.fixtures()}
    assert len({x["seed"] for x in FRICTION}) == 1
    for s in seeds:
        assert s >> 32 and s & 0xFFFFFFFF and s < 1 << 64
    for x in R.fixtures():
        assert 64 <= x["env"] < 72 and 0 <= x["t"] < 1 << 32, x["id"]
    t100 = [x for x in TIES if x["F"] == 100]
    assert any(x["r"] + 1 <= 31 for x in t100) and any(max(x["j"]) >= 64 for x in t100)
    assert any(max(x["j"]) < 64 for x in t100)
    assert {47, 196, 2304} <= {x["F"] for x in TIES}
    assert all(x["r"] + 1 <= 31 for x in TIES)
    assert {(100, 1), (196, 1), (2304, 1)} <= {(x["F"], x["N"]) for x in SHORT}
    assert len({x["id"] for x in R.fixtures()}) == len(R.fixtures())


def test_every_fixture_has_a_gpu_case():
    """The ids collected from the GPU file's case tables: no fixture sits in the file unused."""
    pytest.importorskip("torch")
    import test_gpu_rare_philox as G
    assert G.used_fixture_ids() == {x["id"] for x in R.fixtures()}
    # Neumann m = 3 on every kernel form, Moore m = 5, 6, 7 on the six base forms
    assert {f for _, f in G.NEUMANN_CASES} == set(G.FRICTION_FORMS) and len(G.FRICTION_FORMS) == 12
    assert {(R.fixture(i)["m"], f) for i, f in G.MOORE_CASES} == {(m, f) for m in (5, 6, 7) for f in G.BASE_FORMS}


@pytest.mark.parametrize("fx", FRICTION, ids=_id)
def test_friction_fixture_conditions(fx):
    """The coin says move, the owner's word is rejected, the first friction word is not, and the two
    ranks differ."""
    from oracle import oracle as O
    m, key = fx["m"], R.key_of(fx["seed"])
    b = O.philox([fx["t"], fx["env"], fx["owner"], R.PUR_DECIDE << 28], key).astype(np.uint64)
    z, w = int(b[2]), int(b[3])
    assert z < 1 << 31
    assert w == fx["w"] and (w * m) & 0xFFFFFFFF < _thr(m)
    f = O.philox([fx["t"], fx["env"], fx["owner"], R.PUR_FRICTION << 28], key).astype(np.uint64)
    w1 = int(f[0])
    assert w1 == fx["w_replacement"] and (w1 * m) & 0xFFFFFFFF >= _thr(m)
    assert (w * m) >> 32 == fx["rank_unrejected"] and (w1 * m) >> 32 == fx["rank_replacement"]
    assert fx["rank_unrejected"] != fx["rank_replacement"]
    assert 0 <= fx["rank_replacement"] < m


@pytest.mark.parametrize("fx", FRICTION, ids=_id)
def test_friction_fixture_discriminates(fx):
    """One oracle step of the scenario: exactly one agent stands on the target, the requester of the
    replacement rank (a kernel that dropped the branch moves the requester of the unrejected rank)."""
    from oracle import oracle as O
    m, s = R.well_room()
    core = O.Core(m, s, R.friction_params(R.nbh_of(fx)))
    mir = R.Mirror([core], [0], fx["seed"], fx["env"], auto_reset=False)
    pos, cnt = R.friction_state(fx)
    assert not R.on_target(pos, cnt)
    mir.set_env(0, pos, cnt)
    mir.step(fx["t"], 1)
    assert mir.cnt[0] == cnt
    assert R.on_target(mir.pos[0], cnt) == [fx["owner"] + fx["rank_replacement"]]
    moved = np.flatnonzero(mir.pos[0, fx["owner"]:cnt] != pos[fx["owner"]:cnt]).tolist()
    assert moved == [fx["rank_replacement"]]


@pytest.mark.parametrize("fx", TIES, ids=_id)
def test_tie_fixture(fx):
    """The equal keys sit at ranks r, r + 1 in (key, j) order; reset_philox orders the pair by j, and
    with N = r + 1 only the lower j is placed."""
    from oracle import oracle as O
    F, r, (ja, jb) = fx["F"], fx["r"], fx["j"]
    keys = R.placement_keys(fx)
    assert ja < jb and keys[ja] == keys[jb] == fx["key"]
    order = np.lexsort((np.arange(F), keys))
    assert order[r] == ja and order[r + 1] == jb and r + 1 <= 31
    cells = np.arange(1000, 1000 + F)
    two = O.reset_philox_list(cells, r + 2, fx["seed"], fx["t"], fx["env"])
    assert two[r] == 1000 + ja and two[r + 1] == 1000 + jb
    one = O.reset_philox_list(cells, r + 1, fx["seed"], fx["t"], fx["env"])
    assert one[r] == 1000 + ja and 1000 + jb not in one
    assert np.array_equal(one, cells[order[:r + 1]])


@pytest.mark.parametrize("fx", SHORT, ids=_id)
def test_short_fixture(fx):
    """Fewer than N keys at or under the candidate threshold floor((2N + 16) 2^32 / F)."""
    from oracle import oracle as O
    F, N = fx["F"], fx["N"]
    thr = ((2 * N + 16) << 32) // F
    assert thr < 0xFFFFFFFF and O.reset_threshold(N, F) == thr
    keys = R.placement_keys(fx)
    assert int((keys <= thr).sum()) == fx["count"] < N


def test_search_functions_find_the_fixtures():
    """The library's search loops return each fixture from a window around its t (and nothing is
    found twice): the tool's result is what they report, independent of the thread count."""
    from oracle import oracle as O
    for fx in R.fixtures():
        ts, envs = (max(0, fx["t"] - 3), fx["t"] + 3), (fx["env"], fx["env"] + 1)
        for nthreads in (1, 3):
            if fx["kind"] == "friction":
                rows = O.find_friction_reject(fx["seed"], fx["m"], fx["owner"], envs, ts, nthreads=nthreads)
                want = [fx["t"], fx["env"], fx["rank_unrejected"], fx["rank_replacement"], fx["w"], fx["w_replacement"]]
            elif fx["kind"] == "tie":
                rows = O.find_reset_tie(fx["seed"], fx["F"], 31, envs, ts, nthreads=nthreads)
                want = [fx["t"], fx["env"], fx["r"], fx["j"][0], fx["j"][1], fx["key"]]
            else:
                rows = O.find_reset_short(fx["seed"], fx["F"], fx["N"], envs, ts, nthreads=nthreads)
                want = [fx["t"], fx["env"], fx["count"], 0, 0, 0]
            assert rows.tolist() == [want], fx["id"]
