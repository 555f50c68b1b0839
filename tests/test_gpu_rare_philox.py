"""Engines put on the Philox counters that no random run reaches (tests/golden/rare_philox.json,
found by tools/find_rare_philox.py and pinned on the CPU by test_rare_philox_fixtures.py), and
across the wrap of the u32 step index.

  friction   philox_friction's rejection: the owner's word is replaced from the owner's friction
             stream, inside a per-lane condition of every step kernel;
  tie        two equal placement keys: the free-list index j breaks the tie at every ranking site
             (the candidate pass, the full ranking, the large-F path, block_place_env);
  short      the threshold pass keeps fewer than N keys: the retry with every key, and in the block
             kernel past its key capacity the recomputing path;
  wrap       t runs over 2^32 - 1 into 0: draws, placements, episode lengths.

Counters are pure functions of (seed, t, global env, index), so set_state + step_index + env_base
put an engine's env on one.  Every case compares positions, counts, DFF bits, episodes and counters
with the oracle bit for bit, first right after the event (so a wrong placement is never stepped)
and again after more steps.
"""
import numpy as np
import pytest

import rare_philox_util as R
from test_gpu_geometry import INJ_KERNELS, obstacle_room

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ("FFM_STEP_SHARDS", "FFM_GROUP_ENVS", "FFM_GROUP_ONE", "FFM_WAVE_BLOCKS", "FFM_BLOCK_BS",
            "FFM_RESET_CANDIDATES")
T_RESET = 5                 # the step index of the reset() that places the other envs
_id = lambda v: v if isinstance(v, str) else "own_set" if isinstance(v, dict) else None


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


# ---------------------------------------------------------------------------
# Kernel forms: test_gpu_geometry's table (group G = 2 and 4, lane, wave, block K = 3, fused 4) and
# the forms it lacks.  pep / room: the `kernel` of set_env_params / set_env_rooms that turns the
# form on; one=False: the group kernel's loop form (FFM_GROUP_ONE=0).
# ---------------------------------------------------------------------------
def _form(epb, G=None, fused=1, kernel=None, one=None, pep=None, room=None):
    return dict(epb=epb, G=G, fused=fused, kernel=kernel, one=one, pep=pep, room=room)


FORMS = {k: _form(*v[:4]) for k, v in INJ_KERNELS.items()}
FORMS.update({
    "group_loop": _form(-3, 2, kernel="group", one=False),
    "group_pep": _form(-3, 4, kernel="group", pep="group"),
    "group_room": _form(-3, kernel="group", room="group"),
    "lane_pep": _form(-2, kernel="lane", pep="lane"),
    "lane_room": _form(-2, kernel="lane", room="lane"),
    "block_room": _form(3, kernel="block", room="block"),
    # rooms beyond 12x12: 16x16 (F = 196 > 128: the wave placement's threshold path), 50x50 and
    # 110x110 (the block kernel, LDS and global scratch)
    "lane16": _form(-2, kernel="lane"),
    "wave16": _form(-1, kernel="wave"),
    "block16": _form(3, kernel="block"),
    "block50": _form(0, kernel="block"),
    "block50_k1": _form(1, kernel="block"),      # one env per workgroup: the LDS has room for its parameter record
    "scratch110": _form(0, kernel="block_scratch"),
})
BASE_FORMS = tuple(INJ_KERNELS)
# the sets of the envs around the fixture's (per-env parameter forms); {} = the create-time values
OTHER_SETS = ({}, {"k_S": 1.5, "k_D": 1, "diffuse": 0.5, "decay": 0.1, "n_agents": 7},
              {"k_S": 10, "k_D": 2.5, "diffuse": 0.05, "decay": 0.6, "n_agents": 17})


def _layout(form_id, rooms, params, E, N, s, genv, seed, cap=R.A, fix_set=None):
    """The envs of a case, without an engine: (parameter sets, set of each env, rooms in use, room of
    each env, oracle mirror).  Envs of one room and one parameter point share an O.Core."""
    from oracle import oracle as O
    f = FORMS[form_id]
    sets_on = f["pep"] is not None or fix_set is not None
    others = [{**o, "n_agents": min(o["n_agents"], cap)} if "n_agents" in o else o for o in OTHER_SETS]
    sets = [fix_set or {}] + others if sets_on else [{}]
    soe = [0 if (e == s or not sets_on) else 1 + e % len(OTHER_SETS) for e in range(E)]
    rooms = list(rooms) if f["room"] else [rooms[0]]
    roe = [0 if e == s else e % len(rooms) for e in range(E)]
    made = {}

    def core(e):
        p = {**params, **{k: v for k, v in sets[soe[e]].items() if k != "n_agents"}}
        key = (roe[e], tuple(sorted(p.items())))
        if key not in made:
            made[key] = O.Core(np.array(rooms[roe[e]][0]), np.array(rooms[roe[e]][1]), p)
        return made[key]

    mir = R.Mirror([core(e) for e in range(E)], [sets[soe[e]].get("n_agents", N) for e in range(E)], seed, genv - s,
                   cap=cap)
    return sets if sets_on else None, soe, rooms, roe, mir


def _case(monkeypatch, form_id, rooms, params, E, N, s, genv, seed, cap=R.A, fix_set=None, setting=None, shards=None):
    """(engine, oracle mirror) of E envs with the env of global id `genv` at local index s.
    rooms: (map, sff) pairs, the first the create-time room and the fixture env's; the others are
    used by the room forms (envs alternate).  fix_set: the fixture env's own parameter set."""
    from ffm_amd.engine import Engine
    f = FORMS[form_id]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("FFM_GROUP_ENVS", f["G"]), ("FFM_GROUP_ONE", 0 if f["one"] is False else None),
                 ("FFM_RESET_CANDIDATES", setting), ("FFM_STEP_SHARDS", shards)):
        if v is not None:
            monkeypatch.setenv(k, str(v))
    sets, soe, rooms, roe, mir = _layout(form_id, rooms, params, E, N, s, genv, seed, cap=cap, fix_set=fix_set)
    env_base = genv - s
    eng = Engine(rooms[0][0], rooms[0][1], n_envs=E, n_agents=N, agent_capacity=cap, params=params, rng="philox",
                 seed=seed, auto_reset=True, env_base=env_base, envs_per_block=f["epb"])
    if sets is not None:
        eng.set_env_params(sets, np.asarray(soe, np.int32), kernel=f["pep"])
    if f["room"]:
        eng.set_env_rooms(rooms, np.asarray(roe, np.int32), kernel=f["room"])
    li = eng.launch_info()
    if f["fused"] > 1:
        assert li["multi"], li
    else:
        assert li["kernel"] == f["kernel"], li
        if f["kernel"] == "group":
            assert li["group_one"] == (f["one"] is not False), li
            assert f["G"] is None or li["group_g"] == f["G"], li
    assert li["env_rooms"] == (len(rooms) if f["room"] else 0), li
    return eng, mir


def _event_in_step(eng, mir, form_id, s, state, t, check):
    """reset() at T_RESET, the fixture env's state injected, then the step keyed t (for the fused
    form the first sub-step of one launch of 4) and three more.  check(mir): the oracle went
    through the event, asserted right after the step t."""
    fused = FORMS[form_id]["fused"]
    H, W = mir.dff.shape[1:]
    eng.step_index = T_RESET
    eng.reset()
    mir.reset(T_RESET)
    pos, cnt = state
    eng.set_state(s, positions=pos[None], counts=np.array([cnt], np.int32), dff=np.zeros((1, H, W), np.float32))
    mir.set_env(s, pos, cnt)
    eng.step_index = t
    mir.step(t, 1)
    check(mir)
    try:
        if fused > 1:
            eng.set_fused_steps(fused)
            mir.step(t + 1, fused - 1)
            eng.step(fused)
        else:
            eng.step(1)
            R.assert_engine_equals(eng, mir, "the step of the event")
            mir.step(t + 1, 3)
            eng.step(3)
        R.assert_engine_equals(eng, mir, "three steps later")
        assert eng.step_index == (t + 4) & 0xFFFFFFFF
    finally:
        eng.close()


def _event_by_reset(eng, mir, t):
    """reset() keyed t: the stand-alone placement kernels; then two steps from that placement."""
    try:
        eng.step_index = t
        eng.reset()
        mir.reset(t)
        assert eng.step_index == (t + 1) & 0xFFFFFFFF
        R.assert_engine_equals(eng, mir, "reset()")
        eng.step(2)
        mir.step(t + 1, 2)
        R.assert_engine_equals(eng, mir, "two steps after reset()")
        assert eng.step_index == (t + 3) & 0xFFFFFFFF
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# Friction
# ---------------------------------------------------------------------------
FRICTION_E, FRICTION_N = 41, 20
# the fixture env's local index: slot 0, the last slot of a group of 4, an env beyond the first wave
FRICTION_SLOTS = (0, 3, 37)
FRICTION_FORMS = BASE_FORMS + ("group_loop", "group_pep", "group_room", "lane_pep", "lane_room", "block_room")
NEUMANN_CASES = [(x["id"], f) for x in R.fixtures("friction") if x["m"] == 3 for f in FRICTION_FORMS]
MOORE_CASES = [(x["id"], f) for x in R.fixtures("friction") if x["m"] > 4 for f in BASE_FORMS]


def _friction_rooms():
    from ffm_amd.data import l1_sff
    m2 = obstacle_room(12, 12)
    return [R.well_room(), (m2, l1_sff(m2))]


def _friction(monkeypatch, fid, form_id, s):
    fx = R.fixture(fid)
    eng, mir = _case(monkeypatch, form_id, _friction_rooms(), R.friction_params(R.nbh_of(fx)), FRICTION_E, FRICTION_N,
                     s, fx["env"], fx["seed"])
    state = R.friction_state(fx)

    def check(mir):     # the oracle's winner is the replacement-rank requester, not the unrejected-rank one
        assert R.on_target(mir.pos[s], mir.cnt[s]) == [fx["owner"] + fx["rank_replacement"]]

    _event_in_step(eng, mir, form_id, s, state, fx["t"], check)


@pytest.mark.parametrize("s", FRICTION_SLOTS)
@pytest.mark.parametrize("fid,form_id", NEUMANN_CASES, ids=_id)
def test_friction_rejection_neumann(monkeypatch, fid, form_id, s):
    """m = 3 (threshold 1: w = 0 alone is rejected), owner index 0 and 29, on every kernel form."""
    _friction(monkeypatch, fid, form_id, s)


@pytest.mark.parametrize("s", FRICTION_SLOTS)
@pytest.mark.parametrize("fid,form_id", MOORE_CASES, ids=_id)
def test_friction_rejection_moore(monkeypatch, fid, form_id, s):
    """m = 5 (threshold 1), 6 and 7 (threshold 4), low and high owner indices."""
    _friction(monkeypatch, fid, form_id, s)


# ---------------------------------------------------------------------------
# Placement: ties and short threshold passes
# ---------------------------------------------------------------------------
PLACE_E = 13
PLACE_PARAMS = {"k_S": 10, "k_D": 1, "diffuse": 0.2, "decay": 0.2, "neighborhood": "neumann"}
SIDE_OF_F = {100: 12, 47: 12, 196: 16, 2304: 50, 11664: 110}      # square rooms; 47: the walled 12x12 room
FORMS_OF_F = {100: BASE_FORMS, 47: BASE_FORMS, 196: ("lane16", "wave16", "block16"), 2304: ("block50",),
              11664: ("scratch110",)}
CAND_FORMS = ("group_g2", "group_g4", "lane", "wave")      # step kernels built with the candidate pass


def _place_rooms(F):
    """The room with F free cells, and a second room for the room forms."""
    from ffm_amd.data import l1_sff, make_room
    m = make_room(SIDE_OF_F[F], SIDE_OF_F[F])
    if F == 47:                     # test_gpu_placement_candidates' walled room: an odd count
        m[6:11, 1:11] = 2
        m[5, 1:4] = 2
    assert int((m == 0).sum()) == F
    out = [(m, l1_sff(m))]
    if m.shape == (12, 12):
        m2 = obstacle_room(12, 12)
        out.append((m2, l1_sff(m2)))
    return out


def _below_exit(rooms):
    """One agent on the cell below the exit: it leaves in the next step (exit forcing), and with
    auto-reset the env is re-placed with that step's keys."""
    m = rooms[0][0]
    W = m.shape[1]
    assert m[0, W // 2] == 3 and m[1, W // 2] == 0
    return W + W // 2


def _placed_in_step(monkeypatch, fx, form_id, N, s, cap=R.A, fix_set=None, setting=None):
    rooms = _place_rooms(fx["F"])
    eng, mir = _case(monkeypatch, form_id, rooms, PLACE_PARAMS, PLACE_E, N, s, fx["env"], fx["seed"], cap=cap,
                     fix_set=fix_set, setting=setting)
    pos = np.full(cap, 0xFFFF, np.uint16)
    pos[0] = _below_exit(rooms)

    def check(mir):     # the agent left and the env was re-placed in the step keyed t
        assert mir.eps[s] == 1 and mir.cnt[s] == mir.Ns[s]

    _event_in_step(eng, mir, form_id, s, (pos, 1), fx["t"], check)


def _placed_by_reset(monkeypatch, fx, form_id, N, s, cap=R.A, setting=None):
    eng, mir = _case(monkeypatch, form_id, _place_rooms(fx["F"]), PLACE_PARAMS, PLACE_E, N, s, fx["env"], fx["seed"],
                     cap=cap, setting=setting)
    _event_by_reset(eng, mir, fx["t"])


# (fixture, form, N - r, FFM_RESET_CANDIDATES): N = r + 1 places the lower j of the pair alone, N = r + 2
# both in j order; "0" turns the candidate pass off (the full ranking) where a kernel has one
TIE_STEP_CASES = [(x["id"], f, d, c) for x in R.fixtures("tie") for f in FORMS_OF_F[x["F"]] for d in (1, 2)
                  for c in ((None, "0") if x["F"] <= 128 and f in CAND_FORMS else (None,))]
TIE_RESET_CASES = [(x["id"], f, d, c) for x in R.fixtures("tie") for f in FORMS_OF_F[x["F"]] if f not in ("group_g2", "fused4")
                   for d in (1, 2) for c in ((None, "0") if x["F"] <= 128 else (None,))]


@pytest.mark.parametrize("fid,form_id,d,setting", TIE_STEP_CASES, ids=_id)
def test_tie_placed_in_step(monkeypatch, fid, form_id, d, setting):
    """The step kernels' own placement: an agent below the exit leaves in the step keyed t and the
    env is re-placed with the keys that hold the tie (the wave placement's three ranking sites by
    F and setting, block_place_env in the block kernels)."""
    fx = R.fixture(fid)
    _placed_in_step(monkeypatch, fx, form_id, fx["r"] + d, (3, 10)[d - 1], setting=setting)


@pytest.mark.parametrize("fid,form_id,d,setting", TIE_RESET_CASES, ids=_id)
def test_tie_placed_by_reset(monkeypatch, fid, form_id, d, setting):
    """reset() keyed t: the stand-alone placement kernels (by blocks at 110x110)."""
    fx = R.fixture(fid)
    _placed_by_reset(monkeypatch, fx, form_id, fx["r"] + d, (3, 10)[d - 1], setting=setting)


# (fixture, form, capacity, N at create, the fixture env's own set).  The threshold pass keeps no key
# for N = 1, so the kernels retry with every key:
#   wave16 / lane16   wave_reset_env's threshold path (F = 196 > 128);
#   block3            block_place_env, F = 100 <= its key capacity: retry, then rank all;
#   block50, cap 4    block_keys_cap(4, 2304) = min(2304, m + 8 ceil(sqrt(m)) + 64) with m = 2 * 4 + 16 = 24:
#                     24 + 8 * 5 + 64 = 128 < 2304, so the retry's 2304 keys take the recomputing path;
#   block_room        the room form, with the F of the env's own room.
SHORT_STEP_CASES = [
    ("short_F196_N1", "wave16", 32, 1, None),
    ("short_F196_N1", "lane16", 32, 1, None),
    ("short_F196_N1", "lane16", 32, 12, {"n_agents": 1}),
    ("short_F196_N1", "block16", 32, 12, {"n_agents": 1}),
    ("short_F100_N1", "block3", 32, 1, None),
    ("short_F100_N1", "block3", 32, 12, {"n_agents": 1}),
    ("short_F100_N1", "block_room", 32, 12, {"n_agents": 1}),
    ("short_F2304_N1", "block50", 4, 1, None),
    ("short_F2304_N1", "block50_k1", 4, 3, {"n_agents": 1}),
]
SHORT_RESET_CASES = [
    # (reset() places by the wave placement: its threshold path from F = 129 on)
    ("short_F196_N1", "wave16", 32), ("short_F196_N1", "lane16", 32), ("short_F2304_N1", "block50", 4),
]


def test_short_cases_reach_the_recomputing_path():
    """The arithmetic of the comment above, on the fixture the 50x50 cases use."""
    m = 2 * 4 + 16
    r = next(r for r in range(1, m) if r * r >= m)
    assert m + 8 * r + 64 == 128 < R.fixture("short_F2304_N1")["F"]


@pytest.mark.parametrize("fid,form_id,cap,N,fix_set", SHORT_STEP_CASES, ids=_id)
def test_short_placed_in_step(monkeypatch, fid, form_id, cap, N, fix_set):
    _placed_in_step(monkeypatch, R.fixture(fid), form_id, N, 3, cap=cap, fix_set=fix_set)


@pytest.mark.parametrize("fid,form_id,cap", SHORT_RESET_CASES, ids=_id)
def test_short_placed_by_reset(monkeypatch, fid, form_id, cap):
    _placed_by_reset(monkeypatch, R.fixture(fid), form_id, 1, 10, cap=cap)


def used_fixture_ids():
    """The fixtures at least one case above runs (test_rare_philox_fixtures.py checks: all of them)."""
    cases = NEUMANN_CASES + MOORE_CASES + TIE_STEP_CASES + TIE_RESET_CASES + SHORT_STEP_CASES + SHORT_RESET_CASES
    return {c[0] for c in cases}


# ---------------------------------------------------------------------------
# The step index wraps
# ---------------------------------------------------------------------------
WRAP_E, WRAP_N, WRAP_T, WRAP_SEED, WRAP_BINS = 40, 8, 12, 42, 32
WRAP_T0 = (1 << 32) - 5


def _wrap_engine(monkeypatch, form_id, shards=None):
    from ffm_amd.data import l1_sff, make_room
    m = make_room(12, 12, (0, 1), 10)      # the whole top wall an exit: 8 agents leave within the 12 steps
    return _case(monkeypatch, form_id, [(m, l1_sff(m))], PLACE_PARAMS, WRAP_E, WRAP_N, 0, 0, WRAP_SEED, shards=shards)


@pytest.mark.parametrize("mode", ["single", "sharded", "fused"])
@pytest.mark.parametrize("form_id", ["group_g2", "lane", "wave", "block3"])
def test_step_index_wraps(monkeypatch, form_id, mode):
    """reset() keyed 2^32 - 5, then 12 steps keyed 2^32 - 4 .. 2^32 - 1, 0 .. 7: step(1) twelve times,
    step(12) once under FFM_STEP_SHARDS=2, and fused launches of 4 of which one spans the wrap (two
    single steps first: the launches are keyed 2^32 - 2 .. 1, 2 .. 5, 6 .. 7; the shards are the
    group kernel's, the other kernels take step(12) as twelve launches).  The oracle steps
    with t mod 2^32; episode records carry t_end as u32 and lengths (t_end - start) mod 2^32."""
    eng, mir = _wrap_engine(monkeypatch, form_id, shards=2 if mode == "sharded" else None)
    try:
        eng.set_episode_log(capacity=WRAP_E * WRAP_T, hist_bins=WRAP_BINS)
        eng.step_index = WRAP_T0
        eng.reset()
        mir.reset(WRAP_T0)
        assert eng.step_index == WRAP_T0 + 1
        mir.step(WRAP_T0 + 1, WRAP_T)
        want = np.asarray(mir.records, np.int64).reshape(-1, 4)
        # most envs end their first episode after the wrap, so its length is computed across it
        # (placed at 2^32 - 5: t_end + 5 steps), and are re-placed with a small t and stepped on
        first = want[want[:, 1] == 0]
        across = first[first[:, 3] < 8]
        assert len(across) >= WRAP_E // 2 and (across[:, 2] == across[:, 3] + 5).all()
        if mode == "single":
            for _ in range(WRAP_T):
                eng.step(1)
        elif mode == "sharded":
            eng.step(WRAP_T)
        else:
            eng.step(2)
            eng.set_fused_steps(4)
            eng.step(WRAP_T - 2)
        # 2^32 - 5, + 1 for reset(), + 12 steps = 2^32 + 8
        assert eng.step_index == (WRAP_T0 + 1 + WRAP_T) & 0xFFFFFFFF == 8
        R.assert_engine_equals(eng, mir, "across the wrap")
        got = eng.drain_episodes().view(np.uint32).astype(np.int64)
        want = want[np.lexsort((want[:, 1], want[:, 0]))]
        assert np.array_equal(got, want), (got, want)
        st = eng.episode_stats()
        ln = want[:, 2]
        assert (st["count"], st["sum"], st["sum_sq"], st["min"], st["max"]) == \
            (len(ln), int(ln.sum()), int((ln * ln).sum()), int(ln.min()), int(ln.max()))
        assert np.array_equal(st["hist"], np.bincount(np.minimum(ln, WRAP_BINS - 1), minlength=WRAP_BINS))
    finally:
        eng.close()


@pytest.mark.parametrize("form_id", ["group_g2", "block3"])
def test_reset_at_last_step_index(monkeypatch, form_id):
    """reset() keyed 2^32 - 1 leaves the step index 0; the next steps are keyed 0 and 1."""
    eng, mir = _wrap_engine(monkeypatch, form_id)
    _event_by_reset(eng, mir, (1 << 32) - 1)
