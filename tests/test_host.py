"""Host-side logic that needs no GPU: key packing, the numpy._core alias used by
the table loaders, bench helpers."""
import importlib
import pickle
import sys

import numpy as np

from ffm_amd import learn_keys as K


def test_numpy_core_alias_loads_numpy2_key_pickles(monkeypatch):
    """A table pickle written under NumPy 2 names numpy._core.multiarray.scalar
    (model/ffm_unified.py:8-10 aliases it for NumPy 1.x).  Simulate an
    interpreter without numpy._core: the alias must make such bytes load."""
    b = K.to_cells_bytes(K.pack([1, 0, 2, 3, 1, 0, 0, 0, 2, 3, 0, 1, 2], 4, 7))
    assert b"numpy._core" in b or b"numpy.core" in b
    saved = {k: v for k, v in sys.modules.items() if k == "numpy._core" or k.startswith("numpy._core.")}
    for k in saved:
        monkeypatch.delitem(sys.modules, k)
    monkeypatch.setattr(importlib.util, "find_spec", lambda name, *a: None)
    K.ensure_numpy_core_alias()
    assert sys.modules["numpy._core"] is np.core
    key = K.from_cells_bytes(b)
    assert K.unpack(key, 13) == ((1, 0, 2, 3, 1, 0, 0, 0, 2, 3, 0, 1, 2), (4, 7))


def test_numpy_core_alias_noop_under_numpy2():
    before = sys.modules.get("numpy._core")
    K.ensure_numpy_core_alias()
    assert sys.modules.get("numpy._core") is before


def test_rank_key_roundtrip():
    k = ((3, 0, 2, 1), (255, 17))
    assert K.to_rank_tuple(K.from_rank_tuple(k)) == k
    b = pickle.dumps(k)
    assert K.to_rank_tuple(K.from_rank_tuple(pickle.loads(b))) == k


def test_bench_dump_outputs_writes_float_arrays_and_fixed_samples(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 / float64 files only, dead position slots as -1, table
    rows sorted by key with exact key halves, and the same seeded sample on every call once
    the state or a table exceeds its byte budget."""
    import bench
    rng = np.random.default_rng(3)
    E, A, H, W = 40, 6, 5, 7
    pos = rng.integers(0, H * W, (E, A)).astype(np.uint16)
    cnt = rng.integers(0, A + 1, E).astype(np.int32)
    dff = rng.random((E, H, W), dtype=np.float32)
    keys = rng.permutation(np.arange(1, 31, dtype=np.uint64) * np.uint64(0x1_0000_0003))
    hv = rng.random((30, 5))
    tabs = {"V": (keys, hv[:, 0].copy()), "H": (keys, hv)}

    def load(d):
        out = {f.name[:-4]: np.load(f) for f in d.iterdir()}
        assert all(a.dtype in (np.float32, np.float64) for a in out.values())
        return out

    bench.dump_outputs(str(tmp_path / "all"), 0, 1, (pos, cnt, dff), tabs)
    d = load(tmp_path / "all")
    assert np.array_equal(d["env_index"], np.arange(E))
    assert np.array_equal(d["counts"], cnt) and np.array_equal(d["dff"], dff)
    live = np.arange(A)[None, :] < cnt[:, None]
    assert np.array_equal(d["positions"][live], pos[live]) and np.all(d["positions"][~live] == -1)
    order = np.argsort(keys)
    got = d["H_keys_hi"].astype(np.uint64) << np.uint64(32) | d["H_keys_lo"].astype(np.uint64)
    assert np.array_equal(got, keys[order]) and np.array_equal(d["H_values"], hv[order])
    assert d["V_values"].shape == (30, 1) and np.array_equal(d["V_values"][:, 0], hv[order, 0])

    monkeypatch.setattr(bench, "DUMP_STATE_BYTES", 10 * (4 * (A + 1 + H * W) + 8))
    monkeypatch.setattr(bench, "DUMP_TABLE_BYTES", 2 * 7 * 8 * (3 + 5))
    bench.dump_outputs(str(tmp_path / "a"), 0, 1, (pos, cnt, dff), tabs)
    bench.dump_outputs(str(tmp_path / "b"), 0, 1, (pos, cnt, dff), tabs)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["env_index"].astype(int)
    assert len(idx) == 10 and np.all(np.diff(idx) > 0) and np.array_equal(a["dff"], dff[idx])
    rows = a["H_row_index"].astype(int)
    assert len(rows) == 7 and np.array_equal(a["H_values"], hv[order][rows])
