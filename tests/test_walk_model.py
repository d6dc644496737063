"""The walk model (tests/walk_model.py) before it judges the kernel
(tests/test_walk_trace.py), on the host alone: over every plan's batches the
interval the model's walk ends with is the CPU oracle's, bit for bit, empty
intervals included -- so its steps, skip lookups and jumps compose to the
search -- and every event class a plan is about holds at least its floor of
reads.  Also the record decoder, and the refusals of kfmi_search_trace that
need no device.
"""
import ctypes

import numpy as np
import pytest

import test_walk_trace as twt
import walk_model as wm

BAD_ARGUMENT, NOT_ON_DEVICE = 1, None


@pytest.fixture(scope="module")
def images(kfmi_mod):
    cache = {}

    def image(name, k):
        if (name, k) not in cache:
            idx = kfmi_mod.Index.build(twt.TEXTS[name][0].tobytes(), k=k, d=64)
            cache[(name, k)] = idx.image().copy()
            idx.close()
        return cache[(name, k)]

    return image


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", list(twt.TEXTS))
@pytest.mark.parametrize("plan", list(twt.PLANS))
def test_model_ends_where_the_oracle_ends(kfmi_mod, oracle_mod, images, plan, name, k):
    fb = kfmi_mod.ftab_auto_bases(twt.TEXTS[name][0].size + 1, k, 1 << 40)
    assert fb % k == 0 and fb >= k
    for label, q, st, mod in twt.batches(plan, name, k, fb):
        want = oracle_mod.search(images(name, 1 if q.shape[1] % k else k), q)[0].reshape(-1, 2)
        got = np.stack([mod["L"], mod["R"]], axis=1)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (label, int(bad.size), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
        steps = q.shape[1] // k
        took = mod["jump_outcome"] == wm.TAKEN
        walked = mod["start_steps"] + mod["steps"] + (16 // k) * mod["skip_hits"]
        assert (np.where(took, mod["jump_pos"] + mod["jump_nb"] // k, walked) == steps).all(), label
        assert (mod["skip_misses"] <= 1).all() and (mod["jump_tried"] <= 1).all()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", list(twt.TEXTS))
@pytest.mark.parametrize("plan", list(twt.PLANS))
def test_no_plan_has_an_empty_class(kfmi_mod, plan, name, k):
    fb = kfmi_mod.ftab_auto_bases(twt.TEXTS[name][0].size + 1, k, 1 << 40)
    counts = twt.class_counts(plan, name, k, fb)
    _, needed, floor = twt.PLANS[plan]
    short = {c: counts.get(c, 0) for c in needed if counts.get(c, 0) < floor}
    assert not short, (plan, name, k, short)


def test_the_third_text_ends_one_base_into_a_word():
    assert twt.TEXTS["n2513"][0].size % 16 == 1
    assert sorted(t.size % 16 for t, _, _ in twt.TEXTS.values()) == [0, 1, 13]


def test_model_of_jump_split():
    assert wm.jump_split_of(False, 1, 4, 100) == 1
    assert wm.jump_split_of(True, 0, 0, 100) == 0 and wm.jump_split_of(True, 0, 4, 100) == 4
    assert wm.jump_split_of(True, 1, 0, 250) == 0x100 and wm.jump_split_of(True, 2, 4, 250) == 0x104
    assert wm.jump_split_of(True, 1, 4, 192) == 0x304 and wm.jump_split_of(True, 1, 4, 193) == 0x004


def test_decode_trace(kfmi_mod):
    rec = np.array([[7 | 3 << 16 | 1 << 24, 1 | 2 | 0 << 2 | 5 << 4 | 90 << 16, 3, 0x304],
                    [50, 1 | 2 << 2 | 12 << 4 | 240 << 16, 0, 0x100],
                    [0, 0, 0, 1],
                    [256, 1 | 1 << 2 | 3 << 4 | 250 << 16, 3, 4]], dtype=np.uint32)
    d = kfmi_mod.decode_trace(rec)
    assert tuple(d) == kfmi_mod.TRACE_FIELDS == wm.FIELDS
    assert d["steps"].tolist() == [7, 50, 0, 256] and d["skip_hits"].tolist() == [3, 0, 0, 0]
    assert d["skip_misses"].tolist() == [1, 0, 0, 0] and d["jump_tried"].tolist() == [1, 1, 0, 1]
    assert d["jump_pos"].tolist() == [5, 12, -1, 3] and d["jump_nb"].tolist() == [90, 240, -1, 250]
    assert d["jump_line"].tolist() == [1, 0, -1, 0] and d["jump_outcome"].tolist() == [0, 2, -1, 1]
    assert [kfmi_mod.TRACE_JUMP_OUTCOMES[o] for o in d["jump_outcome"] if o >= 0] == ["taken", "differed", "refused"]
    assert d["start_steps"].tolist() == [3, 0, 0, 3] and d["jump_split"].tolist() == [0x304, 0x100, 1, 4]


def test_refusals_without_a_device(kfmi_mod):
    """Null arguments and handles that are not on a device are refused before anything runs."""
    K = kfmi_mod
    L = K.load()
    t = twt.TEXTS["n2513"][0]
    idx = K.Index.build(t.tobytes(), k=2, d=64)
    q = K.Queries.from_array(twt._reads(t, np.arange(8), 50))
    r = K.Results.alloc(8)
    rec = np.full((8, 4), 0xABCD, dtype=np.uint32)
    out = rec.ctypes.data_as(ctypes.c_void_p)
    try:
        bad = L.kfmi_search_trace(idx.ptr, q.ptr, r.ptr, None)
        assert bad != 0 and b"argument" in L.errorCommon(bad).lower()
        for args in ((None, q.ptr, r.ptr, out), (idx.ptr, None, r.ptr, out), (idx.ptr, q.ptr, None, out)):
            assert L.kfmi_search_trace(*args) == bad
        r9 = K.Results.alloc(9)
        assert L.kfmi_search_trace(idx.ptr, q.ptr, r9.ptr, out) == bad      # another count of results
        r9.close()
        off = L.kfmi_search_trace(idx.ptr, q.ptr, r.ptr, out)               # nothing transferred
        assert off not in (0, bad) and b"device" in L.errorCommon(off).lower()
        assert (rec == 0xABCD).all()
    finally:
        q.close()
        r.close()
        idx.close()
