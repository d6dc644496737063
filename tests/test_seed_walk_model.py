"""The seed walk model (tests/seed_walk_model.py) before it judges the kernels
(tests/test_seed_trace.py), on the host alone.  Over every batch the GPU tests
use, the model's intervals and spans are seed_ref.reference's -- the definition,
on the CPU oracle -- under every table setting, and its count of units that did
not occur on their own is the reference's; its rounds account for every K-step
of the task.  Every class of tasks a batch is about holds its tasks, in the
batch and in each 16-lane group of its first wave, counted on the model alone.
Also expected_form against the table of test_fetch_forms.py, the record
decoders, and the refusals of the two traced calls that need no device.
"""
import ctypes

import numpy as np
import pytest

import seed_ref as sr
import seed_walk_model as swm
import test_seed_trace as tst

FLOOR = 16
BATCHES = [(n, m, 192) for n in tst.TEXTS for m in tst.LENGTHS] + [("n4096", tst.EDGE_M, tst.EDGE_READS)]
AC_BATCHES = [("ac", m, 64) for m in tst.AC_LENGTHS]


def check_against_definition(K, oracle_mod, name, k, m, n_reads):
    f_steps = tst.auto_steps(K, name, k)
    tasks = tst.tasks(name, m, n_reads)
    steps = (m - m % k) // k
    for s in tst.SEEDS:
        iv, sp, skips = tst.reference(K, oracle_mod, name, k, m, s, n_reads)
        for ftab, skip in tst.TABLES.values():
            what = (name, k, m, s, ftab, skip)
            f = f_steps if ftab else 0
            mod = tst.seed_model(name, k, m, s, f, skip, n_reads)
            for got, want, part in ((mod["intervals"], iv, "intervals"), (mod["spans"], sp, "spans")):
                assert np.array_equal(got, want), (what, part, int(np.argwhere(got != want)[0][0]))
            assert np.array_equal(mod["lone_units"], skips), what
            assert np.array_equal(mod["records"], sr.counts(iv, sp)), what
            # every round moves the task: a K-step that ends a segment stays where it is and stores a record
            ends = mod["records"] - (sp[np.arange(tasks.shape[0]), np.maximum(mod["records"], 1) - 1, 0] == 0) * (mod["records"] > 0)
            walked = (0 if m % k else f) * mod["start_hits"] + (16 // k) * mod["skip_hits"] + mod["steps"] - ends
            done = (mod["records"] < s) | (sp[:, s - 1, 0] == 0)
            assert (walked[done] == steps).all() and (walked <= steps).all(), what
            assert (mod["skip_misses"] + mod["start_empty"] <= mod["records"] + mod["lone_units"] + 1).all(), what
            if not ftab or m % k:
                assert not mod["start_hits"].any() and not mod["start_empty"].any(), what
            if not skip:
                assert not mod["skip_hits"].any() and not mod["skip_misses"].any(), what


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name,m,n_reads", BATCHES + AC_BATCHES, ids=[f"{n}-m{m}" for n, m, _ in BATCHES + AC_BATCHES])
def test_model_is_the_definition(kfmi_mod, oracle_mod, name, m, n_reads, k):
    check_against_definition(kfmi_mod, oracle_mod, name, k, m, n_reads)


def strand_orders(mod, m):
    """The classes of a batch's model in the task order of each strand mode."""
    c = swm.classes(mod, m)
    return {st: {f: v[tst.rows_of(st)] for f, v in c.items()} for st in tst.STRANDS}


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", list(tst.TEXTS))
def test_no_batch_has_an_empty_class(kfmi_mod, name, k):
    """At m >= 100, with both tables: at least 16 tasks of every class in the
    task order of every strand mode."""
    f = tst.auto_steps(kfmi_mod, name, k)
    checked = 0
    for m in tst.LENGTHS:
        if m < 100:
            continue
        for st, c in strand_orders(tst.seed_model(name, k, m, 8, f, True), m).items():
            for cl in swm.LOOKUPS + ("three_records", "one_whole"):
                if m % k and cl in ("start_hit", "start_empty"):
                    continue                                     # the remainder table replaces the jump start
                assert int(c[cl].sum()) >= FLOOR, (name, k, m, st, cl, int(c[cl].sum()))
                checked += 1
    assert checked >= 4 * 3 * 4


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", list(tst.TEXTS))
def test_first_wave_shows_a_wrong_group(kfmi_mod, name, k):
    """Every 16-lane group of the first wave of every batch and task order holds
    a task of each lookup class, so a gather that one group never issues is
    visible; PERM_SEED is the first permutation seed for which this holds."""
    f = tst.auto_steps(kfmi_mod, name, k)
    missing = []
    for m in tst.LENGTHS:
        for st, c in strand_orders(tst.seed_model(name, k, m, 8, f, True), m).items():
            for cl in swm.LOOKUPS:
                if m % k and cl in ("start_hit", "start_empty"):
                    continue
                for g in range(4):
                    if not c[cl][16 * g:16 * g + 16].any():
                        missing.append((m, st, cl, "group", g))
    assert missing == [], (name, k, missing)


@pytest.mark.parametrize("k", [1, 2])
def test_the_ac_plan_has_lone_units(kfmi_mod, k):
    f = tst.auto_steps(kfmi_mod, "ac", k)
    assert f * k == 4
    for m in tst.AC_LENGTHS:
        for st, c in strand_orders(tst.seed_model("ac", k, m, 8, f, True, 64), m).items():
            assert int(c["lone_unit"].sum()) >= FLOOR, (k, m, st, int(c["lone_unit"].sum()))
    for name in tst.TEXTS:                                       # and nowhere else: these texts hold every unit
        assert not tst.seed_model(name, k, 100, 8, tst.auto_steps(kfmi_mod, name, k), True)["lone_units"].any()


def test_the_texts_have_six_base_tables(kfmi_mod):
    for name in tst.TEXTS:
        assert [tst.auto_steps(kfmi_mod, name, k) * k for k in (1, 2)] == [6, 6], name


# the table of test_fetch_forms.py's docstring: (K, d), layouts, class 1, class 2 8w, class 2 16w, class 4
FORM_TABLE = [((2, 64), ("task-mid", "task"), 8, 7, 7, 7),
              ((1, 128), ("task-mid", "task"), 8, 7, 7, 7),
              ((1, 64), ("task-mid", "task"), 1, 4, 1, 4),
              ((1, 32), ("task-mid",), 1, 4, 1, 4),
              ((2, 128), ("task-mid",), 1, 4, 1, 4),
              ((2, 192), ("task-mid",), 1, 1, 1, 1)]


def test_expected_form_is_the_table():
    from test_fetch_forms import GEOMETRIES
    seen = set()
    for (k, d), layouts, c1, c2w8, c2w16, c4 in FORM_TABLE:
        for lay in layouts:
            seen.add((lay, k, d))
            got = [swm.expected_form(lay, k, d, cls, mw) for cls, mw in ((1, 8), (1, 16), (2, 8), (2, 16), (4, 8), (4, 16))]
            assert got == [c1, c1, c2w8, c2w16, c4, c4], (lay, k, d, got)
            assert swm.expected_form(lay, k, d, 0, 8) == c1      # by size: a small index is class 1
    assert seen == set(GEOMETRIES)
    assert [swm.registers(k, m) for k, m in ((1, 128), (1, 129), (2, 129), (2, 130), (2, 256))] == [8, 16, 8, 16, 16]


def test_expected_launch():
    e = swm.expected_launch
    assert e("task-mid", 2, 64, 4, 100, sr.FWD, True, 3, True) == dict(form=7, maxw=8, kernel=swm.SEED_KERNEL, skip_split=4,
                                                                      ftab_folded=0, ftab_steps=3)
    assert e("task-mid", 2, 64, 0, 101, sr.FWD, True, 3, True)["ftab_steps"] == 0          # the remainder table
    assert e("task-mid", 2, 64, 0, 101, sr.FWD, True, 3, True, folded=True)["ftab_folded"] == 0
    assert e("task-mid", 2, 64, 0, 101, sr.BOTH, True, 3, True)["kernel"] == swm.SEED_WORDS_KERNEL
    assert e("task-mid", 2, 64, 0, 100, sr.BOTH, True, 3, False)["kernel"] == swm.SEED_STRANDS_KERNEL
    assert e("task", 1, 64, 2, 256, sr.REV, False, 6, True, seeds=False) == dict(
        form=1, maxw=16, kernel=swm.TASK_WORDS_SKIP_KERNEL, skip_split=2, ftab_folded=0, ftab_steps=6)
    assert e("task", 1, 64, 2, 100, sr.REV, True, 6, False, seeds=False, folded=True) == dict(
        form=4, maxw=8, kernel=swm.TASK_STRANDS_KERNEL, skip_split=1, ftab_folded=1, ftab_steps=6)
    assert e("task", 1, 64, 2, 100, sr.REV, False, 6, False, seeds=False) is None


def test_decoders(kfmi_mod):
    K = kfmi_mod
    rec = np.array([[7 | 3 << 16 | 1 << 24, 2 | 5 << 16, 4 | 8 << 16, 7 | 1 << 4 | 2 << 8 | 4 << 12 | 1 << 16 | 3 << 24],
                    [300, 0, 0, 1 | 2 << 4 | 4 << 8 | 1 << 12]], dtype=np.uint32)
    d = K.decode_seed_trace(rec)
    assert tuple(d) == K.SEED_TRACE_FIELDS == swm.FIELDS
    assert [d[f].tolist() for f in swm.FIELDS] == [[7, 300], [3, 0], [1, 0], [2, 0], [5, 0], [4, 0], [8, 0]]
    w = K.decode_launch_id(rec)
    assert tuple(w) == K.LAUNCH_ID_FIELDS
    assert [w[f].tolist() for f in K.LAUNCH_ID_FIELDS] == [[7, 1], [8, 16], [2, 4], [4, 1], [1, 0], [3, 0]]
    assert K.TRACE_KERNELS[swm.SEED_WORDS_KERNEL] == "seed_words_kernel"
    assert K.TRACE_KERNELS[swm.TASK_WORDS_SKIP_KERNEL] == "task_words_skip_kernel" and len(K.TRACE_KERNELS) == 5


def test_refusals_without_a_device(kfmi_mod):
    """Null arguments, handles of another size and handles that are not on a
    device are refused before anything runs, with the untraced calls' codes."""
    K = kfmi_mod
    L = K.load()
    q = K.Queries.from_array(tst.reads("n2513", 100)[:8])
    idx = K.Index.build(tst.TEXTS["n2513"][0].tobytes(), k=2, d=64)
    iv, sp, r, r9 = K.Results.alloc(4 * 16), K.Results.alloc(4 * 16), K.Results.alloc(16), K.Results.alloc(17)
    rec = np.full((16, 4), 0xABCD, dtype=np.uint32)
    out = rec.ctypes.data_as(ctypes.c_void_p)
    try:
        bad = L.kfmi_search_seeds_trace(idx.ptr, q.ptr, iv.ptr, sp.ptr, 4, sr.BOTH, None)
        assert bad == tst.BAD_ARGUMENT and b"argument" in L.errorCommon(bad).lower()
        assert L.kfmi_search_strands_trace(idx.ptr, q.ptr, r.ptr, sr.BOTH, None) == bad
        for args in ((None, q.ptr, iv.ptr, sp.ptr), (idx.ptr, None, iv.ptr, sp.ptr), (idx.ptr, q.ptr, None, sp.ptr),
                     (idx.ptr, q.ptr, iv.ptr, None), (idx.ptr, q.ptr, iv.ptr, iv.ptr), (idx.ptr, q.ptr, r9.ptr, sp.ptr)):
            assert L.kfmi_search_seeds_trace(*args, 4, sr.BOTH, out) == bad, args
        for s, st in ((0, sr.BOTH), (9, sr.BOTH), (4, 0), (4, 4), (4, sr.FWD)):      # FWD: 8 tasks, not these 16
            assert L.kfmi_search_seeds_trace(idx.ptr, q.ptr, iv.ptr, sp.ptr, s, st, out) == bad, (s, st)
        for args in ((None, q.ptr, r.ptr), (idx.ptr, None, r.ptr), (idx.ptr, q.ptr, None), (idx.ptr, q.ptr, r9.ptr)):
            assert L.kfmi_search_strands_trace(*args, sr.BOTH, out) == bad, args
        for st in (0, sr.FWD, 4):
            assert L.kfmi_search_strands_trace(idx.ptr, q.ptr, r.ptr, st, out) == bad, st
        off = L.kfmi_search_seeds_trace(idx.ptr, q.ptr, iv.ptr, sp.ptr, 4, sr.BOTH, out)     # nothing transferred
        assert off not in (0, bad) and b"device" in L.errorCommon(off).lower()
        assert L.kfmi_search_strands_trace(idx.ptr, q.ptr, r.ptr, sr.BOTH, out) == off
        assert (rec == 0xABCD).all()
    finally:
        for h in (q, iv, sp, r, r9, idx):
            h.close()
