"""The seed, strand and verify kernels in every fetch form and table-size class.

split_for() answers class 4 for every table of a 3 Gbase index, so the searches
the bench runs get the large-table forms: the asm fetch in two 32-lane groups
(form 7), the C++ fetch in four exec-masked 16-lane groups (form 4), the jump-
start and skip gathers group by group (ix.skip_split == 4) and verify_kernel's
split4 branch.  The other tests of these kernels run on 20 k-base texts at class
0, which resolves to class 1.  Here kfmi_set_split_class puts a small index into
each class, as test_gpu_parity.py::test_split_gathers_equal_oracle does for the
forward search, and the results are held to the same references as at class 1:
seed_ref.reference on the CPU oracle's K = 1 image for the seed records, the
CPU oracle for the strand intervals, verify_ref's model for the hits.  No
search function of the library is a reference.

The form launch_seeds (seed_kernel, seed_strands_kernel, seed_words_kernel) and
launch_task (task_strands_kernel; task_words_skip_kernel where a strand search
packs first and a skip table is in effect) pick, read from kfmi_kernels.h.
8 / 7 = the asm fetch in one / two groups, 4 / 1 = the C++ fetch in four groups
/ one; "8w" and "16w" are the 8- and 16-word kernels:

    (K, d)    layouts          class 1   class 2 8w   class 2 16w   class 4
    (2, 64)   task-mid, task      8          7             7           7
    (1, 128)  task-mid, task      8          7             7           7
    (1, 64)   task-mid, task      1          4             1           4
    (1, 32)   task-mid            1          4             1           4
    (2, 128)  task-mid            1          4             1           4
    (2, 192)  task-mid            1          1             1           1

seed_walk_model.expected_form is this table as a function, and
tests/test_seed_trace.py holds the form of every traced launch to it.
(2, 192) is not SMALL: its walk is lf_stream whatever the form.  A strand search
that packs first without a skip table (set_fused(False) under set_skip(0)) runs
task_kernel<G, 1, 0, SPLIT>, which launch_task sends to form 1 at class 2 on the
non-asm geometries.  On "task" every geometry above is NEIGHBOR: the forms carry
block b - 1's planes too.  The table gathers of seed_walk and skip_walk go out
in four groups at class 4 only, and so does verify_kernel's split4 branch.

Lengths 34, 100, 101: 8 words; 256: 16 words; 129: 16 words at K = 1, 8 words
at K = 2 (128 bases in K-steps and the remainder table).

The batch of each length is seed_ref.main_reads' 196 reads under one pinned
permutation; test_first_wave_can_show_a_wrong_group asserts on the reference
alone that every lane group of the first wave holds what shows a wrong group."""
import numpy as np
import pytest

import seed_ref as sr
import test_seeds_gpu as tsg
import test_verify_gpu as tvg
import verify_ref as vr
from test_verify_host import handmade, host_hits

CLASSES = (1, 2, 4)
GEOMETRIES = [("task-mid", 2, 64), ("task-mid", 1, 128), ("task-mid", 1, 64), ("task-mid", 1, 32), ("task-mid", 2, 128),
              ("task-mid", 2, 192), ("task", 2, 64), ("task", 1, 128), ("task", 1, 64)]
D_MAX = 192
LENGTHS = (34, 100, 101, 129, 256)
PREFIXES = (1, 31, 33, 65)
SEEDS = (1, 8)
STRANDS = (sr.FWD, sr.REV, sr.BOTH)
PERM_SEED = 0          # the first seed under which test_first_wave_can_show_a_wrong_group holds
VERIFY_LENGTHS = (100, 101, 128, 129, 256)
VERIFY_PREFIXES = (1, 63, 65, 257)


def shuffled(t, m, perm_seed=PERM_SEED):
    """main_reads' batch of one length under the permutation: unshuffled, its
    first three 16-lane groups are unchanged reads, which never diverge."""
    q = sr.main_reads(t, m, 9_000 + m, n_reads=192)
    return np.ascontiguousarray(q[np.random.default_rng(perm_seed).permutation(q.shape[0])])


_batches = {}


def batches(K, oracle_mod):
    """Per length: the 196 shuffled reads, the seed records of BOTH at S = 8 per
    K (seed_ref.reference on the oracle's K = 1 image) and the oracle's interval
    of every task of BOTH per K (the K image when m % K == 0, else the K = 1
    image).  Once per session; they depend on neither d nor the layout."""
    if _batches:
        return _batches
    t = sr.main_text()
    idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
    try:
        img = {k: idx[k].image().copy() for k in (1, 2)}
    finally:
        for i in idx.values():
            i.close()
    search = lambda q: oracle_mod.search(img[1], q)[0]   # noqa: E731
    cases = {}
    for m in LENGTHS:
        q = shuffled(t, m)
        both = sr.tasks_of(q, sr.BOTH)
        ref = {k: sr.reference(search, both, k, 8) for k in (1, 2)}
        walk = {k: np.asarray(oracle_mod.search(img[k if m % k == 0 else 1], both)[0], np.uint32).reshape(-1, 2).copy()
                for k in (1, 2)}
        for a in [q] + [x for k in (1, 2) for x in ref[k]] + list(walk.values()):
            a.setflags(write=False)
        cases[m] = (q, ref, walk)
    _batches.update(text=t, cases=cases)
    return _batches


def wave_shows_a_wrong_group(m, iv, sp):
    """What is missing from the first wave of one task order (iv, sp: the
    records of its tasks at S = 8); an empty list when every group can show a
    wrong fetch or gather."""
    iv, sp = iv[:64].astype(np.int64), sp[:64].astype(np.int64)
    assert iv.shape[0] == 64
    c = sr.counts(iv, sp)
    whole = (c == 1) & (sp[:, 0, 0] == 0) & (sp[:, 0, 1] == m)
    rec = sp[:, :, 1] > 0
    width = iv[:, :, 1] - iv[:, :, 0]
    wide = (rec & (width > D_MAX)).any(axis=1)
    row1 = (rec & (width == 1)).any(axis=1)
    missing = []
    for g in range(4):
        lanes = slice(16 * g, 16 * g + 16)
        if not whole[lanes].any():
            missing.append(("group", g, "no task with one full-length record"))
        if not (c[lanes] >= 3).any():      # restarts mid-walk: partial exec at the fetch
            missing.append(("group", g, "no task with three or more records"))
    for h in range(2):
        lanes = slice(32 * h, 32 * h + 32)
        if not wide[lanes].any():          # L and R in different blocks at every d tested
            missing.append(("half", h, "no record with R - L > %d" % D_MAX))
        if not row1[lanes].any():
            missing.append(("half", h, "no record with R - L == 1"))
    return missing


def test_first_wave_can_show_a_wrong_group(kfmi_mod, oracle_mod):
    """On the reference alone, for every K, every length >= 100 and the task
    orders of FWD and BOTH: each 16-lane group of the whole batch's first wave
    holds a task with exactly one full-length record and a task with three or
    more records, each 32-lane half a record with R - L > 192 and one with
    R - L == 1."""
    b = batches(kfmi_mod, oracle_mod)
    checked = 0
    for m in LENGTHS:
        if m < 100:
            continue
        q, ref, _ = b["cases"][m]
        assert q.shape[0] == 196
        for k in (1, 2):
            for order in (sr.FWD, sr.BOTH):
                assert wave_shows_a_wrong_group(m, *tsg.cut(ref[k], order, 8)) == [], (k, m, order)
                checked += 1
    assert checked == 16


@pytest.fixture(scope="module")
def device(kfmi_mod, oracle_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    b = batches(K, oracle_mod)
    K.set_device(0)
    tvg.defaults(K)
    yield K, b
    tvg.defaults(K)


def interval_rows(walk, strands, num):
    """The flat intervals search_array returns for the first num reads."""
    rows = {sr.REV: walk[1::2], sr.BOTH: walk}[strands]
    return rows[:num * (2 if strands == sr.BOTH else 1)].reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", GEOMETRIES, ids=["%s-k%d-d%d" % g for g in GEOMETRIES])
@pytest.mark.parametrize("cls", CLASSES, ids=["class%d" % c for c in CLASSES])
def test_seed_and_strand_searches(device, cls, backend, k, d):
    """One upload under the class (its tables are built under it), then every
    length, batch prefix, staging and strand mode, with the auto tables and
    with every K-step through the fetch form."""
    K, b = device
    idx = K.Index.build(b["text"].tobytes(), k=k, d=d)
    try:
        tvg.defaults(K)
        K.set_split_class(cls)
        tsg.fresh_upload(K, idx, backend)
        for tables in ("auto", "walk"):
            K.set_ftab("auto" if tables == "auto" else 0)
            K.set_skip("auto" if tables == "auto" else 0)
            for fused in (True, False):
                K.set_fused(fused)
                for m, (q, ref, walk) in b["cases"].items():
                    for num in (q.shape[0],) + PREFIXES:
                        part = np.ascontiguousarray(q[:num])
                        what = (cls, backend, k, d, tables, fused, m, num)
                        for s in SEEDS:
                            for st in STRANDS:
                                tsg.same(K.search_seeds_array(idx, part, backend, max_seeds=s, strands=st),
                                         tsg.cut(ref[k], st, s, num), what + ("seeds", s, st))
                        for st in (sr.REV, sr.BOTH):
                            got = K.search_array(idx, part, backend, strands=st)
                            want = interval_rows(walk[k], st, num)
                            assert got.shape == want.shape, what + ("strands", st)
                            assert np.array_equal(got, want), what + ("strands", st, "first differing task",
                                                                       int(np.flatnonzero(got != want)[0]) // 2)
            if tables == "auto":
                assert idx.skip_bytes() != 0 and idx.ftab_bytes() != 0   # an absent table must not pass silently
    finally:
        tvg.defaults(K)
        idx.close()


@pytest.fixture(scope="module")
def verify_world(device, oracle_mod):
    """verify_ref.world's main text with its model, and indexes of this file's
    own: an upload under class 4 must not stay on the indexes other files share."""
    K, _ = device
    x = vr.world(K, oracle_mod)["main"]
    idx = {k: K.Index.build(x["text"].tobytes(), k=k, d=64) for k in (1, 2)}
    yield K, x, idx
    tvg.defaults(K)
    for i in idx.values():
        i.close()


def verify_lengths(K, x, idx, k, cls, what):
    for m in VERIFY_LENGTHS:
        q, _, per_k = x["cases"][m]
        c = per_k[k][2]
        for st in vr.STRANDS:
            rows = vr.strand_rows(st)
            d = tvg.Device(K, idx, q, 4, st)
            try:
                d.seeds()
                for occ in (1, 8):
                    for mm in vr.mism_bounds(m):
                        tvg.same(d.verify(occ, mm), vr.records(c, 4, occ, mm, rows), (what, "class", cls, m, st, occ, mm))
            finally:
                d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k", [("task-mid", 1), ("task-mid", 2), ("task", 2)])
def test_verify_class_4(verify_world, backend, k):
    """verify_kernel's split4 branch (and the seed search under class 4 that
    feeds it): lengths on both sides of 128, every strand mode, max_occ 1 and 8,
    then the same cases at class 1 on the same upload, so that a difference
    points at the branch; batch prefixes on a hits handle filled with
    0xA5A5A5A5."""
    K, x, idxs = verify_world
    idx = idxs[k]
    try:
        tvg.defaults(K)
        K.set_split_class(4)
        tvg.fresh_upload(K, idx, backend)
        verify_lengths(K, x, idx, k, 4, backend)
        assert idx.jump_bytes() != 0
        q, _, per_k = x["cases"][101]
        c = per_k[k][2]
        assert q.shape[0] >= max(VERIFY_PREFIXES)
        for num in VERIFY_PREFIXES:
            part = np.ascontiguousarray(q[:num])
            for st in vr.STRANDS:
                T = (2 if st == sr.BOTH else 1) * num
                d = tvg.Device(K, idx, part, 4, st)
                try:
                    assert d.filled == tvg.FILL
                    d.seeds()
                    tvg.same(d.verify(8, 3), vr.records(c, 4, 8, 3, vr.strand_rows(st))[:T], (backend, "prefix", num, st))
                finally:
                    d.close()
        K.set_split_class(1)
        verify_lengths(K, x, idx, k, 1, backend)
    finally:
        tvg.defaults(K)
        idx.free_gpu()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_verify_class_4_hand_made_handles(verify_world, k):
    """Slots filled on the host and transferred, at max_occ = 256: the whole
    array cut by max_occ, every ignored-slot form, R > rows, garbage."""
    K, x, idxs = verify_world
    idx = idxs[k]
    q, iv, sp = handmade(x["world"])
    c = vr.candidates(x["world"], q, iv, sp, 256)
    assert (c.why == vr.SCORED).any() and (c.why != vr.SCORED).any()
    try:
        tvg.defaults(K)
        K.set_split_class(4)
        tvg.fresh_upload(K, idx, "task-mid")
        d = tvg.Device(K, idx, q, 8, sr.FWD)
        try:
            d.iv.array()[:] = iv.reshape(-1)
            d.sp.array()[:] = sp.reshape(-1)
            K.results_to_gpu(d.iv)
            K.results_to_gpu(d.sp)
            for mm in (0, 40, 0xFFFFFFFF):
                got = d.verify(256, mm)
                tvg.same(got, vr.records(c, 8, 256, mm), ("hand-made", k, mm))
                tvg.same(got, host_hits(K, x["world"], q, iv, sp, 8, sr.FWD, 256, mm), ("hand-made, host form", k, mm))
            assert (d.verify(256, 40)[:, 1] >> vr.SCORED_SHIFT).max() > 200
        finally:
            d.close()
    finally:
        tvg.defaults(K)
        idx.free_gpu()


@pytest.mark.gpu
def test_map_reads_class_4(verify_world):
    """Upload, seed search and verify in one call under class 4, against the
    model and, as a cross-check, against the same call on the host."""
    K, x, idxs = verify_world
    idx = idxs[2]
    q, _, per_k = x["cases"][101]
    try:
        tvg.defaults(K)
        K.set_split_class(4)
        tvg.fresh_upload(K, idx, "task-mid")
        got = K.map_reads_array(idx, q, "task-mid", max_seeds=4, max_occ=8, max_mism=3)
        model = K.decode_hits(vr.records(per_k[2][2], 4, 8, 3))
        want = K.map_reads_array(idx, q, max_seeds=4, max_occ=8, max_mism=3, cpu=True, text=x["text"])
        for g, mo, h, name in zip(got, model, want, ("origin", "mism", "multi", "scored")):
            assert np.array_equal(g, mo), (name, "model")
            assert np.array_equal(g, h), (name, "host")
        assert (got[0] >= 0).any() and (got[0] < 0).any() and got[2].any()
    finally:
        tvg.defaults(K)
        idx.free_gpu()
