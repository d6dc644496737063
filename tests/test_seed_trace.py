"""What every task of a seed or strand search took, lane by lane: the records
of kfmi_search_seeds_trace and kfmi_search_strands_trace (kstep_fmi.h) against
tests/seed_walk_model.py and tests/walk_model.py, field for field and without
tolerance -- the ordinary K-steps, the jump-start lookups that hit and that came
back empty, the skip lookups that matched and that did not, the units that did
not occur on their own, the records stored -- and word 3, the launch identity,
against seed_walk_model.expected_launch: the kernel, its fetch form and code
registers, skip_split, the folded bit and the jump start's step count.  The
traced intervals and spans are held to search_seeds_array's / search_array's,
to seed_ref.reference and the CPU oracle, bit for bit.

seed_walk and skip_walk use the two tables as shortcuts that check themselves:
a lookup that brings nothing, or never happens, leaves the lane on the K-steps
that end on the same records.  No test of results tells a lookup that fires
from one that never does, or a launch rule that picks another fetch form; these
tests do.  tests/test_seed_walk_model.py runs the same batches on the host,
vouches for the model against the definition and holds that every class of
tasks a batch is about has its tasks, so that no test here passes on an empty
class.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import seed_ref as sr
import seed_walk_model as swm
import test_jump_lines_search as tjl
import test_walk_trace as twt
import walk_model as wm
from skip_texts import ACGT
from strand_reads import revcomp_def
from test_fetch_forms import CLASSES, GEOMETRIES

CASES, IDS, TEXTS = twt.CASES, twt.IDS, twt.TEXTS
LENGTHS = (34, 100, 101, 129, 256)
FORM_LENGTHS = (100, 101, 256)
AC_LENGTHS = (100, 101)
SEEDS = (1, 8)
STRANDS = (sr.FWD, sr.REV, sr.BOTH)
EDGES = (1, 63, 64, 65, 257)
EDGE_READS, EDGE_M = 264, 100
PERM_SEED = 2          # the first seed under which test_seed_walk_model.test_first_wave_shows_a_wrong_group holds
# label -> (jump-start table, skip table)
TABLES = {"all": (True, True), "skip-off": (True, False), "ftab-off": (False, True), "all-off": (False, False)}
NOT_IMPLEMENTED, BAD_ARGUMENT = 19, 33


# ---- the batches and their models (host only) ------------------------------------------------------------------

def text_of(name):
    return sr.ac_text() if name == "ac" else TEXTS[name][0]


@lru_cache(maxsize=None)
def world(name):
    return wm.World(text_of(name))


@lru_cache(maxsize=None)
def reads(name, m, n_reads=192):
    """n_reads windows of the text in equal quarters with 0, 1, 2 and 3
    substituted bases, every second read reverse-complemented, under the pinned
    permutation.  "ac": seed_ref.ac_reads, whose G and T bytes make lone units."""
    if name == "ac":
        q = sr.ac_reads(sr.ac_text(), m, 4_000 + m)
    else:
        t = TEXTS[name][0]
        rng = np.random.default_rng(1_000 * sum(map(ord, name)) + m)
        g = n_reads // 4
        st = rng.integers(0, t.size - m + 1, size=n_reads)
        q = t[st[:, None] + np.arange(m)[None, :]].copy()
        for r in range(g, n_reads):
            cols = rng.permutation(m)[:r // g]
            q[r, cols] = ACGT[(np.searchsorted(ACGT, q[r, cols]) + rng.integers(1, 4, size=cols.size)) % 4]
        q[1::2] = revcomp_def(q[1::2])
        q = q[np.random.default_rng(PERM_SEED).permutation(n_reads)]
    q = np.ascontiguousarray(q)
    q.setflags(write=False)
    return q


@lru_cache(maxsize=None)
def tasks(name, m, n_reads=192):
    """The batch as BOTH runs it: read q on rows 2q (as written) and 2q + 1."""
    return sr.tasks_of(reads(name, m, n_reads), sr.BOTH)


def rows_of(strands, num=None):
    """The rows of tasks() a strand mode runs for the first num reads."""
    stop = None if num is None else 2 * num
    return {sr.FWD: slice(0, stop, 2), sr.REV: slice(1, stop, 2), sr.BOTH: slice(0, stop)}[strands]


@lru_cache(maxsize=None)
def seed_model(name, k, m, s, f_steps, skip, n_reads=192):
    return swm.play(world(name), k, tasks(name, m, n_reads), ftab_steps=f_steps, skip=skip, s=s)


@lru_cache(maxsize=None)
def strand_model(name, k, m, f_steps, skip, n_reads=192):
    return wm.play(world(name), k, tasks(name, m, n_reads), ftab_steps=f_steps, skip=skip, jump=False)


def auto_steps(K, name, k):
    """The auto jump-start table's K-steps for this text."""
    fb = K.ftab_auto_bases(text_of(name).size + 1, k, 1 << 40)
    assert fb % k == 0 and fb >= k
    return fb // k


_host = {}


def image(K, name, k):
    if ("img", name, k) not in _host:
        idx = K.Index.build(text_of(name).tobytes(), k=k, d=64)
        try:
            _host[("img", name, k)] = idx.image().copy()
        finally:
            idx.close()
    return _host[("img", name, k)]


def reference(K, oracle_mod, name, k, m, s, n_reads=192):
    """seed_ref.reference of the batch's BOTH tasks on the CPU oracle's K = 1 image."""
    key = ("ref", name, k, m, s, n_reads)
    if key not in _host:
        img = image(K, name, 1)
        _host[key] = sr.reference(lambda q: oracle_mod.search(img, q)[0], tasks(name, m, n_reads), k, s)
        for a in _host[key]:
            a.setflags(write=False)
    return _host[key]


def strand_oracle(K, oracle_mod, name, k, m, n_reads=192):
    key = ("walk", name, k, m, n_reads)
    if key not in _host:
        img = image(K, name, k if m % k == 0 else 1)
        _host[key] = np.asarray(oracle_mod.search(img, tasks(name, m, n_reads))[0], np.uint32).reshape(-1, 2).copy()
    return _host[key]


# ---- the GPU side ---------------------------------------------------------------------------------------------

def defaults(K):
    tjl._defaults(K)
    K.set_fused(True)
    K.set_ftab_budget(None)
    K.set_ftab_fold(1)
    K.set_ftab_fold_bound(None)


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    defaults(kfmi_mod)
    yield kfmi_mod
    defaults(kfmi_mod)


def fresh_upload(K, idx, backend):
    """The index on the device again under the settings in effect: its tables are built here."""
    K.set_backend(backend)
    idx.free_gpu()
    K.transfer_to_gpu(idx, None, None)


def set_tables(K, ftab, skip):
    K.set_ftab("auto" if ftab else 0)
    K.set_skip(("auto" if ftab else 1) if skip else 0)


def same_fields(dec, mod, fields, what):
    for f in fields:
        bad = np.flatnonzero(dec[f] != mod[f])
        assert bad.size == 0, (what, f, "tasks", int(bad.size), "first", int(bad[0]), "kernel", int(dec[f][bad[0]]),
                               "model", int(mod[f][bad[0]]), {g: int(dec[g][bad[0]]) for g in fields},
                               {g: int(mod[g][bad[0]]) for g in fields})


def same_launch(K, rec, want, what):
    got = K.decode_launch_id(rec)
    assert tuple(got) == K.LAUNCH_ID_FIELDS == tuple(want)
    for f, v in want.items():
        assert (got[f] == v).all(), (what, "word 3", f, "kernel", sorted(set(got[f].tolist())), "expected", v,
                                     None if f != "kernel" else K.TRACE_KERNELS[v])


def plan_of(K, geo, cls, m, strands, fused, skip, seeds):
    """The library's own launch plan of the traced call (kfmi_launch_plan, no
    device): class 0 is class 1 on these texts, and the one-shot calls upload
    ASCII rows."""
    backend, k, d = geo
    return K.launch_plan(backend, k, d, cls or 1, m, seeds=seeds, strands=strands, ascii=True, fused=fused, skip=skip,
                         traced=True)


def same_plan(K, rec, plan, what):
    """Word 3 as the device reports it is what the host plan says it launches."""
    got = K.decode_launch_id(rec)
    for f, v in (("form", plan["form"]), ("maxw", plan["maxw"] or plan["words_maxw"]), ("kernel", plan["kernel"])):
        assert (got[f] == v).all(), (what, "word 3 against kfmi_launch_plan", f, sorted(set(got[f].tolist())), "plan", plan)


def check_seeds(K, oracle_mod, idx, name, geo, cls, m, s, strands, fused, ftab, skip, folded, num=None, n_reads=192):
    """One seed search: records three ways, every field of every trace record, word 3."""
    backend, k, d = geo
    what = (name, geo, "class", cls, "m", m, "S", s, "strands", strands, "fused", fused, "ftab", ftab, "skip", skip, num)
    f_steps = auto_steps(K, name, k) if ftab else 0
    rows = rows_of(strands, num)
    mod = seed_model(name, k, m, s, f_steps, skip, n_reads)
    ref = reference(K, oracle_mod, name, k, m, s, n_reads)
    q = reads(name, m, n_reads)[:num]
    iv, sp, rec = K.search_seeds_trace(idx, q, backend, max_seeds=s, strands=strands)
    plain = K.search_seeds_array(idx, q, backend, max_seeds=s, strands=strands)
    for got, pl, rf, md, part in ((iv, plain[0], ref[0], mod["intervals"], "intervals"), (sp, plain[1], ref[1], mod["spans"], "spans")):
        for other, label in ((pl, "search_seeds_array"), (rf[rows], "reference"), (md[rows], "model")):
            assert got.shape == other.shape, (what, part, label, got.shape, other.shape)
            assert np.array_equal(got, other), (what, part, "trace != " + label, int(np.argwhere(got != other)[0][0]))
    dec = K.decode_seed_trace(rec)
    assert tuple(dec) == swm.FIELDS == K.SEED_TRACE_FIELDS
    same_fields(dec, {f: mod[f][rows] for f in swm.FIELDS}, swm.FIELDS, what)
    same_launch(K, rec, swm.expected_launch(backend, k, d, cls, m, strands, fused, f_steps, skip, True, folded), what)
    same_plan(K, rec, plan_of(K, geo, cls, m, strands, fused, skip, True), what)


STRAND_FIELDS = ("steps", "skip_hits", "skip_misses", "start_steps")


def check_strands(K, oracle_mod, idx, name, geo, cls, m, strands, fused, ftab, skip, folded, num=None, n_reads=192):
    """One strand search: intervals three ways, words 0 .. 2 against walk_model, word 3."""
    backend, k, d = geo
    what = (name, geo, "class", cls, "m", m, "strands", strands, "fused", fused, "ftab", ftab, "skip", skip, num)
    f_steps = auto_steps(K, name, k) if ftab else 0
    rows = rows_of(strands, num)
    want = swm.expected_launch(backend, k, d, cls, m, strands, fused, f_steps, skip, False, folded)
    q = reads(name, m, n_reads)[:num]
    if want is None:                                             # the plain walk of packed words: no traced form
        with pytest.raises(K.KfmiError) as e:
            K.search_strands_trace(idx, q, backend, strands)
        assert e.value.code == NOT_IMPLEMENTED, what
        with pytest.raises(K.KfmiError) as e:                    # and the host plan refuses what the call refused
            plan_of(K, geo, cls, m, strands, fused, skip, False)
        assert e.value.code == NOT_IMPLEMENTED, what
        return
    mod = strand_model(name, k, m, f_steps, skip, n_reads)
    got, rec = K.search_strands_trace(idx, q, backend, strands)
    plain = K.search_array(idx, q, backend, strands=strands)
    oracle = strand_oracle(K, oracle_mod, name, k, m, n_reads)[rows].reshape(-1)
    model = np.stack([mod["L"], mod["R"]], axis=1)[rows].reshape(-1)
    for other, label in ((plain, "search_array"), (oracle, "oracle"), (model, "model")):
        assert got.shape == other.shape, (what, label)
        assert np.array_equal(got, other), (what, "trace != " + label, int(np.flatnonzero(got != other)[0]) // 2)
    dec = K.decode_trace(rec)
    same_fields(dec, {f: mod[f][rows] for f in STRAND_FIELDS}, STRAND_FIELDS, what)
    assert (rec[:, 1] == 0).all() and (rec[:, 2] >> 31 == 0).all(), (what, "a strand search never takes the text jump")
    same_launch(K, rec, want, what)
    same_plan(K, rec, plan_of(K, geo, cls, m, strands, fused, skip, False), what)


def check_all(K, oracle_mod, idx, name, geo, cls, lengths, fused, ftab, skip, folded):
    for m in lengths:
        for st in STRANDS:
            for s in SEEDS:
                check_seeds(K, oracle_mod, idx, name, geo, cls, m, s, st, fused, ftab, skip, folded)
            if st != sr.FWD:
                check_strands(K, oracle_mod, idx, name, geo, cls, m, st, fused, ftab, skip, folded)


PARAMS = [(n, b, k, d) for n in TEXTS for b, k, d in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,backend,k,d", PARAMS, ids=[f"{n}-{b}-k{k}d{d}" for n, b, k, d in PARAMS])
def test_tables(gpu, oracle_mod, name, backend, k, d):
    """Class 0, every length, S, strand mode and table setting on an upload
    whose jump-start table is folded, then the settings with a jump-start table
    on an upload whose table is not: the same counts either way, and the folded
    bit of word 3 says which."""
    K = gpu
    idx = K.Index.build(TEXTS[name][0].tobytes(), k=k, d=d)
    try:
        for fold in (1, 0):
            defaults(K)
            K.set_ftab_fold(fold)
            fresh_upload(K, idx, backend)
            folded = idx.ftab_entries()[1]
            assert folded == bool(fold), (name, fold)
            for label, (ftab, skip) in TABLES.items():
                if not fold and not ftab:
                    continue                                     # no jump-start table: nothing the fold changes
                set_tables(K, ftab, skip)
                check_all(K, oracle_mod, idx, name, (backend, k, d), 0, LENGTHS, True, ftab, skip, folded)
                assert (idx.skip_bytes() != 0) if skip else True, label
                assert (idx.ftab_bytes() != 0) if ftab else True, label
    finally:
        defaults(K)
        idx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", GEOMETRIES, ids=["%s-k%d-d%d" % g for g in GEOMETRIES])
@pytest.mark.parametrize("cls", CLASSES, ids=["class%d" % c for c in CLASSES])
def test_classes_and_forms(gpu, oracle_mod, cls, backend, k, d):
    """One upload under the class (its tables are built under it), then the
    fused kernels and, with fused packing off, the words kernels: every record
    against the model, and word 3 against the form table."""
    K = gpu
    name = "n3021"
    idx = K.Index.build(TEXTS[name][0].tobytes(), k=k, d=d)
    try:
        defaults(K)
        K.set_split_class(cls)
        fresh_upload(K, idx, backend)
        folded = idx.ftab_entries()[1]
        for fused in (True, False):
            K.set_fused(fused)
            check_all(K, oracle_mod, idx, name, (backend, k, d), cls, FORM_LENGTHS, fused, True, True, folded)
        assert idx.skip_bytes() != 0 and idx.ftab_bytes() != 0   # an absent table must not pass silently
        K.set_skip(0)                                            # packs first, no skip table: refused, nothing written
        check_strands(K, oracle_mod, idx, name, (backend, k, d), cls, 100, sr.BOTH, False, True, False, folded)
    finally:
        defaults(K)
        idx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_lone_units(gpu, oracle_mod, k):
    """The A / C text: units with a G or a T do not occur on their own, at odd
    m and K = 2 the remainder unit among them."""
    K = gpu
    geo = ("task-mid", k, 64)
    idx = K.Index.build(sr.ac_text().tobytes(), k=k, d=64)
    try:
        defaults(K)
        fresh_upload(K, idx, geo[0])
        folded = idx.ftab_entries()[1]
        for ftab, skip in (TABLES["all"], TABLES["all-off"]):
            set_tables(K, ftab, skip)
            for m in AC_LENGTHS:
                for st in STRANDS:
                    for s in SEEDS:
                        check_seeds(K, oracle_mod, idx, "ac", geo, 0, m, s, st, True, ftab, skip, folded, n_reads=64)
    finally:
        defaults(K)
        idx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", [("task-mid", 2, 64), ("task", 1, 64)])
def test_batch_edges(gpu, oracle_mod, backend, k, d):
    """Batches of 1, 63, 64, 65 and 257 tasks: FWD and REV run one task per read."""
    K = gpu
    name = "n4096"
    idx = K.Index.build(TEXTS[name][0].tobytes(), k=k, d=d)
    try:
        defaults(K)
        fresh_upload(K, idx, backend)
        folded = idx.ftab_entries()[1]
        for num in EDGES:
            for st in (sr.FWD, sr.REV):
                check_seeds(K, oracle_mod, idx, name, (backend, k, d), 0, EDGE_M, 8, st, True, True, True, folded, num,
                            EDGE_READS)
            check_strands(K, oracle_mod, idx, name, (backend, k, d), 0, EDGE_M, sr.REV, True, True, True, folded, num,
                          EDGE_READS)
    finally:
        defaults(K)
        idx.close()


class Handles:
    """Resident handles of one seed search and one strand search, results filled with a pattern."""
    FILL = 0xA5A5A5A5

    def __init__(self, K, idx, q, s, strands, fill=True):
        self.K, self.idx, self.s, self.strands = K, idx, s, strands
        n = (2 if strands == sr.BOTH else 1) * q.shape[0]
        self.q = K.Queries.from_array(q)
        self.iv, self.sp, self.r = K.Results.alloc(s * n), K.Results.alloc(s * n), K.Results.alloc(n)
        K.transfer_to_gpu(idx, self.q, self.iv)
        K.transfer_to_gpu(idx, None, self.sp)
        K.transfer_to_gpu(idx, None, self.r)
        for h in (self.iv, self.sp, self.r) if fill else ():
            h.array()[:] = self.FILL
            K.results_to_gpu(h)
        self.rec = np.full((n, 4), 0xABCD, dtype=np.uint32)

    def seeds(self, trace=True, intervals=None):
        out = self.rec.ctypes.data_as(ctypes.c_void_p) if trace else None
        return self.K.load().kfmi_search_seeds_trace(self.idx.ptr, self.q.ptr, (intervals or self.iv).ptr, self.sp.ptr,
                                                     self.s, self.strands, out)

    def walk(self, trace=True, results=None):
        out = self.rec.ctypes.data_as(ctypes.c_void_p) if trace else None
        return self.K.load().kfmi_search_strands_trace(self.idx.ptr, self.q.ptr, (results or self.r).ptr, self.strands, out)

    def untouched(self):
        for h in (self.iv, self.sp, self.r):
            self.K.transfer_to_cpu(h)
            if not (h.array() == self.FILL).all():
                return False
        return bool((self.rec == 0xABCD).all())

    def close(self):
        for h in (self.q, self.iv, self.sp, self.r):
            h.close()


@pytest.mark.gpu
def test_refusals_on_the_device(gpu, oracle_mod):
    """What has no traced kernel, and what the untraced calls refuse, is refused
    with their codes before anything is written: the trace array and the
    results handles keep their fill, and the handles still serve afterwards."""
    K = gpu
    name, m = "n3021", 100
    t = TEXTS[name][0]
    q = reads(name, m)[:40]
    idx = K.Index.build(t.tobytes(), k=2, d=64)
    i4 = K.Index.build(t.tobytes(), k=4, d=64)
    try:
        defaults(K)
        for backend in ("coop", "coop-mid", "task-ac", "task-ac-mid"):
            fresh_upload(K, idx, backend)
            h = Handles(K, idx, q, 4, sr.BOTH)
            try:
                assert h.seeds() == NOT_IMPLEMENTED and h.walk() == NOT_IMPLEMENTED, backend
                assert h.untouched(), backend
            finally:
                h.close()
        fresh_upload(K, i4, "task-grp")
        h = Handles(K, i4, q, 4, sr.BOTH)
        try:
            assert h.seeds() == NOT_IMPLEMENTED and h.walk() == NOT_IMPLEMENTED
            assert h.untouched()
        finally:
            h.close()
        K.set_devices([0, 0])
        fresh_upload(K, idx, "task-mid")
        h = Handles(K, idx, q, 4, sr.BOTH, fill=False)       # group handles take no fill from the host
        try:
            assert h.seeds() == NOT_IMPLEMENTED and h.walk() == NOT_IMPLEMENTED
            assert (h.rec == 0xABCD).all()
        finally:
            h.close()
        K.set_devices([])
        fresh_upload(K, idx, "task-mid")
        long_reads = np.ascontiguousarray(t[np.arange(8)[:, None] + np.arange(300)[None, :]])
        h = Handles(K, idx, long_reads, 4, sr.BOTH)
        try:
            assert h.seeds() == BAD_ARGUMENT              # kfmi_search_seeds' own answer to reads over 256 bases
            assert h.walk() == NOT_IMPLEMENTED            # the strand search walks them; no traced kernel does
            assert h.untouched()
        finally:
            h.close()
        h = Handles(K, idx, q, 4, sr.BOTH)
        other = K.Results.alloc(4 * 2 * q.shape[0] + 1)
        try:
            K.transfer_to_gpu(idx, None, other)
            assert h.seeds(trace=False) == BAD_ARGUMENT and h.walk(trace=False) == BAD_ARGUMENT      # a null trace
            assert h.seeds(intervals=other) == BAD_ARGUMENT and h.walk(results=other) == BAD_ARGUMENT   # another size
            h.strands = sr.FWD
            assert h.walk() == BAD_ARGUMENT               # FWD is kfmi_search_trace
            h.strands = sr.BOTH
            assert h.untouched()
            assert h.seeds() == 0 and h.walk() == 0       # and the handles still serve
            assert not (h.rec == 0xABCD).any()
        finally:
            other.close()
            h.close()
        check_seeds(K, oracle_mod, idx, name, ("task-mid", 2, 64), 0, m, 8, sr.BOTH, True, True, True, idx.ftab_entries()[1])
        check_strands(K, oracle_mod, idx, name, ("task-mid", 2, 64), 0, m, sr.BOTH, True, True, True, idx.ftab_entries()[1])
    finally:
        K.set_devices([])
        defaults(K)
        idx.close()
        i4.close()
