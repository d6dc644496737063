"""Seed search on the device (kfmi_search_seeds): every staging and walk path
against the restatement of the definition in seed_ref.py -- the CPU oracle on
the K = 1 image for substring intervals, revcomp_def for the reverse strand,
no search function of the library.  Every comparison is bit-exact on both
arrays, unused slots included.

The reference is computed once per (text, K, length), for both strands at
S = 8: the tasks of FWD and REV are the even and odd rows of BOTH, and fewer
slots keep a prefix of the records (test_seeds_host.py asserts that of the
restatement at every S)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import seed_ref as sr
import util
from strand_reads import code_of

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 34, 48, 64, 99, 100, 101, 127, 128, 129, 130, 255, 256)
SEEDS = (1, 3, 8)
STRANDS = (sr.FWD, sr.REV, sr.BOTH)
EDGE_LENGTHS = (100, 101, 129)
EDGE_SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)
PACKED_LENGTHS = (33, 100, 101, 256)
FILL = 0xA5A5A5A5


def defaults(K):
    K.set_devices([])
    K.set_split_class(0)
    K.set_fused(True)
    K.set_ftab_budget(None)
    K.set_skip("auto")
    K.set_ftab("auto")


def cut(ref, strands, s, num=None):
    """(intervals, spans) of a strand mode and S from the reference of BOTH at S = 8."""
    rows = {sr.FWD: slice(0, None, 2), sr.REV: slice(1, None, 2), sr.BOTH: slice(None)}[strands]
    iv, sp = ref[0][rows, :s], ref[1][rows, :s]
    if num is not None:
        iv, sp = iv[:num * (2 if strands == sr.BOTH else 1)], sp[:num * (2 if strands == sr.BOTH else 1)]
    return iv, sp


def same(got, want, what):
    for g, w, name in zip(got, want, ("intervals", "spans")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, "first differing task", int(np.argwhere(g != w)[0][0]))


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    """The two texts, their K = 1, 2 indexes, the reads of every length and the
    reference of their tasks; the non-vacuity conditions are asserted here, on
    the reference alone, before any seed search runs."""
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    K.set_device(0)
    defaults(K)
    out = {}
    for name, t, reads in (("main", sr.main_text(), lambda t, m: sr.main_reads(t, m, 3_000 + m)),
                           ("ac", sr.ac_text(), lambda t, m: sr.ac_reads(t, m, 4_000 + m))):
        idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
        img1 = idx[1].image()
        search = lambda q, img1=img1: oracle_mod.search(img1, q)[0]   # noqa: E731
        cases = {}
        for m in LENGTHS:
            q = reads(t, m)
            both = sr.tasks_of(q, sr.BOTH)
            ref = {k: sr.reference(search, both, k, 8) for k in (1, 2)}
            for k in (1, 2):
                if name == "main" and m >= 48:
                    ref2 = sr.reference(search, both, k, 2)
                    for rows, strand in ((slice(0, None, 2), "fwd"), (slice(1, None, 2), "rev")):
                        sr.assert_main_not_vacuous(m, tuple(a[rows] for a in ref[k]), tuple(a[rows] for a in ref2),
                                                   (k, m, strand))
                if name == "ac" and m >= 15:
                    sr.assert_ac_not_vacuous(tuple(a[0::2] for a in ref[k]), 8, (k, m))
                for a in ref[k]:
                    a.setflags(write=False)
            q.setflags(write=False)
            cases[m] = (q, ref)
        out[name] = dict(text=t, idx=idx, cases=cases, search=search)
    yield K, out
    defaults(K)
    for w in out.values():
        for i in w["idx"].values():
            i.close()


def fresh_upload(K, idx, backend):
    """The index on the device again under the settings in effect: its tables are built here."""
    K.set_backend(backend)
    idx.free_gpu()
    K.transfer_to_gpu(idx, None, None)


def check_lengths(K, idx, backend, cases, k, what, seeds=SEEDS, strands=STRANDS):
    for m, (q, ref) in cases.items():
        for s in seeds:
            for st in strands:
                same(K.search_seeds_array(idx, q, backend, max_seeds=s, strands=st), cut(ref[k], st, s), (what, m, s, st))


@pytest.mark.parametrize("tables", ["auto", "walk"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "packed-first"])
@pytest.mark.parametrize("k", [1, 2])
def test_task_mid_every_length(world, k, fused, tables):
    """task-mid at K = 1, 2.  Fused: seed_kernel (FWD, any m % K) and
    seed_strands_kernel (REV / BOTH, m % K == 0) in their 8- and 16-word forms,
    seed_words_kernel behind the strand pack for REV / BOTH at odd m, K = 2.
    Not fused: seed_words_kernel behind the forward or the strand pack.  auto:
    the jump-start and skip tables built at upload, taken by every new segment;
    walk: every K-step."""
    K, w = world
    idx = w["main"]["idx"][k]
    try:
        defaults(K)
        fresh_upload(K, idx, "task-mid")
        K.set_fused(fused)
        if tables == "walk":
            K.set_ftab(0)
            K.set_skip(0)
        check_lengths(K, idx, "task-mid", w["main"]["cases"], k, ("task-mid", k, fused, tables))
        if tables == "auto":
            assert idx.skip_bytes() != 0              # the auto tables are on the device
            assert idx.ftab_bytes() != 0
    finally:
        defaults(K)


def test_task_backend_defaults(world):
    """The reference's own layout (tag 101): the "task" backend at K = 2."""
    K, w = world
    try:
        defaults(K)
        fresh_upload(K, w["main"]["idx"][2], "task")
        check_lengths(K, w["main"]["idx"][2], "task", w["main"]["cases"], 2, "task", seeds=(3,))
    finally:
        defaults(K)


@pytest.mark.parametrize("tables", ["auto", "walk"])
@pytest.mark.parametrize("k", [1, 2])
def test_units_that_do_not_occur(world, k, tables):
    """The A / C text: reads with G / T bytes, so units that do not occur on
    their own (no record, the walk goes on past them), an empty remainder entry
    at odd m and K = 2, empty jump-start entries, and on the reverse strand
    tasks without any record."""
    K, w = world
    idx = w["ac"]["idx"][k]
    try:
        defaults(K)
        fresh_upload(K, idx, "task-mid")
        if tables == "walk":
            K.set_ftab(0)
            K.set_skip(0)
        check_lengths(K, idx, "task-mid", w["ac"]["cases"], k, ("ac", k, tables), seeds=(1, 8))
    finally:
        defaults(K)


@pytest.fixture(scope="module")
def edges(world):
    """One shuffled batch of 513 reads per edge length with its reference; every
    smaller batch is a prefix of it."""
    _, w = world
    t, search = w["main"]["text"], w["main"]["search"]
    out = {}
    for m in EDGE_LENGTHS:
        q = sr.main_reads(t, m, 6_000 + m, n_reads=512)
        q = np.ascontiguousarray(q[np.random.default_rng(m).permutation(q.shape[0])[:513]])
        both = sr.tasks_of(q, sr.BOTH)
        ref = {k: sr.reference(search, both, k, 8) for k in (1, 2)}
        for k in (1, 2):
            c = sr.counts(*ref[k][:2])
            for num in (n for n in EDGE_SIZES if n >= 31):
                assert (c[:2 * num] == 1).any() and (c[:2 * num] >= 3).any(), (m, k, num)
        out[m] = (q, ref)
    return out


def seeds_on_handles(K, idx, q, s, strands, stale=None):
    """A seed search on handles of exactly S * ns * num entries, filled on the
    host before the transfer; with `stale`, a search of those other reads runs
    first on the same device arrays, so every slot holds another task's record
    when the search under test starts."""
    ns = 2 if strands == sr.BOTH else 1
    slots = s * ns * q.shape[0]
    iv, sp = K.Results.alloc(slots), K.Results.alloc(slots)
    Q = K.Queries.from_array(q)
    try:
        iv.array()[:] = FILL
        sp.array()[:] = FILL
        K.transfer_to_gpu(idx, Q, iv)
        K.transfer_to_gpu(idx, None, sp)
        if stale is not None:
            P = K.Queries.from_array(stale)
            try:
                K.transfer_to_gpu(idx, P, None)
                K.search_seeds(idx, P, iv, sp, s, strands)
            finally:
                P.close()
        K.search_seeds(idx, Q, iv, sp, s, strands)
        K.transfer_to_cpu(iv)
        K.transfer_to_cpu(sp)
        return iv.array().copy().reshape(ns * q.shape[0], s, 2), sp.array().copy().reshape(ns * q.shape[0], s, 2)
    finally:
        Q.close()
        iv.close()
        sp.close()


@pytest.mark.parametrize("m", EDGE_LENGTHS)
@pytest.mark.parametrize("k,fused", [(1, True), (2, True), (2, False)], ids=["k1-fused", "k2-fused", "k2-packed-first"])
def test_batch_edges(world, edges, k, fused, m):
    """Batches that end inside a wave, a staging round or a block, on handles of
    exactly S * ns * num entries whose slots hold other tasks' records
    beforehand (the unused slots must be zeroed by the search itself); after
    each, the whole 513-read batch again, which a block that wrote past its own
    batch would have damaged."""
    K, w = world
    q, ref = edges[m]
    idx = w["main"]["idx"][k]
    try:
        defaults(K)
        K.set_fused(fused)
        K.set_backend("task-mid")
        for num in EDGE_SIZES:
            part = np.ascontiguousarray(q[:num])
            stale = np.ascontiguousarray(np.roll(part, 1, axis=0)[:, ::-1]) if num > 1 else np.ascontiguousarray(part[:, ::-1])
            for st in STRANDS:
                same(seeds_on_handles(K, idx, part, 3, st, stale), cut(ref[k], st, 3, num), (m, num, st))
                same(seeds_on_handles(K, idx, q, 3, st), cut(ref[k], st, 3), (m, num, st, "whole batch after"))
    finally:
        defaults(K)


CHILD = r"""
import json, sys
sys.path[:0] = %(paths)r
import numpy as np
import kstep_fmi as K
K.load(); K.set_device(0); K.set_backend("task-mid")
d = dict(np.load(%(data)r))
idx = K.Index.build(d["text"].tobytes(), k=%(k)d, d=64)
forms, bad, done = set(), [], 0
for m in d["lens"].tolist():
    q = d["q%%d" %% m]
    for strands in (1, 2, 3):
        ns = 2 if strands == 3 else 1
        Q, iv, sp = K.Queries.from_array(q), K.Results.alloc(3 * ns * q.shape[0]), K.Results.alloc(3 * ns * q.shape[0])
        K.transfer_to_gpu(idx, Q, iv)
        K.transfer_to_gpu(idx, None, sp)
        forms.add(K.upload_form(Q))
        K.search_seeds(idx, Q, iv, sp, 3, strands)
        K.transfer_to_cpu(iv); K.transfer_to_cpu(sp)
        rows = {1: slice(0, None, 2), 2: slice(1, None, 2), 3: slice(None)}[strands]
        if not (np.array_equal(iv.array().reshape(-1, 3, 2), d["iv%%d" %% m][rows]) and
                np.array_equal(sp.array().reshape(-1, 3, 2), d["sp%%d" %% m][rows])):
            bad.append([m, strands])
        Q.close(); iv.close(); sp.close()
        done += 1
print(json.dumps({"forms": sorted(forms), "bad": bad, "done": done}))
"""


@pytest.mark.parametrize("k", [1, 2])
def test_host_packed_upload(world, k, tmp_path):
    """KFMI_UPLOAD=packed in a process of its own: no ASCII on the device, so
    FWD walks the host's code words and REV / BOTH the strand pack's from them
    (seed_words_kernel either way), remainder codes included."""
    _, w = world
    cases = w["main"]["cases"]
    fn = tmp_path / "seeds.npz"
    data = {"text": w["main"]["text"], "lens": np.array(PACKED_LENGTHS, np.int64)}
    for m in PACKED_LENGTHS:
        data["q%d" % m] = cases[m][0]
        data["iv%d" % m], data["sp%d" % m] = cases[m][1][k][0][:, :3], cases[m][1][k][1][:, :3]
    np.savez(fn, **data)
    env = dict(os.environ)
    for v in ("KFMI_UPLOAD", "KFMI_UPLOAD_CHUNK", "KFMI_STREAM_HOSTPACK", "KFMI_STREAM_CHUNK", "KFMI_DEVICES",
              "KFMI_BACKEND", "KFMI_FTAB", "KFMI_SKIP", "KFMI_FUSED"):
        env.pop(v, None)
    env.update({"KFMI_UPLOAD": "packed", "KFMI_UPLOAD_CHUNK": "50"})
    code = CHILD % {"paths": [str(util.REPO), str(util.PKG), str(util.REPO / "tests")], "k": k, "data": str(fn)}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["done"] == 3 * len(PACKED_LENGTHS) and out["forms"] == ["packed"], out
    assert out["bad"] == [], out


def test_locate_reports_the_segments(world):
    """kfmi_locate on `intervals` as it stands (SA rate 1): record (start, len)
    of a task has R - L positions, and the text reads the task's segment at
    every one of them; the empty slots have none."""
    K, w = world
    t = w["main"]["text"]
    q, ref = w["main"]["cases"][100]
    idx = K.Index.build(t.tobytes(), k=2, d=64, sa_rate=1)
    s = 3
    tasks = code_of(sr.tasks_of(q, sr.BOTH))
    tc = code_of(t)
    Q, iv, sp = K.Queries.from_array(q), K.Results.alloc(s * tasks.shape[0]), K.Results.alloc(s * tasks.shape[0])
    try:
        defaults(K)
        K.set_backend("task-mid")
        K.transfer_to_gpu(idx, Q, iv)
        K.transfer_to_gpu(idx, None, sp)
        K.search_seeds(idx, Q, iv, sp, s, K.STRAND_BOTH)
        loc = K.locate(idx, iv, 0)
        off, pos = loc.offsets().copy(), loc.positions().copy()
        loc.close()
        K.transfer_to_cpu(iv)
        K.transfer_to_cpu(sp)
        ivs, sps = iv.array().reshape(-1, s, 2), sp.array().reshape(-1, s, 2)
        same((ivs, sps), cut(ref[2], sr.BOTH, s), "locate")
        assert off.size == s * tasks.shape[0] + 1
        seen = 0
        for ti in range(tasks.shape[0]):
            for r in range(s):
                slot = ti * s + r
                L, R = (int(x) for x in ivs[ti, r])
                b, ln = (int(x) for x in sps[ti, r])
                assert int(off[slot + 1] - off[slot]) == R - L, (ti, r)
                for p in pos[int(off[slot]):int(off[slot + 1])]:
                    assert np.array_equal(tc[int(p):int(p) + ln], tasks[ti, b:b + ln]), (ti, r, int(p))
                    seen += 1
        assert seen > tasks.shape[0]
    finally:
        Q.close()
        iv.close()
        sp.close()
        idx.close()
        defaults(K)


def refused(K, idx, q, s, strands):
    """(error code, whether the device arrays hold anything but the zeros of the transfer)."""
    slots = s * (2 if strands == sr.BOTH else 1) * q.shape[0]
    Q, iv, sp = K.Queries.from_array(q), K.Results.alloc(slots), K.Results.alloc(slots)
    try:
        K.transfer_to_gpu(idx, Q, iv)
        K.transfer_to_gpu(idx, None, sp)
        code = 0
        try:
            K.search_seeds(idx, Q, iv, sp, s, strands)
        except K.KfmiError as e:
            code = e.code
        K.transfer_to_cpu(iv)
        K.transfer_to_cpu(sp)
        return code, bool(iv.array().any() or sp.array().any())
    finally:
        Q.close()
        iv.close()
        sp.close()


def test_refusals_leave_both_arrays_untouched(world):
    K, w = world
    t = w["main"]["text"]
    q = w["main"]["cases"][100][0]
    idx2 = w["main"]["idx"][2]
    idx4 = K.Index.build(t.tobytes(), k=4, d=64)
    try:
        defaults(K)
        K.set_backend("task-mid")
        assert refused(K, idx2, q, 3, K.STRAND_BOTH) == (0, True)
        for backend, idx in (("coop-mid", idx2), ("task-ac-mid", idx2), ("task-grp", idx4)):
            K.set_backend(backend)
            assert refused(K, idx, q, 3, K.STRAND_FWD) == (19, False), backend
            assert refused(K, idx, q, 2, K.STRAND_BOTH) == (19, False), backend
        K.set_backend("task-mid")
        K.set_devices([0, 0])
        assert refused(K, idx2, q, 3, K.STRAND_FWD) == (19, False)
        K.set_devices([])
        long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
        assert refused(K, idx2, long, 3, K.STRAND_FWD) == (33, False)
        assert refused(K, idx2, long, 1, K.STRAND_REV) == (33, False)
    finally:
        defaults(K)
        idx2.free_gpu()
        idx4.close()


def test_device_equals_host(world):
    """A cross-check, not the reference: kfmi_search_seeds and kfmi_search_seeds_cpu agree."""
    K, w = world
    q = w["main"]["cases"][101][0]
    idx = w["main"]["idx"][2]
    try:
        defaults(K)
        got = K.search_seeds_array(idx, q, "task-mid", max_seeds=4, strands=K.STRAND_BOTH)
        same(got, K.search_seeds_array(idx, q, max_seeds=4, strands=K.STRAND_BOTH, cpu=True), "device against host")
    finally:
        defaults(K)
