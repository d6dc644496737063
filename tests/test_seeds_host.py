"""Seed search on the host (kstep_fmi.h, "seed search"), no GPU needed:

* kfmi_search_seeds_cpu equals the restatement of the definition in
  seed_ref.py (the CPU oracle on the K = 1 image for substring intervals,
  revcomp_def for the reverse strand), bit for bit on both arrays, unused slots
  included -- K = 1, 2, twelve lengths on both sides of every unit and word
  boundary, S in {1, 2, 3, 8}, every strand mode, the main text and the A / C
  text whose reads hold units that do not occur;
* a task whose whole-read interval is not empty has the single record
  {kfmi_search_cpu's interval, 0, m};
* the refusals (S = 0 and 9, reads of 257 bases, an AltCounters image, handles
  of another size, an unknown strand mode) return 33 and write nothing;
* the header's new symbols load through the binding."""
import re

import numpy as np
import pytest

import seed_ref as sr
import util

LENGTHS = (1, 2, 3, 15, 16, 17, 33, 64, 100, 101, 255, 256)
SEEDS = (1, 2, 3, 8)
STRANDS = (sr.FWD, sr.REV, sr.BOTH)
N_MAIN, N_AC = 64, 64


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    """Per text: the indexes at K = 1, 2, the reads of every length and the
    search callable of the reference (the oracle on the K = 1 image)."""
    K = kfmi_mod
    out = {}
    for name, t, reads in (("main", sr.main_text(), lambda t, m: sr.main_reads(t, m, 9_000 + m, N_MAIN)),
                           ("ac", sr.ac_text(), lambda t, m: sr.ac_reads(t, m, 8_000 + m, N_AC))):
        idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
        img1 = idx[1].image()
        out[name] = dict(text=t, idx=idx, reads={m: reads(t, m) for m in LENGTHS},
                         search=lambda q, img1=img1: oracle_mod.search(img1, q)[0])
    yield out
    for w in out.values():
        for i in w["idx"].values():
            i.close()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, "first differing task", int(np.argwhere(got != want)[0][0]))


@pytest.mark.parametrize("m", LENGTHS)
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", ["main", "ac"])
def test_host_equals_the_definition(kfmi_mod, world, text, k, m):
    K, w = kfmi_mod, world[text]
    q = w["reads"][m]
    for strands in STRANDS:
        tasks = sr.tasks_of(q, strands)
        refs = {s: sr.reference(w["search"], tasks, k, s) for s in SEEDS}
        if text == "main" and m >= 48 and strands != sr.BOTH:
            sr.assert_main_not_vacuous(m, refs[8], refs[2], (k, m, strands))
        if text == "ac" and m >= 15 and strands == sr.FWD:
            sr.assert_ac_not_vacuous(refs[8], 8, (k, m))
        for s in SEEDS:
            # the loop of the definition depends on S only through its end: fewer slots, a prefix
            # (test_seeds_gpu.py computes the reference once, at S = 8, and cuts it)
            assert np.array_equal(refs[s][0], refs[8][0][:, :s]) and np.array_equal(refs[s][1], refs[8][1][:, :s])
            iv, sp = K.search_seeds_array(w["idx"][k], q, max_seeds=s, strands=strands, cpu=True)
            same(iv, refs[s][0], (text, k, m, s, strands, "intervals"))
            same(sp, refs[s][1], (text, k, m, s, strands, "spans"))


@pytest.mark.parametrize("k", [1, 2])
def test_reference_records_are_what_they_claim(world, k):
    """The restatement against brute force on the A / C text: every record's
    interval is the suffix-array interval of its substring, the next unit to
    the left does not extend it, and records tile the task from the right with
    gaps only where a unit was skipped."""
    w = world["ac"]
    bf = util.BruteForce(w["text"].tobytes().decode())
    for m in (3, 17, 100):
        tasks = sr.tasks_of(w["reads"][m], sr.BOTH)
        iv, sp, skips = sr.reference(w["search"], tasks, k, 8)
        for t in range(tasks.shape[0]):
            e, covered, n = m, 0, 0
            for s in range(8):
                b, ln = int(sp[t, s, 0]), int(sp[t, s, 1])
                if ln == 0:
                    assert not iv[t, s:].any() and not sp[t, s:].any()
                    break
                assert b + ln <= e and tuple(iv[t, s]) == bf.interval(tasks[t, b:b + ln].tobytes())
                assert iv[t, s, 1] > iv[t, s, 0] and (b + ln == m or (m - b - ln - m % k) % k == 0)
                if b > 0:
                    lo, hi = bf.interval(tasks[t, b - k:b + ln].tobytes())
                    assert hi <= lo
                e, covered, n = b, covered + ln, n + 1
            if n < 8:   # the whole task was walked: what no record covers was skipped, unit by unit
                assert (m - covered > 0) == (skips[t] > 0)
                assert m - covered in (k * skips[t], k * (skips[t] - 1) + m % k)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("m", [16, 17, 100, 101, 256])
def test_whole_read_match_is_the_single_record(kfmi_mod, world, k, m):
    K, w = kfmi_mod, world["main"]
    q = w["reads"][m]
    whole = K.search_cpu_array(w["idx"][k], q, strands=K.STRAND_BOTH).reshape(-1, 2)
    hit = whole[:, 1] > whole[:, 0]
    assert 4 * np.count_nonzero(hit) >= hit.size
    for s in (1, 4):
        iv, sp = K.search_seeds_array(w["idx"][k], q, max_seeds=s, strands=K.STRAND_BOTH, cpu=True)
        assert np.array_equal(iv[hit, 0], whole[hit])
        assert np.all(sp[hit, 0, 0] == 0) and np.all(sp[hit, 0, 1] == m)
        assert not iv[hit, 1:].any() and not sp[hit, 1:].any()
        # and a task without a whole-read match never reports one
        assert np.all(sp[~hit, :, 1] < m)


def _call(K, idx, q, s, strands, slots_iv, slots_sp):
    """search_seeds_cpu on handles of the given sizes, pre-filled; returns
    (error code, whether either array changed)."""
    Q, iv, sp = K.Queries.from_array(q), K.Results.alloc(slots_iv), K.Results.alloc(slots_sp)
    try:
        iv.array()[:] = 0xA5A5A5A5
        sp.array()[:] = 0xA5A5A5A5
        code = 0
        try:
            K.search_seeds_cpu(idx, Q, iv, sp, s, strands)
        except K.KfmiError as e:
            code = e.code
        touched = bool((iv.array() != 0xA5A5A5A5).any() or (sp.array() != 0xA5A5A5A5).any())
        return code, touched
    finally:
        Q.close()
        iv.close()
        sp.close()


def test_refusals_write_nothing(kfmi_mod, world):
    K, w = kfmi_mod, world["main"]
    idx, q = w["idx"][2], w["reads"][100]
    n = q.shape[0]
    assert _call(K, idx, q, 3, K.STRAND_FWD, 3 * n, 3 * n) == (0, True)
    for s, strands, a, b in ((0, K.STRAND_FWD, n, n), (9, K.STRAND_FWD, 9 * n, 9 * n), (3, 0, 3 * n, 3 * n),
                             (3, 4, 3 * n, 3 * n), (3, K.STRAND_FWD, 3 * n - 1, 3 * n), (3, K.STRAND_FWD, 3 * n, 3 * n + 1),
                             (3, K.STRAND_BOTH, 3 * n, 3 * n), (3, K.STRAND_REV, 6 * n, 6 * n)):
        assert _call(K, idx, q, s, strands, a, b) == (33, False), (s, strands, a, b)
    long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
    assert _call(K, idx, long, 2, K.STRAND_FWD, 2 * n, 2 * n) == (33, False)
    acs = idx.alt_counters()
    try:
        for ac in acs:
            assert _call(K, ac, q, 2, K.STRAND_FWD, 2 * n, 2 * n) == (33, False)
    finally:
        for ac in acs:
            ac.close()


def test_header_symbols_load_through_the_binding(kfmi_mod):
    lib = kfmi_mod.load()
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name, nargs in (("kfmi_search_seeds", 6), ("kfmi_search_seeds_cpu", 7)):
        assert re.search(r"\bint32_t\s+%s\(" % name, header), name
        f = getattr(lib, name)
        assert len(f.argtypes) == nargs and f.restype is not None
    for name in ("search_seeds", "search_seeds_cpu", "search_seeds_array"):
        assert callable(getattr(kfmi_mod, name))
