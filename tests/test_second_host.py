"""Second placement / mapping quality on the host (kstep_fmi.h, "second
placement / mapping quality"), no GPU needed:

* kfmi_align_second_cpu and kfmi_map_quality_cpu equal the model of
  second_ref.py bit for bit on both words of every record -- K = 1, 2, six
  lengths, every strand mode, greedy seeds at S in {1, 8} and piece seeds at S
  in {1, 4}, max_occ in {1, 8}, bands 0, 1, 3, 15, max_second in {0, 1, m}, on
  the model's align records as hits, under max_edits = m and under max_edits
  = 0, where records hold KFMI_HIT_NONE: the whole product, in every strand
  mode;
* the non-vacuity conditions hold on the model alone (second_ref.world asserts
  them before any library call);
* the header's consequences hold on kfmi_align_seeds_cpu's own hits;
* at band 0 the second is a direct second-best Hamming count;
* hand-made handles: X = NONE, X past the text, empty and ignored slots, the
  FILL pattern overwritten everywhere;
* every refusal returns 33 and writes nothing;
* the header's and the binding's symbols are there;
* tests/asan/second_asan.c runs clean under AddressSanitizer + UBSan;
* tests/asan/second_fold_host.cpp: band_fold_far (csrc/hip/kfmi_align_dp.h,
  compiled for the host) equals a fold over the plain table at every band and
  every X offset from -3w - 1 to 3w + 1, under the same sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_ref as ar
import second_ref as s2
import seed_ref as sr
import util
import verify_ref as vr
from test_verify_host import handmade, same

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    return s2.world(kfmi_mod, oracle_mod)


class Host:
    """Handles filled with the given seed records; second() / quality() run the host forms on them."""

    def __init__(self, K, w, q, iv, sp, s, strands, sa=None):
        ns = 2 if strands == sr.BOTH else 1
        self.K, self.w, self.s, self.strands, self.T = K, w, s, strands, ns * q.shape[0]
        assert iv.shape == (self.T, s, 2) and sp.shape == (self.T, s, 2)
        self.sa = (w.sa if sa is None else sa).astype(np.uint32)
        self.Q, self.I, self.S = K.Queries.from_array(q), K.Results.alloc(self.T * s), K.Results.alloc(self.T * s)
        self.H, self.H2, self.HQ = K.Results.alloc(self.T), K.Results.alloc(self.T), K.Results.alloc(self.T)
        self.I.array()[:] = iv.reshape(-1)
        self.S.array()[:] = sp.reshape(-1)

    def align(self, occ, band, me):
        self.K.align_seeds_cpu(self.w.text, self.sa, self.Q, self.I, self.S, self.H, self.s, self.strands, occ, band, me)
        return self.H.array().copy().reshape(self.T, 2)

    def second(self, hits, occ, band, ms):
        if hits is not None:
            self.H.array()[:] = np.asarray(hits, np.uint32).reshape(-1)
        self.H2.array()[:] = FILL
        self.K.align_second_cpu(self.w.text, self.sa, self.Q, self.I, self.S, self.H, self.H2, self.s, self.strands, occ,
                                band, ms)
        return self.H2.array().copy().reshape(self.T, 2)

    def quality(self, ms):
        self.HQ.array()[:] = FILL
        self.K.map_quality_cpu(self.H, self.H2, self.HQ, self.strands, ms)
        return self.HQ.array().copy().reshape(self.T, 2)

    def close(self):
        for h in (self.Q, self.I, self.S, self.H, self.H2, self.HQ):
            h.close()


def seed_sets(greedy, piece, k):
    """(name, Seeded, the S values) of the two seed kinds."""
    return (("greedy", greedy[k], (1, 8)), ("piece", piece, (1, s2.PIECES)))


@pytest.mark.parametrize("k", [1, 2])
def test_host_equals_the_model(kfmi_mod, world, k):
    K, w = kfmi_mod, world["world"]
    for m, (q, both, greedy, piece) in world["cases"].items():
        for name, x, seeds in seed_sets(greedy, piece, k):
            if name == "piece" and k == 2:
                continue                                          # piece seeds do not depend on K
            for strands in ar.STRANDS:
                rows = vr.strand_rows(strands)
                for s in seeds:
                    h = Host(K, w, q, np.ascontiguousarray(x.iv[rows, :s]), np.ascontiguousarray(x.sp[rows, :s]), s, strands)
                    try:
                        for occ in (1, 8):
                            trunc = x.trunc(s, occ)
                            for band in s2.BANDS:
                                for me in (m, 0):                              # me = 0: records with KFMI_HIT_NONE
                                    hits = ar.records(x.a, s, occ, band, me)
                                    for ms in s2.second_bounds(m):
                                        what = (name, k, m, strands, s, occ, band, me, ms)
                                        want = s2.second_records(x.a, hits[:, 0], s, occ, band, ms, trunc)
                                        same(h.second(hits[rows], occ, band, ms), want[rows], what)
                                        same(h.quality(ms), s2.quality(hits[rows], want[rows], strands, ms), what + ("quality",))
                    finally:
                        h.close()


def test_consequences_on_the_aligns_own_hits(kfmi_mod, world):
    """E2 >= E, E2 = E <=> KFMI_HIT_MULTI and counted <= scored, on what kfmi_align_seeds_cpu itself reported."""
    K, w = kfmi_mod, world["world"]
    seen = 0
    for m in (17, 100, 129, 256):
        q, both, greedy, piece = world["cases"][m]
        for name, x, seeds in seed_sets(greedy, piece, 2):
            h = Host(K, w, q, x.iv, x.sp, x.S, sr.BOTH)
            try:
                for occ in (1, 8):
                    for band in s2.BANDS:
                        hits = h.align(occ, band, m)
                        sec = h.second(None, occ, band, m)
                        placed, have = hits[:, 0] != s2.NONE, sec[:, 0] != s2.NONE
                        assert not (have & ~placed).any()
                        E, E2 = (hits[:, 1] & s2.EDIT_MASK).astype(np.int64), (sec[:, 1] & s2.EDIT_MASK).astype(np.int64)
                        assert (E2[have] >= E[have]).all(), (name, m, occ, band)
                        multi = (hits[:, 1] & s2.MULTI) != 0
                        assert np.array_equal(have & (E2 == E), placed & multi), (name, m, occ, band)
                        assert ((sec[:, 1] >> s2.SCORED_SHIFT) <= (hits[:, 1] >> s2.SCORED_SHIFT)).all(), (name, m, occ, band)
                        seen += int((have & (E2 == E)).sum())
            finally:
                h.close()
    assert seen > 0


def test_band_zero_is_the_second_best_hamming_count(kfmi_mod, world):
    K, w = kfmi_mod, world["world"]
    for m in (16, 100, 256):
        q, both, greedy, piece = world["cases"][m]
        x = piece
        c = x.a.c
        h = Host(K, w, q, x.iv, x.sp, x.S, sr.BOTH)
        try:
            hits = h.align(8, 0, m)
            sec = h.second(None, 8, 0, m)
        finally:
            h.close()
        sc = c.why == vr.SCORED
        some = False
        for t in range(c.T):
            if hits[t, 0] == s2.NONE:
                assert sec[t].tolist() == [s2.NONE, 0]
                continue
            others = sc & (c.task == t) & (c.origin != int(hits[t, 0]))
            if others.any():
                best = int(c.mism[others].min())
                assert sec[t, 0] == int(c.origin[others & (c.mism == best)].min()) and (sec[t, 1] & s2.EDIT_MASK) == best, (m, t)
                some = True
            else:
                assert sec[t, 0] == s2.NONE, (m, t)
        assert some


def test_hand_made_handles(kfmi_mod, world):
    """test_verify_host.handmade's slots (ignored forms, R > rows, garbage, rows
    without a suffix) with hand-made X: the aligns own, NONE, past the text, 0."""
    K, w = kfmi_mod, world["world"]
    q, iv, sp = handmade(w)
    holes = w.sa.copy()
    holes[::3] = 0xFFFFFFFF
    for sa in (w.sa, holes):
        for occ in (1, 7, 256):
            a = ar.Aligned(w, q, vr.candidates(w, q, iv, sp, occ, sa=sa), bands=(0, 2, 15))
            trunc = s2.truncated(w, q.shape[1], iv, sp, 8, occ)
            assert trunc.any() and not trunc.all()
            h = Host(K, w, q, iv, sp, 8, sr.FWD, sa=sa)
            try:
                for band in (0, 2, 15):
                    own = ar.records(a, 8, occ, band, 0xFFFFFFFF)
                    for X in (own[:, 0], np.asarray([s2.NONE, w.n + 50, 0, 7], np.uint32), np.full(4, s2.NONE, np.uint32)):
                        hits = np.stack([X, np.full(4, FILL, np.uint32)], axis=1)      # word y is not read
                        for ms in (0, 40, 0xFFFFFFFF):
                            got = h.second(hits, occ, band, ms)
                            same(got, s2.second_records(a, X, 8, occ, band, ms, trunc), ("hand-made", occ, band, ms))
                            assert not (got == FILL).all(axis=1).any()
                            same(h.quality(ms), s2.quality(hits, got, sr.FWD, ms), ("hand-made quality", occ, band, ms))
            finally:
                h.close()


BY_HAND_HITS = [[10, 1], [s2.NONE, 0], [10, 2], [500, 2], [10, 0], [20, 0], [10, 0], [s2.NONE, 0]]
BY_HAND_SECOND = [[90, 3], [s2.NONE, 0], [s2.NONE, 0], [s2.NONE, 0], [s2.NONE, s2.TRUNC], [s2.NONE, 0], [s2.NONE, 0], [s2.NONE, 0]]
BY_HAND_QUALITY = {      # (strands, max_second) -> records worked out by hand from the header's rule
    (sr.FWD, 6): [[20, 2], [0, 0], [50, 5], [50, 5], [3, 7], [60, 7], [60, 7], [0, 0]],
    (sr.REV, 6): [[20, 2], [0, 0], [50, 5], [50, 5], [3, 7], [60, 7], [60, 7], [0, 0]],
    # the other strand competes; equal edits on both strands; a truncated strand caps the other
    (sr.BOTH, 6): [[20, 2], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [60, 7], [0, 0]],
    # max_second + 1 = 2^32: the gap's word saturates
    (sr.FWD, 0xFFFFFFFF): [[20, 2], [0, 0], [60, 0xFFFFFFFE], [60, 0xFFFFFFFE], [3, 0xFFFFFFFF], [60, 0xFFFFFFFF], [60, 0xFFFFFFFF], [0, 0]],
    (sr.FWD, 0): [[0, 0], [0, 0], [0, 0], [0, 0], [3, 1], [10, 1], [10, 1], [0, 0]],
}


def test_quality_host_equals_the_rule_by_hand(kfmi_mod):
    """kfmi_map_quality_cpu and the model on records written out by hand, against numbers worked out by hand:
    the strand that competes, the REV clause, the cap under truncation, saturation."""
    K = kfmi_mod
    hits, sec = np.asarray(BY_HAND_HITS, np.uint32), np.asarray(BY_HAND_SECOND, np.uint32)
    hs = [K.Results.alloc(8) for _ in range(3)]
    try:
        hs[0].array()[:], hs[1].array()[:] = hits.reshape(-1), sec.reshape(-1)
        for (strands, ms), want in BY_HAND_QUALITY.items():
            want = np.asarray(want, np.uint32)
            hs[2].array()[:] = FILL
            K.map_quality_cpu(hs[0], hs[1], hs[2], strands, ms)
            same(hs[2].array().copy().reshape(8, 2), want, ("host", strands, ms))
            same(s2.quality(hits, sec, strands, ms), want, ("model", strands, ms))
    finally:
        for h in hs:
            h.close()


def _call(K, w, q, s, strands, occ, band, sizes, same_handles=False):
    """(error code, whether any array changed); sizes: intervals, spans, hits, second."""
    Q = K.Queries.from_array(q)
    hs = [K.Results.alloc(n) for n in sizes]
    try:
        for h in hs:
            h.array()[:] = FILL
        code = 0
        try:
            K.align_second_cpu(w.text, w.sa.astype(np.uint32), Q, hs[0], hs[1], hs[2], hs[2] if same_handles else hs[3], s,
                               strands, occ, band, 3)
        except K.KfmiError as e:
            code = e.code
        return code, any(bool((h.array() != FILL).any()) for h in hs)
    finally:
        Q.close()
        for h in hs:
            h.close()


def test_refusals_write_nothing(kfmi_mod, world):
    K, w = kfmi_mod, world["world"]
    q = world["cases"][100][0][:16]
    n = q.shape[0]
    assert _call(K, w, q, 3, K.STRAND_FWD, 8, 3, (3 * n, 3 * n, n, n)) == (0, True)
    assert _call(K, w, q, 3, K.STRAND_BOTH, 8, 15, (6 * n, 6 * n, 2 * n, 2 * n)) == (0, True)
    for s, strands, occ, band, sizes in (
            (0, 1, 8, 3, (n, n, n, n)), (9, 1, 8, 3, (9 * n, 9 * n, n, n)), (3, 0, 8, 3, (3 * n, 3 * n, n, n)),
            (3, 4, 8, 3, (3 * n, 3 * n, n, n)), (3, 1, 0, 3, (3 * n, 3 * n, n, n)), (3, 1, 257, 3, (3 * n, 3 * n, n, n)),
            (3, 1, 8, 3, (3 * n - 1, 3 * n, n, n)), (3, 1, 8, 3, (3 * n, 3 * n + 1, n, n)), (3, 1, 8, 3, (3 * n, 3 * n, n + 1, n)),
            (3, 1, 8, 3, (3 * n, 3 * n, n, n - 1)), (3, 1, 8, 3, (3 * n, 3 * n, n, n + 1)), (3, 3, 8, 3, (3 * n, 3 * n, n, n)),
            (3, 3, 8, 3, (6 * n, 6 * n, n, 2 * n)), (3, 2, 8, 3, (6 * n, 6 * n, 2 * n, 2 * n)),
            (3, 1, 8, 16, (3 * n, 3 * n, n, n)), (3, 1, 8, 0xFFFFFFFF, (3 * n, 3 * n, n, n))):
        assert _call(K, w, q, s, strands, occ, band, sizes) == (33, False), (s, strands, occ, band, sizes)
    assert _call(K, w, q, 3, K.STRAND_FWD, 8, 3, (3 * n, 3 * n, n, n), same_handles=True) == (33, False)
    long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
    assert _call(K, w, long, 2, K.STRAND_FWD, 8, 3, (2 * n, 2 * n, n, n)) == (33, False)
    # the quality: strands, sizes, one handle twice, an odd size in BOTH mode
    for strands, sizes, twice in ((0, (8, 8, 8), False), (4, (8, 8, 8), False), (1, (8, 8, 9), False), (1, (8, 9, 8), False),
                                  (1, (9, 8, 8), False), (3, (7, 7, 7), False), (1, (8, 8, 8), True)):
        hs = [K.Results.alloc(x) for x in sizes]
        try:
            for h in hs:
                h.array()[:] = FILL
            with pytest.raises(K.KfmiError) as e:
                K.map_quality_cpu(hs[0], hs[1], hs[1] if twice else hs[2], strands, 3)
            assert e.value.code == 33
            assert all(bool((h.array() == FILL).all()) for h in hs)
        finally:
            for h in hs:
                h.close()


def test_header_symbols_load_through_the_binding(kfmi_mod):
    lib = kfmi_mod.load()
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name, nargs in (("kfmi_align_second", 11), ("kfmi_align_second_cpu", 15), ("kfmi_map_quality", 6),
                        ("kfmi_map_quality_cpu", 5)):
        assert re.search(r"\bint32_t\s+%s\(" % name, header), name
        f = getattr(lib, name)
        assert len(f.argtypes) == nargs and f.restype is not None
    assert re.search(r"#define\s+KFMI_SECOND_TRUNCATED\s+0x00080000u\b", header)
    for name, value in (("KFMI_MAPQ_MAX", 60), ("KFMI_MAPQ_PER_EDIT", 10), ("KFMI_MAPQ_TRUNCATED", 3)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), header), name
    assert kfmi_mod.SECOND_TRUNCATED == s2.TRUNC == 0x80000
    assert (kfmi_mod.MAPQ_MAX, kfmi_mod.MAPQ_PER_EDIT, kfmi_mod.MAPQ_TRUNCATED) == (s2.MAPQ_MAX, s2.MAPQ_PER_EDIT, s2.MAPQ_TRUNCATED)
    assert s2.TRUNC & (kfmi_mod.PAIR_PROPER | kfmi_mod.PAIR_RESCUED | kfmi_mod.HIT_MULTI | kfmi_mod.HIT_MISM_MASK) == 0
    for name in ("align_second", "align_second_cpu", "map_quality", "map_quality_cpu", "decode_second", "piece_seeds",
                 "map_reads_array"):
        assert callable(getattr(kfmi_mod, name))
    assert kfmi_mod.piece_bounds(129, 4) == s2.piece_bounds(129, 4) == [(0, 32), (32, 32), (64, 32), (96, 33)]


def test_piece_seeds_and_map_reads_on_the_host(kfmi_mod, world):
    """piece_seeds(cpu=True) gives the model's rows wherever a piece occurs, and
    map_reads_array(cpu=True, mapq=True) is the three host calls in a row; the
    call without the new keyword arguments returns the four arrays it returned."""
    K, w = kfmi_mod, world["world"]
    q, both, greedy, piece = world["cases"][129]
    iv, sp = K.piece_seeds(world["idx"][2], q, s2.PIECES, K.STRAND_BOTH, cpu=True)
    found = piece.iv[:, :, 1] > piece.iv[:, :, 0]
    assert found.any() and (~found).any()
    assert np.array_equal(iv[found], piece.iv[found]) and np.array_equal(sp, piece.sp)
    assert (iv[~found][:, 1] <= iv[~found][:, 0]).all()
    for strands in (K.STRAND_FWD, K.STRAND_REV):
        ivs, sps = K.piece_seeds(world["idx"][1], q, s2.PIECES, strands, cpu=True)
        rows = vr.strand_rows(strands)
        assert np.array_equal(ivs[found[rows]], piece.iv[rows][found[rows]]) and np.array_equal(sps, piece.sp[rows])
    got = K.map_reads_array(world["idx"][2], q, max_occ=8, cpu=True, text=world["text"], band=3, max_edits=129, mapq=True,
                            max_second=6, pieces=s2.PIECES)
    assert len(got) == 6
    hits = ar.records(piece.a, s2.PIECES, 8, 3, 129)
    sec = s2.second_records(piece.a, hits[:, 0], s2.PIECES, 8, 3, 6, piece.trunc(s2.PIECES, 8))
    ql = s2.quality(hits, sec, sr.BOTH, 6)
    assert np.array_equal(got[0], np.where(hits[:, 0] == s2.NONE, -1, hits[:, 0].astype(np.int64)))
    assert np.array_equal(got[4], ql[:, 0]) and np.array_equal(got[5], ql[:, 1])
    assert len(set(got[4].tolist())) >= 4 and 60 in got[4] and 3 in got[4]
    plain = K.map_reads_array(world["idx"][2], q, max_seeds=8, max_occ=8, cpu=True, text=world["text"], band=3, max_edits=3)
    assert len(plain) == 4
    want = ar.records(greedy[2].a, 8, 8, 3, 3)
    assert np.array_equal(plain[0], np.where(want[:, 0] == s2.NONE, -1, want[:, 0].astype(np.int64)))
    assert np.array_equal(plain[3], want[:, 1] >> s2.SCORED_SHIFT)
    with pytest.raises(ValueError):
        K.map_reads_array(world["idx"][2], q, cpu=True, text=world["text"], mapq=True)


def _sanitized(tmp_path, compiler, std, name, srcs, extra=()):
    if not shutil.which(compiler):
        pytest.skip(compiler + " not available")
    out = tmp_path / name
    cmd = [compiler, "-g", "-O1", std, *extra, "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(out)] + srcs
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4")
    p = subprocess.run([str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK"), p.stdout[-2000:] + p.stderr[-4000:]
    return int(p.stdout.split()[1])


def test_second_clean_under_asan(tmp_path):
    """tests/asan/second_asan.c with csrc/host/*.c under -fsanitize=address,undefined:
    a stand-alone program, the HIP layer stubbed."""
    srcs = sorted(str(p) for p in (util.PKG / "csrc" / "host").glob("*.c"))
    checks = _sanitized(tmp_path, "gcc", "-std=gnu11", "second_asan", [str(util.REPO / "tests" / "asan" / "second_asan.c")] + srcs,
                        ("-fopenmp",))
    assert checks > 5_000


def test_far_fold_equals_the_plain_table_under_asan(tmp_path):
    """tests/asan/second_fold_host.cpp: band_fold_far against a fold over row 0
    of the plain table, every band, every X offset from -3w - 1 to 3w + 1."""
    cases = _sanitized(tmp_path, "g++", "-std=c++17", "second_fold_host",
                       [str(util.REPO / "tests" / "asan" / "second_fold_host.cpp")])
    # 3 texts x 3 lengths x 6 origins x 16 bands x about (6w + 4) offsets, two folds each where the neighbour fits
    assert cases >= 3 * 3 * 6 * sum(3 * w + 3 for w in range(16))
