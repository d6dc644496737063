"""Align seeds on the host (kstep_fmi.h, "align seeds"), no GPU needed:

* kfmi_align_seeds_cpu equals the model of align_ref.py bit for bit on both
  words of every record -- four texts, K = 1, 2, fourteen lengths, six bands,
  every strand mode, S in {1, 4, 8}, max_occ in {1, 2, 8}, max_edits in
  {0, 1, m}.  The seed records it is given are seed_ref.reference's, written
  into the handles' host arrays; the suffix array it is given is the model's;
* the non-vacuity conditions hold on the model alone (align_ref.world asserts
  them before any library call);
* at band 0 it equals kfmi_verify_seeds_cpu on the same handles;
* test_verify_host.handmade's slots (ignored forms, R > rows, garbage, rows
  without a suffix) at max_occ 1, 7, 256;
* the refusals return 33 and write nothing;
* the header's and the binding's symbols are there;
* tests/asan/align_asan.c runs clean under AddressSanitizer + UBSan;
* tests/asan/align_dp_host.cpp: the kernel's own arithmetic (csrc/hip/
  kfmi_align_dp.h, compiled for the host) equals a plain full-table DP, under
  the same sanitizers, on low-complexity texts at every band."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_ref as ar
import seed_ref as sr
import util
import verify_ref as vr
from test_verify_host import handmade, host_hits as verify_hits, same

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    return ar.world(kfmi_mod, oracle_mod)


class Host:
    """Handles filled with the given records; align() runs kfmi_align_seeds_cpu on them."""

    def __init__(self, K, w, q, iv, sp, s, strands, sa=None):
        ns = 2 if strands == sr.BOTH else 1
        self.K, self.w, self.s, self.strands, self.T = K, w, s, strands, ns * q.shape[0]
        assert iv.shape == (self.T, s, 2) and sp.shape == (self.T, s, 2)
        self.sa = (w.sa if sa is None else sa).astype(np.uint32)
        self.Q, self.I, self.S, self.H = (K.Queries.from_array(q), K.Results.alloc(self.T * s), K.Results.alloc(self.T * s),
                                          K.Results.alloc(self.T))
        self.I.array()[:] = iv.reshape(-1)
        self.S.array()[:] = sp.reshape(-1)

    def align(self, occ, band, me):
        self.H.array()[:] = FILL
        self.K.align_seeds_cpu(self.w.text, self.sa, self.Q, self.I, self.S, self.H, self.s, self.strands, occ, band, me)
        return self.H.array().copy().reshape(self.T, 2)

    def close(self):
        for h in (self.Q, self.I, self.S, self.H):
            h.close()


def host_hits(K, w, q, iv, sp, s, strands, occ, band, me, sa=None):
    h = Host(K, w, q, iv, sp, s, strands, sa)
    try:
        return h.align(occ, band, me)
    finally:
        h.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", list(vr.texts()))
def test_host_equals_the_model(kfmi_mod, world, text, k):
    K, w = kfmi_mod, world[text]
    for m, (q, both, per_k) in w["cases"].items():
        iv, sp, a = per_k[k]
        for strands in ar.STRANDS:
            rows = vr.strand_rows(strands)
            # BOTH holds every task of FWD and of REV: the single strands go through one S and one max_occ
            for s in ar.SEEDS if strands == sr.BOTH else (4,):
                h = Host(K, w["world"], q, np.ascontiguousarray(iv[rows, :s]), np.ascontiguousarray(sp[rows, :s]), s, strands)
                try:
                    for occ in ar.OCCS if strands == sr.BOTH else (8,):
                        for band in ar.BANDS:
                            for me in ar.edit_bounds(m):
                                same(h.align(occ, band, me), ar.records(a, s, occ, band, me, rows),
                                     (text, k, m, strands, s, occ, band, me))
                finally:
                    h.close()


def test_band_zero_is_the_verify(kfmi_mod, world):
    """Band 0: the model's records are verify_ref's, and the host form equals kfmi_verify_seeds_cpu."""
    K = kfmi_mod
    for text, w in world.items():
        for m in (1, 17, 100, 129, 256):
            q, both, per_k = w["cases"][m]
            iv, sp, a = per_k[2]
            for mm in (0, 3, m):
                want = verify_hits(K, w["world"], q, iv, sp, 8, sr.BOTH, 8, mm)
                same(vr.records(a.c, 8, 8, mm), want, (text, m, mm, "verify_ref"))
                same(ar.records(a, 8, 8, 0, mm), want, (text, m, mm, "model"))
                same(host_hits(K, w["world"], q, iv, sp, 8, sr.BOTH, 8, 0, mm), want, (text, m, mm, "host"))


def test_indel_reads_are_placed(world):
    """On the model: every single-indel read maps with one edit at band 1 on
    the strand it was built from, and the 3-base indels with three at band 3."""
    for name, w in world.items():
        t = w["text"]
        for m in (100, 101, 256):
            q, both, per_k = w["cases"][m]
            a = per_k[2][2]
            extra = ar.indel_reads(t, m, 17_000 + m + 1)
            first = vr.reads_for(t, m, 17_000 + m).shape[0]
            assert np.array_equal(q[first:first + extra.shape[0]], extra)
            e1, e3 = ar.edits_of(ar.records(a, 8, 8, 1, m)), ar.edits_of(ar.records(a, 8, 8, 3, m))
            singles = 2 * len(ar.pinned(m))
            for r in range(singles):
                assert 0 <= e1[2 * (first + r)] <= 1, (name, m, r, e1[2 * (first + r)])
            for r in (singles, singles + 1):
                assert 0 <= e3[2 * (first + r)] <= 3, (name, m, r)
            assert 0 <= e1[2 * (first + singles + 2)] <= 2, (name, m, "deletion and insertion")


def test_hand_made_slots(kfmi_mod, world):
    w = world["n1005"]["world"]
    q, iv, sp = handmade(w)
    holes = w.sa.copy()
    holes[::3] = 0xFFFFFFFF                                    # rows without a suffix
    for sa in (w.sa, holes):
        for occ in (1, 7, 256):
            a = ar.Aligned(w, q, vr.candidates(w, q, iv, sp, occ, sa=sa), bands=(0, 2, 15))
            for band in (0, 2, 15):
                for me in (0, 40, 0xFFFFFFFF):
                    got = host_hits(kfmi_mod, w, q, iv, sp, 8, sr.FWD, occ, band, me, sa=sa)
                    same(got, ar.records(a, 8, occ, band, me), ("hand-made", occ, band, me))
    assert (host_hits(kfmi_mod, w, q, iv, sp, 8, sr.FWD, 256, 15, 40)[:, 1] >> ar.SCORED_SHIFT).max() > 200


def _call(K, w, q, s, strands, occ, band, n_iv, n_sp, n_hits):
    """(error code, whether any array changed)."""
    Q = K.Queries.from_array(q)
    hs = [K.Results.alloc(n) for n in (n_iv, n_sp, n_hits)]
    try:
        for h in hs:
            h.array()[:] = FILL
        code = 0
        try:
            K.align_seeds_cpu(w.text, w.sa.astype(np.uint32), Q, hs[0], hs[1], hs[2], s, strands, occ, band, 3)
        except K.KfmiError as e:
            code = e.code
        return code, any(bool((h.array() != FILL).any()) for h in hs)
    finally:
        Q.close()
        for h in hs:
            h.close()


def test_refusals_write_nothing(kfmi_mod, world):
    K, w = kfmi_mod, world["n1008"]["world"]
    q = world["n1008"]["cases"][100][0][:16]
    n = q.shape[0]
    assert _call(K, w, q, 3, K.STRAND_FWD, 8, 3, 3 * n, 3 * n, n) == (0, True)
    assert _call(K, w, q, 3, K.STRAND_BOTH, 8, 15, 6 * n, 6 * n, 2 * n) == (0, True)
    for s, strands, occ, band, a, b, c in (
            (0, 1, 8, 3, n, n, n), (9, 1, 8, 3, 9 * n, 9 * n, n), (3, 0, 8, 3, 3 * n, 3 * n, n), (3, 4, 8, 3, 3 * n, 3 * n, n),
            (3, 1, 0, 3, 3 * n, 3 * n, n), (3, 1, 257, 3, 3 * n, 3 * n, n), (3, 1, 8, 3, 3 * n - 1, 3 * n, n),
            (3, 1, 8, 3, 3 * n, 3 * n + 1, n), (3, 1, 8, 3, 3 * n, 3 * n, n + 1), (3, 1, 8, 3, 3 * n, 3 * n, n - 1),
            (3, 3, 8, 3, 3 * n, 3 * n, n), (3, 3, 8, 3, 6 * n, 6 * n, n), (3, 2, 8, 3, 6 * n, 6 * n, 2 * n),
            (3, 1, 8, 16, 3 * n, 3 * n, n), (3, 1, 8, 0xFFFFFFFF, 3 * n, 3 * n, n)):
        assert _call(K, w, q, s, strands, occ, band, a, b, c) == (33, False), (s, strands, occ, band, a, b, c)
    long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
    assert _call(K, w, long, 2, K.STRAND_FWD, 8, 3, 2 * n, 2 * n, n) == (33, False)
    Q, hs = K.Queries.from_array(q), [K.Results.alloc(x) for x in (n, n, n)]
    try:
        with pytest.raises(K.KfmiError) as e:     # a suffix array that is not the text's n + 1 rows
            K.align_seeds_cpu(w.text, w.sa[:-1].astype(np.uint32), Q, hs[0], hs[1], hs[2], 1, 1, 8, 3, 0)
        assert e.value.code == 33
    finally:
        Q.close()
        for h in hs:
            h.close()


def test_header_symbols_load_through_the_binding(kfmi_mod):
    lib = kfmi_mod.load()
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name, nargs in (("kfmi_align_seeds", 10), ("kfmi_align_seeds_cpu", 14)):
        assert re.search(r"\bint32_t\s+%s\(" % name, header), name
        f = getattr(lib, name)
        assert len(f.argtypes) == nargs and f.restype is not None
    assert re.search(r"#define\s+KFMI_ALIGN_MAX_BAND\s+15u\b", header)
    assert kfmi_mod.ALIGN_MAX_BAND == ar.MAX_BAND == 15
    for name in ("align_seeds", "align_seeds_cpu", "map_reads_array"):
        assert callable(getattr(kfmi_mod, name))


def test_map_reads_on_the_host(kfmi_mod, world):
    """map_reads_array(cpu=True, band=3): the host seed search and the host
    align in one call, against the model on the reference's seed records;
    band=None is the verify's path."""
    w = world["main"]
    q, both, per_k = w["cases"][101]
    a = per_k[2][2]
    want = ar.records(a, 4, 8, 3, 3)
    origin, edits, multi, scored = kfmi_mod.map_reads_array(w["idx"][2], q, max_seeds=4, max_occ=8, cpu=True, text=w["text"],
                                                            band=3, max_edits=3)
    none = want[:, 0] == ar.NONE
    assert np.array_equal(origin, np.where(none, -1, want[:, 0].astype(np.int64)))
    assert np.array_equal(edits, np.where(none, 0, want[:, 1] & ar.EDIT_MASK))
    assert np.array_equal(multi, ~none & ((want[:, 1] & ar.MULTI) != 0))
    assert np.array_equal(scored, want[:, 1] >> ar.SCORED_SHIFT)
    assert (~none).any() and none.any() and multi.any()
    plain = kfmi_mod.map_reads_array(w["idx"][2], q, max_seeds=4, max_occ=8, max_mism=3, cpu=True, text=w["text"])
    wantv = vr.records(a.c, 4, 8, 3)
    assert np.array_equal(plain[0], np.where(wantv[:, 0] == vr.NONE, -1, wantv[:, 0].astype(np.int64)))
    assert (origin >= 0).sum() > (plain[0] >= 0).sum()          # the indel reads are placed now


def test_align_clean_under_asan(tmp_path):
    """tests/asan/align_asan.c with csrc/host/*.c under -fsanitize=address,undefined:
    a stand-alone program, the HIP layer stubbed."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    out = tmp_path / "align_asan"
    srcs = sorted(str(p) for p in (util.PKG / "csrc" / "host").glob("*.c"))
    cmd = ["gcc", "-g", "-O1", "-std=gnu11", "-fopenmp", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(out), str(util.REPO / "tests" / "asan" / "align_asan.c")] + srcs
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4")
    p = subprocess.run([str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK"), p.stdout[-2000:] + p.stderr[-4000:]


def planned_dp_cases() -> dict:
    """The cases tests/asan/align_dp_host.cpp says it runs, counted here from its
    header's description and not from its loops."""
    kinds, bands = 6, 16
    sweep_n, sweep_m, pin_m = (40, 257, 300, 303, 320), (1, 2, 15, 16, 17, 33, 100, 128, 129, 255, 256), (17, 100, 129, 256)
    fits = lambda m, k: 3 * k <= m                                       # noqa: E731
    beside = lambda w: 1 + (w > 1) + (w < 15)                            # noqa: E731  the band and the bands beside it
    return {
        "sweep": kinds * sum(sum(m <= n for m in sweep_m) for n in sweep_n) * bands * (16 + 16 + 8),
        "ends": kinds * 2 * bands * sum(32 * len(ar.pinned(m)) * 2 for m in pin_m),
        "edge": kinds * 3 * len(pin_m) * 15 * 3 * 2,
        "indel": kinds * 3 * sum(3 * beside(w) * 2 for m in pin_m for w in range(1, 16) for k in (w, w + 1) if fits(m, k)),
        "leave": kinds * 3 * sum(3 * beside(w) for m in pin_m for w in range(1, 16) if fits(m, w + 1)),
        "comeback": kinds * 3 * sum(3 * beside(w) for m in pin_m for w in range(1, 16) if fits(m, w + 1)),
    }


def test_dp_header_equals_the_definition_under_asan(tmp_path):
    """tests/asan/align_dp_host.cpp: csrc/hip/kfmi_align_dp.h compiled for the
    host under -fsanitize=address,undefined, band_rows<8>, band_rows<16> and
    band_fold against a plain full-table DP on low-complexity texts, every
    band, both text ends, band-edge placements and indels of w and w + 1 bases.
    A stand-alone program; every family must have run its planned cases."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = tmp_path / "align_dp_host"
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(out), str(util.REPO / "tests" / "asan" / "align_dp_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = dict(ln.split() for ln in p.stdout.strip().splitlines())
    plan = planned_dp_cases()
    assert plan["sweep"] >= 185_280
    for family, want in plan.items():
        assert int(lines[family]) >= want, (family, lines[family], want)
    assert int(lines["OK"]) >= sum(plan.values()), (lines["OK"], plan)
