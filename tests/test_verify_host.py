"""Verify seeds on the host (kstep_fmi.h, "verify seeds"), no GPU needed:

* kfmi_verify_seeds_cpu equals the model of verify_ref.py bit for bit on both
  words of every record -- four texts, K = 1, 2, eighteen lengths, S in
  {1, 4, 8}, every strand mode, max_occ in {1, 2, 8}, max_mism in {0, 1, m}.
  The seed records it is given are seed_ref.reference's, written into the
  handles' host arrays, so no search of the library stands between the model
  and the function under test; the suffix array it is given is the model's;
* the non-vacuity conditions hold on the model alone (verify_ref.world asserts
  them before any library call);
* hand-made slots: a wide slot cut by max_occ, every ignored-slot form,
  R > rows, rows without a suffix;
* the refusals return 33 and write nothing;
* the header's and the binding's symbols are there;
* tests/asan/verify_asan.c runs clean under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import seed_ref as sr
import util
import verify_ref as vr

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    return vr.world(kfmi_mod, oracle_mod)


def host_hits(K, w, q, iv, sp, s, strands, occ, mm, sa=None):
    """kfmi_verify_seeds_cpu on handles filled with the given records; uint32 [T, 2]."""
    ns = 2 if strands == sr.BOTH else 1
    T = ns * q.shape[0]
    assert iv.shape == (T, s, 2) and sp.shape == (T, s, 2)
    Q, I, S, H = K.Queries.from_array(q), K.Results.alloc(T * s), K.Results.alloc(T * s), K.Results.alloc(T)
    try:
        I.array()[:] = iv.reshape(-1)
        S.array()[:] = sp.reshape(-1)
        H.array()[:] = FILL
        K.verify_seeds_cpu(w.text, (w.sa if sa is None else sa).astype(np.uint32), Q, I, S, H, s, strands, occ, mm)
        return H.array().copy().reshape(T, 2)
    finally:
        for h in (Q, I, S, H):
            h.close()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        t = int(np.argwhere(got != want)[0][0])
        raise AssertionError((what, "task", t, "got", got[t].tolist(), "want", want[t].tolist()))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", list(vr.texts()))
def test_host_equals_the_model(kfmi_mod, world, text, k):
    K, w = kfmi_mod, world[text]
    for m, (q, both, per_k) in w["cases"].items():
        iv, sp, c = per_k[k]
        for strands in vr.STRANDS:
            rows = vr.strand_rows(strands)
            for s in vr.SEEDS:
                ivs, sps = np.ascontiguousarray(iv[rows, :s]), np.ascontiguousarray(sp[rows, :s])
                for occ in vr.OCCS:
                    for mm in vr.mism_bounds(m):
                        got = host_hits(K, w["world"], q, ivs, sps, s, strands, occ, mm)
                        same(got, vr.records(c, s, occ, mm, rows), (text, k, m, strands, s, occ, mm))


def test_repeats_and_shared_origins(world):
    """On the model: a read inside the copied segment has MULTI and the smaller
    origin at max_occ = 2 and the first row's origin without MULTI at
    max_occ = 1."""
    for name, w in world.items():
        src, dst, ln = vr.copy_of(w["text"])
        q, both, per_k = w["cases"][100]
        iv, sp, c = per_k[1]
        two, one = vr.records(c, 8, 2, 0), vr.records(c, 8, 1, 0)
        t = 2 * int(np.flatnonzero((q == w["text"][src + 3:src + 103]).all(axis=1))[0])
        assert two[t, 0] == src + 3 and two[t, 1] & vr.MULTI and (two[t, 1] & vr.MISM_MASK) == 0, (name, two[t])
        assert one[t, 0] in (src + 3, dst + 3) and not one[t, 1] & vr.MULTI and one[t, 1] >> vr.SCORED_SHIFT == 1
        assert one[t, 0] == w["world"].sa[int(iv[t, 0, 0])]


def handmade(w, m=40):
    """Four reads of the text and hand-made slots: (q, iv, sp) at S = 8, FWD."""
    n, rows = w.n, w.n + 1
    q = np.stack([w.text[o:o + m] for o in (0, 7, n - m, 300)])
    iv, sp = np.zeros((4, 8, 2), np.uint32), np.zeros((4, 8, 2), np.uint32)
    iv[0, 0], sp[0, 0] = (0, rows), (0, m)                     # the whole array, cut by max_occ
    iv[0, 1], sp[0, 1] = (5, 0xFFFFFFFF), (3, 9)               # R far past rows
    iv[1, 0], sp[1, 0] = (rows, rows + 5), (0, m)              # L >= rows
    iv[1, 1], sp[1, 1] = (9, 9), (0, m)                        # R <= L
    iv[1, 2], sp[1, 2] = (10, 4), (0, m)
    iv[1, 3], sp[1, 3] = (0, rows), (0, 0)                     # len == 0
    iv[1, 4], sp[1, 4] = (0, rows), (m - 3, 4)                 # start + len > m
    iv[1, 5], sp[1, 5] = (0, rows), (0xFFFFFFFF, 2)            # ... with a start that wraps in 32 bits
    iv[1, 6], sp[1, 6] = (rows - 3, rows + 100), (0, m)        # the last rows, R > rows
    iv[2, 7], sp[2, 7] = (0, 3), (m - 1, 1)                    # only the last slot used; row 0 is the '$' suffix
    iv[3] = (0xFFFFFFFF, 0xFFFFFFFF)                           # garbage everywhere
    sp[3] = (0xFFFFFFFF, 0xFFFFFFFF)
    return np.ascontiguousarray(q), iv, sp


def test_hand_made_slots(kfmi_mod, world):
    w = world["n1005"]["world"]
    q, iv, sp = handmade(w)
    holes = w.sa.copy()
    holes[::3] = 0xFFFFFFFF                                    # rows without a suffix
    for sa in (w.sa, holes):
        for occ in (1, 7, 256):
            c = vr.candidates(w, q, iv, sp, occ, sa=sa)
            assert (c.why == vr.SCORED).any() and (c.why != vr.SCORED).any()
            for mm in (0, 40, 0xFFFFFFFF):
                got = host_hits(kfmi_mod, w, q, iv, sp, 8, sr.FWD, occ, mm, sa=sa)
                same(got, vr.records(c, 8, occ, mm), ("hand-made", occ, mm))
    assert (host_hits(kfmi_mod, w, q, iv, sp, 8, sr.FWD, 256, 40)[:, 1] >> vr.SCORED_SHIFT).max() > 200


def _call(K, w, q, s, strands, occ, n_iv, n_sp, n_hits):
    """(error code, whether any array changed)."""
    Q = K.Queries.from_array(q)
    hs = [K.Results.alloc(n) for n in (n_iv, n_sp, n_hits)]
    try:
        for h in hs:
            h.array()[:] = FILL
        code = 0
        try:
            K.verify_seeds_cpu(w.text, w.sa.astype(np.uint32), Q, hs[0], hs[1], hs[2], s, strands, occ, 3)
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
    assert _call(K, w, q, 3, K.STRAND_FWD, 8, 3 * n, 3 * n, n) == (0, True)
    assert _call(K, w, q, 3, K.STRAND_BOTH, 8, 6 * n, 6 * n, 2 * n) == (0, True)
    for s, strands, occ, a, b, c in ((0, 1, 8, n, n, n), (9, 1, 8, 9 * n, 9 * n, n), (3, 0, 8, 3 * n, 3 * n, n),
                                     (3, 4, 8, 3 * n, 3 * n, n), (3, 1, 0, 3 * n, 3 * n, n), (3, 1, 257, 3 * n, 3 * n, n),
                                     (3, 1, 8, 3 * n - 1, 3 * n, n), (3, 1, 8, 3 * n, 3 * n + 1, n),
                                     (3, 1, 8, 3 * n, 3 * n, n + 1), (3, 1, 8, 3 * n, 3 * n, n - 1),
                                     (3, 3, 8, 3 * n, 3 * n, n), (3, 3, 8, 6 * n, 6 * n, n), (3, 2, 8, 6 * n, 6 * n, 2 * n)):
        assert _call(K, w, q, s, strands, occ, a, b, c) == (33, False), (s, strands, occ, a, b, c)
    long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
    assert _call(K, w, long, 2, K.STRAND_FWD, 8, 2 * n, 2 * n, n) == (33, False)
    # a suffix array that is not the text's n + 1 rows
    Q, hs = K.Queries.from_array(q), [K.Results.alloc(x) for x in (n, n, n)]
    try:
        with pytest.raises(K.KfmiError) as e:
            K.verify_seeds_cpu(w.text, w.sa[:-1].astype(np.uint32), Q, hs[0], hs[1], hs[2], 1, 1, 8, 0)
        assert e.value.code == 33
    finally:
        Q.close()
        for h in hs:
            h.close()


def test_header_symbols_load_through_the_binding(kfmi_mod):
    lib = kfmi_mod.load()
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name, nargs in (("kfmi_verify_seeds", 9), ("kfmi_verify_seeds_cpu", 13)):
        assert re.search(r"\bint32_t\s+%s\(" % name, header), name
        f = getattr(lib, name)
        assert len(f.argtypes) == nargs and f.restype is not None
    for name, value in (("KFMI_HIT_NONE", "0xFFFFFFFFu"), ("KFMI_HIT_MISM_MASK", "0x0000FFFFu"),
                        ("KFMI_HIT_MULTI", "0x00010000u"), ("KFMI_HIT_SCORED_SHIFT", "20"),
                        ("KFMI_VERIFY_MAX_OCC", "256u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), header), name
    assert (kfmi_mod.HIT_NONE, kfmi_mod.HIT_MISM_MASK, kfmi_mod.HIT_MULTI, kfmi_mod.HIT_SCORED_SHIFT,
            kfmi_mod.VERIFY_MAX_OCC) == (vr.NONE, vr.MISM_MASK, vr.MULTI, vr.SCORED_SHIFT, 256)
    for name in ("verify_seeds", "verify_seeds_cpu", "map_reads_array", "decode_hits"):
        assert callable(getattr(kfmi_mod, name))


def test_map_reads_on_the_host(kfmi_mod, world):
    """map_reads_array(cpu=True): the host seed search and the host verify in
    one call, against the model on the reference's seed records."""
    w = world["main"]
    q, both, per_k = w["cases"][101]
    want = vr.records(per_k[2][2], 4, 8, 3)
    origin, mism, multi, scored = kfmi_mod.map_reads_array(w["idx"][2], q, max_seeds=4, max_occ=8, max_mism=3, cpu=True,
                                                           text=w["text"])
    none = want[:, 0] == vr.NONE
    assert np.array_equal(origin, np.where(none, -1, want[:, 0].astype(np.int64)))
    assert np.array_equal(mism, np.where(none, 0, want[:, 1] & vr.MISM_MASK))
    assert np.array_equal(multi, ~none & ((want[:, 1] & vr.MULTI) != 0))
    assert np.array_equal(scored, want[:, 1] >> vr.SCORED_SHIFT)
    assert (~none).any() and none.any() and multi.any()


def test_verify_clean_under_asan(tmp_path):
    """tests/asan/verify_asan.c with csrc/host/*.c under -fsanitize=address,undefined:
    a stand-alone program, the HIP layer stubbed, hand-made slots with garbage."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    out = tmp_path / "verify_asan"
    srcs = sorted(str(p) for p in (util.PKG / "csrc" / "host").glob("*.c"))
    cmd = ["gcc", "-g", "-O1", "-std=gnu11", "-fopenmp", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(out), str(util.REPO / "tests" / "asan" / "verify_asan.c")] + srcs
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4")
    p = subprocess.run([str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("OK"), p.stdout[-2000:] + p.stderr[-4000:]
