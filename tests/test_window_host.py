"""Place windows / pairs on the host (kstep_fmi.h, "place windows / pairs"), no
GPU needed:

* tests/asan/window_dp_host.cpp: the kernel's own arithmetic (csrc/hip/
  kfmi_window_dp.h compiled for the host: match words, the column step, the
  fold, the scan bound) equals a plain table out to the text's end under
  AddressSanitizer + UBSan, and ran the cases its header plans;
* the non-vacuity conditions hold on the model alone (window_ref.world,
  short_case and pair_table assert them before any library call);
* kfmi_place_windows_cpu equals the model of window_ref.py bit for bit -- four
  texts, every length, every window kind, every strand mode, max_edits in {0,
  1, 8, m}, a text shorter than the reads, the batch the GPU test uses;
* kfmi_mate_windows_cpu and kfmi_pair_hits_cpu equal the model on the
  hand-made table and on windows clipped at 0 and at n, modes 0 and 1 (the
  simulated pairs are in test_pairs_host.py);
* the refusals return 33 and leave a 0xA5A5A5A5 fill intact;
* the header's and the binding's symbols are there."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import seed_ref as sr
import util
import verify_ref as vr
import window_ref as wr

FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def world():
    return wr.world()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        t = int(np.argwhere(got != want)[0][0])
        raise AssertionError((what, "task", t, "got", [hex(int(v)) for v in got[t]], "want", [hex(int(v)) for v in want[t]]))


def host_place(K, text, q, strands, win, me):
    """kfmi_place_windows_cpu on fresh handles: the records, [T, 2]."""
    T = (2 if strands == sr.BOTH else 1) * q.shape[0]
    Q, W, H = K.Queries.from_array(q), K.Results.alloc(T), K.Results.alloc(T)
    try:
        W.array()[:] = np.asarray(win, np.uint32).reshape(-1)
        H.array()[:] = FILL
        K.place_windows_cpu(text, Q, W, H, strands, me)
        assert np.array_equal(W.array().reshape(T, 2), np.asarray(win, np.uint32))      # the windows are read only
        return H.array().copy().reshape(T, 2)
    finally:
        for h in (Q, W, H):
            h.close()


def host_records(K, call, arrays, *args):
    """A record call of the host on fresh handles filled from `arrays`, the last handle the output."""
    n = np.asarray(arrays[0]).reshape(-1, 2).shape[0]
    hs = [K.Results.alloc(n) for _ in range(len(arrays) + 1)]
    try:
        for h, a in zip(hs, arrays):
            h.array()[:] = np.asarray(a, np.uint32).reshape(-1)
        hs[-1].array()[:] = FILL
        call(*hs, *args)
        return hs[-1].array().copy().reshape(n, 2)
    finally:
        for h in hs:
            h.close()


def host_mate(K, n, hits, m, lo, hi, mode):
    return host_records(K, lambda h, w, *a: K.mate_windows_cpu(n, h, w, *a), [hits], m, lo, hi, mode)


def host_pair(K, hits, resc, m, lo, hi):
    return host_records(K, K.pair_hits_cpu, [hits, resc], m, lo, hi)


@pytest.mark.parametrize("text", list(wr.texts()))
def test_place_equals_the_model(kfmi_mod, world, text):
    K, x = kfmi_mod, world[text]
    checked = 0
    for m, (q, tasks, win, tags, b) in x["cases"].items():
        for st in (sr.BOTH, sr.FWD, sr.REV):
            rows = vr.strand_rows(st)
            for me in wr.edit_bounds(m) if st == sr.BOTH else (8,):
                got = host_place(K, x["text"], q, st, win[rows], me)
                same(got, wr.place(b, win[rows], me, rows), (text, m, st, me))
                checked += got.shape[0]
                assert (got[:, 1] >> 20 == 0).all()
    assert checked > 4_000


def test_place_on_a_text_shorter_than_the_reads(kfmi_mod):
    K = kfmi_mod
    t, w, q, tasks, win, b = wr.short_case()
    for me in (0, 43, 57, 100):
        same(host_place(K, t, q, sr.BOTH, win, me), wr.place(b, win, me), ("short", me))


def test_place_on_the_batch(kfmi_mod, world):
    K, x = kfmi_mod, world["n1009"]
    q, tasks, win, b = wr.batch_case(x)
    for me in (3, 100):
        same(host_place(K, x["text"], q, sr.BOTH, win, me), wr.place(b, win, me), ("batch", me))


def test_low_complexity_texts(kfmi_mod):
    """all-A, CG.. and ACT..: every begin position ties or nearly does; windows all over the text."""
    K = kfmi_mod
    for name, t in wr.low_texts().items():
        w = vr.World(t)
        rng = np.random.default_rng(71_000)
        for m in (17, 100, 129):
            o = rng.integers(0, w.n - m, size=24)
            q = np.stack([t[a:a + m] for a in o])
            q[1::3, m // 2] = ord("G") if name != "cg" else ord("A")
            q[2::3] = np.stack([wr.deleted(t, int(a), m, m // 3, 2) for a in o[2::3]])
            q = np.ascontiguousarray(q)
            tasks = sr.tasks_of(q, sr.BOTH)
            T = tasks.shape[0]
            win = np.stack([(o.repeat(2) + np.arange(T) * 7) % (w.n + 1), 1 + (np.arange(T) * 53) % 120], axis=1).astype(np.uint32)
            b = wr.Begins(w, tasks)
            for me in (0, 2, m):
                got = host_place(K, t, q, sr.BOTH, win, me)
                same(got, wr.place(b, win, me), (name, m, me))
            assert ((got[:, 1] & wr.MULTI) != 0).any()


def test_pair_table(kfmi_mod):
    K = kfmi_mod
    hits, resc, names, want = wr.pair_table()
    got = host_pair(K, hits, resc, 100, 200, 400)
    for p, name in enumerate(names):
        same(got[4 * p:4 * p + 4], want[4 * p:4 * p + 4], name)


def clip_hits(n: int, m: int = 100):
    """Hits whose mate windows are clipped at 0 and at n, lie wholly outside the text, or are whole."""
    N = (wr.NONE, 0)
    rows = [[(n - 200, 0), N, N, (150, 0)],          # task 0 from B = 150: [-150, 50] clipped at 0; task 3 from n - 200: clipped at n
            [N, (20, 1), (n - 50, 2), N],            # task 2 from B = 20: [-280, -80], task 1 from n - 50: [n + 50, ..]: nothing left
            [(n, 0), N, N, N],                       # task 3 from B = n: nothing left of [n + 100, n + 300]
            [(100, 0), N, N, (300, 0)],              # concordant: mode 0 writes (0, 0) for both, mode 1 the whole windows
            [(100, 0), (900, 3), (100, 0), (300, 0)]]
    return np.asarray([r for p in rows for r in p], np.uint32)


def test_mate_windows(kfmi_mod):
    K = kfmi_mod
    n = 1_009
    hits = clip_hits(n)
    seen = set()
    for mode in (0, 1):
        want = wr.mate_windows(hits, n, 100, 200, 400, mode)
        same(host_mate(K, n, hits, 100, 200, 400, mode), want, ("clip", mode))
        lo, ln = want[:, 0].astype(np.int64), want[:, 1].astype(np.int64)
        seen |= {"at 0" for t in range(len(lo)) if ln[t] and lo[t] == 0 and ln[t] < 201}
        seen |= {"at n" for t in range(len(lo)) if ln[t] and lo[t] + ln[t] - 1 == n and ln[t] < 201}
        seen |= {"whole" for t in range(len(lo)) if ln[t] == 201}
    assert seen == {"at 0", "at n", "whole"}
    assert (wr.mate_windows(hits, n, 100, 200, 400, 0)[[12, 15], 1] == 0).all()
    assert (wr.mate_windows(hits, n, 100, 200, 400, 1)[[12, 15], 1] == 201).all()
    # the widest window the calls accept, and fragments of exactly the read length
    for lo_f, hi_f in ((100, 100), (100, 100 + wr.MAX_LEN - 1), (4_000_000_000, 4_000_000_000 + wr.MAX_LEN - 1)):
        same(host_mate(K, n, hits, 100, lo_f, hi_f, 1), wr.mate_windows(hits, n, 100, lo_f, hi_f, 1), (lo_f, hi_f))
    big = hits.copy()
    big[:, 0] = np.where(big[:, 0] == wr.NONE, wr.NONE, 0xFFFFFF00 + (big[:, 0] & 0x7F))     # begin positions near 2^32
    same(host_mate(K, 0xFFFFFFFE, big, 100, 200, 400, 1), wr.mate_windows(big, 0xFFFFFFFE, 100, 200, 400, 1), "near 2^32")


def _code(call):
    try:
        call()
    except Exception as e:                      # KfmiError
        return e.code
    return 0


def test_refusals_write_nothing(kfmi_mod, world):
    K, x = kfmi_mod, world["n1008"]
    q = x["cases"][100][0][:16]
    n = q.shape[0]

    def place(strands, n_w, n_h, lens=None, reads=q):
        Q, W, H = K.Queries.from_array(reads), K.Results.alloc(n_w), K.Results.alloc(n_h)
        try:
            W.array()[:] = 0
            W.array()[1::2] = 33 if lens is None else lens
            H.array()[:] = FILL
            code = _code(lambda: K.place_windows_cpu(x["text"], Q, W, H, strands, 3))
            return code, bool((H.array() != FILL).any())
        finally:
            for h in (Q, W, H):
                h.close()

    assert place(K.STRAND_FWD, n, n) == (0, True)
    assert place(K.STRAND_BOTH, 2 * n, 2 * n, wr.MAX_LEN) == (0, True)
    lens = np.full(n, 33)
    lens[n - 1] = wr.MAX_LEN + 1                     # one entry too long, the last: nothing before it is written either
    assert place(K.STRAND_FWD, n, n, lens) == (33, False)
    for strands, a, b in ((0, n, n), (4, n, n), (1, n + 1, n), (1, n, n - 1), (3, n, n), (2, 2 * n, 2 * n)):
        assert place(strands, a, b) == (33, False), (strands, a, b)
    long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
    assert place(K.STRAND_FWD, n, n, reads=long) == (33, False)

    def records(call, sizes, *args):
        hs = [K.Results.alloc(s) for s in sizes]
        try:
            for h in hs:
                h.array()[:] = FILL
            code = _code(lambda: call(*hs, *args))
            return code, any(bool((h.array() != FILL).any()) for h in hs)
        finally:
            for h in hs:
                h.close()

    mate = lambda h, w, *a: K.mate_windows_cpu(1_008, h, w, *a)   # noqa: E731
    assert records(mate, (8, 8), 100, 200, 400, 0) == (0, True)
    assert records(K.pair_hits_cpu, (8, 8, 8), 100, 200, 400) == (0, True)
    for args in ((100, 99, 400, 0), (100, 300, 299, 0), (100, 200, 200 + wr.MAX_LEN, 0), (100, 200, 400, 2),
                 (0, 200, 400, 0), (257, 300, 400, 0)):
        assert records(mate, (8, 8), *args) == (33, False), args
        if args[3] == 0:
            assert records(K.pair_hits_cpu, (8, 8, 8), *args[:3]) == (33, False), args
    for sizes in ((6, 6), (8, 12), (2, 2)):          # an odd number of reads; handles of two sizes
        assert records(mate, sizes, 100, 200, 400, 0) == (33, False), sizes
    for sizes in ((6, 6, 6), (8, 8, 12), (8, 12, 8)):
        assert records(K.pair_hits_cpu, sizes, 100, 200, 400) == (33, False), sizes


def test_header_symbols_load_through_the_binding(kfmi_mod):
    lib = kfmi_mod.load()
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name, nargs in (("kfmi_place_windows", 6), ("kfmi_place_windows_cpu", 8), ("kfmi_mate_windows", 7),
                        ("kfmi_mate_windows_cpu", 7), ("kfmi_pair_hits", 7), ("kfmi_pair_hits_cpu", 6)):
        assert re.search(r"\bint32_t\s+%s\(" % name, header), name
        f = getattr(lib, name)
        assert len(f.argtypes) == nargs and f.restype is not None
    assert re.search(r"#define\s+KFMI_WINDOW_MAX_LEN\s+4096u\b", header)
    assert re.search(r"#define\s+KFMI_PAIR_PROPER\s+0x00020000u\b", header)
    assert re.search(r"#define\s+KFMI_PAIR_RESCUED\s+0x00040000u\b", header)
    assert (kfmi_mod.WINDOW_MAX_LEN, kfmi_mod.PAIR_PROPER, kfmi_mod.PAIR_RESCUED) == (wr.MAX_LEN, wr.PROPER, wr.RESCUED)
    for name in ("place_windows", "place_windows_cpu", "mate_windows", "mate_windows_cpu", "pair_hits", "pair_hits_cpu",
                 "decode_pairs", "map_pairs_array"):
        assert callable(getattr(kfmi_mod, name))


def test_decode_pairs(kfmi_mod):
    rec = np.asarray([[157, 1 | wr.PROPER], [wr.NONE, 0], [90, 5 | wr.MULTI | wr.PROPER | wr.RESCUED], [7, 2]], np.uint32)
    b, e, multi, proper, rescued = kfmi_mod.decode_pairs(rec)
    assert b.tolist() == [157, -1, 90, 7] and e.tolist() == [1, 0, 5, 2] and multi.tolist() == [False, False, True, False]
    assert proper.tolist() == [True, False, True, False] and rescued.tolist() == [False, False, True, False]


def planned_cases() -> dict:
    """The cases tests/asan/window_dp_host.cpp says it runs, counted from its header's description."""
    ms = (1, 2, 31, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256)
    inst = lambda m: sum(32 * nw >= m for nw in (1, 2, 4, 8))   # noqa: E731
    return {
        "sweep": 4 * 7 * 9 * 3 * sum(inst(m) for m in ms),
        "long": 4 * 5 * 2 * sum(inst(m) for m in ms if m >= 63),
        "short": 4 * 2 * sum(inst(m) for n in (1, 5, 30) for m in ms if m > n),
        "tight": 4 * 3 * sum(inst(m) for m in ms if m >= 33),
    }


def test_dp_header_equals_the_definition_under_asan(tmp_path):
    """A stand-alone program with its own main under -fsanitize=address,undefined."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = tmp_path / "window_dp_host"
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(out), str(util.REPO / "tests" / "asan" / "window_dp_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = dict(ln.split() for ln in p.stdout.strip().splitlines())
    plan = planned_cases()
    assert plan == {"sweep": 25_704, "long": 600, "short": 656, "tight": 216}
    for fam, count in plan.items():
        assert int(lines[fam]) == count, (fam, lines)
    assert int(lines["OK"]) == sum(plan.values()), lines
    assert int(lines["hits"]) > sum(plan.values()) // 2, lines
