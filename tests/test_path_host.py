"""Align paths on the host (kstep_fmi.h, "align paths"), no GPU needed:

* tests/asan/path_dp_host.cpp: the kernel's own arithmetic (csrc/hip/
  kfmi_path_dp.h compiled for the host: the row step that keeps its rows, the
  value of a cell from the deltas, the walk over the kept rows) equals a plain
  full-table DP and walk under AddressSanitizer + UBSan, and ran the cases its
  header plans;
* the non-vacuity conditions hold on the model alone (path_ref.world asserts
  them before any library call);
* kfmi_align_paths_cpu equals the model of path_ref.py bit for bit on `paths`
  and on every word of `cigars` -- six texts, every length, bands 0, 1, 3, 8,
  15, every strand mode, the align step's hits and caller-filled ones,
  max_edits in {0, 1, m}, C in {1, 2, 32};
* the header's sum and replay properties hold on every record, and D <= E for
  the align step's hits with E <= w and B + m <= n;
* with band 0 every path is m diagonal ops and D the Hamming count;
* the refusals return 33 and leave a 0xA5A5A5A5 fill intact;
* the header's and the binding's symbols are there."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import path_ref as pr
import seed_ref as sr
import util
import verify_ref as vr

FILL = 0xA5A5A5A5
ENTRIES = (1, 2, 32)


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    return pr.world(kfmi_mod, oracle_mod)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        t = int(np.argwhere(got != want)[0][0])
        raise AssertionError((what, "task", t, "got", [hex(int(v)) for v in got[t]], "want", [hex(int(v)) for v in want[t]]))


class Host:
    """The reads of one strand mode and a hits handle on the host; paths() runs kfmi_align_paths_cpu on them."""

    def __init__(self, K, text, q, strands):
        self.K, self.text, self.strands = K, text, strands
        self.T = (2 if strands == sr.BOTH else 1) * q.shape[0]
        self.Q, self.H = K.Queries.from_array(q), K.Results.alloc(self.T)

    def paths(self, B, band, me, C):
        h = self.H.array().reshape(self.T, 2)
        h[:, 0], h[:, 1] = B, FILL                     # only word x is read
        P, G = self.K.Results.alloc(self.T), self.K.Results.alloc(self.T * C)
        try:
            P.array()[:] = FILL
            G.array()[:] = FILL
            self.K.align_paths_cpu(self.text, self.Q, self.H, P, G, self.strands, band, me, C)
            return P.array().copy().reshape(self.T, 2), G.array().copy().reshape(self.T, 2 * C)
        finally:
            P.close()
            G.close()

    def close(self):
        self.Q.close()
        self.H.close()


def cuts(m: int):
    """(max_edits, C) pairs: every bound at C = 2, every C at the bound m."""
    return [(me, 2) for me in (0, 1, m)] + [(m, C) for C in ENTRIES if C != 2]


@pytest.mark.parametrize("text", ["main", "n1005", "n1008", "n1009", "allA", "tandem"])
def test_host_equals_the_model(kfmi_mod, world, text):
    K, x = kfmi_mod, world[text]
    checked = 0
    for label, (m, q, both, per_k) in x["cases"].items():
        ks = x["ks"] if label in (100, 101, "x") else x["ks"][-1:]
        for st in (sr.BOTH, sr.FWD, sr.REV):
            rows = vr.strand_rows(st)
            h = Host(K, x["text"], q, st)
            try:
                for k in ks if st == sr.BOTH else ks[-1:]:
                    for band in pr.BANDS:
                        for kind in ("seed", "hand"):
                            if st != sr.BOTH and (kind == "hand" or band not in (3, 15)):
                                continue
                            B, E, p = pr.walk_of(text, label, k, band, kind)
                            for me, C in cuts(m) if st == sr.BOTH else ((m, 2),):
                                what = (text, label, k, st, band, kind, me, C)
                                got_p, got_c = h.paths(B[rows], band, me, C)
                                want_p, want_c = pr.records(p, me, C, rows)
                                same(got_p, want_p, what + ("paths",))
                                same(got_c, want_c, what + ("cigars",))
                                if me == m:
                                    checked += pr.check_properties(x["world"], both[rows], B[rows], band, got_p, got_c, what)
                            if st == sr.BOTH and E is not None:        # D <= E where the header promises it
                                sure = p.ok & (E >= 0) & (E <= band) & (B + m <= x["world"].n)
                                assert (p.D[sure] <= E[sure]).all(), (text, label, k, band)
                                if band == 0:
                                    assert (p.D[p.ok] == E[p.ok]).all(), (text, label, k, "band 0 is the Hamming count")
            finally:
                h.close()
    assert checked > 1_000


def _call(K, x, q, strands, band, C, n_hits, n_paths, n_cig, text=None):
    """(error code, whether any array changed)."""
    Q = K.Queries.from_array(q)
    hs = [K.Results.alloc(n) for n in (n_hits, n_paths, n_cig)]
    try:
        for h in hs:
            h.array()[:] = FILL
        code = 0
        try:
            K.align_paths_cpu(x["text"] if text is None else text, Q, hs[0], hs[1], hs[2], strands, band, 3, C)
        except K.KfmiError as e:
            code = e.code
        return code, any(bool((h.array() != FILL).any()) for h in hs[1:]), bool((hs[0].array() != FILL).any())
    finally:
        Q.close()
        for h in hs:
            h.close()


def test_refusals_write_nothing(kfmi_mod, world):
    K, x = kfmi_mod, world["n1008"]
    q = x["cases"][100][1][:16]
    n = q.shape[0]
    assert _call(K, x, q, K.STRAND_FWD, 3, 2, n, n, 2 * n) == (0, True, False)      # the hits are read only
    assert _call(K, x, q, K.STRAND_BOTH, 15, 32, 2 * n, 2 * n, 64 * n) == (0, True, False)
    for strands, band, C, a, b, c in (
            (1, 16, 2, n, n, 2 * n), (1, 0xFFFFFFFF, 2, n, n, 2 * n), (1, 3, 0, n, n, n), (1, 3, 33, n, n, 33 * n),
            (0, 3, 2, n, n, 2 * n), (4, 3, 2, n, n, 2 * n), (1, 3, 2, n + 1, n, 2 * n), (1, 3, 2, n, n - 1, 2 * n),
            (1, 3, 2, n, n, 2 * n + 1), (1, 3, 2, n, n, n), (3, 3, 2, n, n, 2 * n), (2, 3, 2, 2 * n, 2 * n, 4 * n)):
        assert _call(K, x, q, strands, band, C, a, b, c) == (33, False, False), (strands, band, C, a, b, c)
    long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
    assert _call(K, x, long, K.STRAND_FWD, 3, 2, n, n, 2 * n) == (33, False, False)
    # a text shorter than the reads is no refusal: every task is without a path
    assert _call(K, x, q, K.STRAND_FWD, 3, 2, n, n, 2 * n, text=x["text"][:50]) == (0, True, False)


def test_header_symbols_load_through_the_binding(kfmi_mod):
    lib = kfmi_mod.load()
    header = (util.REPO / "include" / "kstep_fmi.h").read_text()
    for name, nargs in (("kfmi_align_paths", 9), ("kfmi_align_paths_cpu", 11), ("kfmi_set_path_chunk", 1)):
        assert re.search(r"\bint32_t\s+%s\(" % name, header), name
        f = getattr(lib, name)
        assert len(f.argtypes) == nargs and f.restype is not None
    assert re.search(r"#define\s+KFMI_PATH_OVERFLOW\s+0x80000000u\b", header)
    assert re.search(r"#define\s+KFMI_PATH_MAX_ENTRIES\s+32u\b", header)
    assert (kfmi_mod.PATH_OVERFLOW, kfmi_mod.PATH_RUNS_SHIFT, kfmi_mod.PATH_MAX_ENTRIES) == (pr.OVERFLOW, pr.RUNS_SHIFT, pr.MAX_ENTRIES)
    for name in ("align_paths", "align_paths_cpu", "decode_paths", "cigar_strings", "map_paths_array", "set_path_chunk"):
        assert callable(getattr(kfmi_mod, name))


def test_decode_and_cigar_strings(kfmi_mod):
    paths = np.asarray([[157, 1 | 3 << 16], [pr.NONE, 0], [90, 5 | 11 << 16 | pr.OVERFLOW]], np.uint32)
    cig = np.zeros((3, 4), np.uint32)
    cig[0, :3] = (57 << 4 | 7, 1 << 4 | 8, 42 << 4 | 7)
    end, edits, runs, over = kfmi_mod.decode_paths(paths)
    assert end.tolist() == [157, -1, 90] and edits.tolist() == [1, 0, 5] and runs.tolist() == [3, 0, 11]
    assert over.tolist() == [False, False, True]
    assert kfmi_mod.cigar_strings(paths, cig, 2) == ["57=1X42=", "*", "*"]


def planned_cases() -> int:
    """The cases tests/asan/path_dp_host.cpp says it runs, counted from its header's description."""
    ns, ms = (5, 12, 20, 40, 257, 300, 303, 320), (1, 15, 16, 17, 100, 128, 129, 255, 256)
    return 4 * sum(sum(m <= n for m in ms) for n in ns) * 16 * 32


def test_dp_header_equals_the_definition_under_asan(tmp_path):
    """A stand-alone program with its own main under -fsanitize=address,undefined."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = tmp_path / "path_dp_host"
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(out), str(util.REPO / "tests" / "asan" / "path_dp_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = dict(ln.split() for ln in p.stdout.strip().splitlines())
    assert planned_cases() == 94_208
    assert int(lines["cases"]) == int(lines["OK"]) == planned_cases(), lines
    assert int(lines["paths"]) > planned_cases() // 2, lines
