"""Searches that take their text window and ISA entry from the line table
(DESIGN.md 5a''') equal the CPU oracle and the same search under
set_jump_lines(0), bit for bit, where this kernel can go wrong: window ends at
every residue of a line, both ends of the text, windows on both sides of the
longest one a line serves (W = 240 bases) inside one wave, one substitution at
either end of the window and at the dword boundaries next to them, a long
repeat, the batch edges, with the skip table and without it, and every issue
form of the loads (set_jump_lines(1 | 2) under set_split_class(0 | 4)).

No result shows which form a lane took, so the host asserts from brute force
what decides it: every exact read reaches one row with at least jump_min bases
left, and how many are left there (`left_at_jump`).  What the kernel did with
them is held by tests/test_walk_trace.py, from the kernel's own records; the
windows test below also asks the trace that each exact read jumped with
exactly `left_at_jump` bases left, from a line up to W bases and from the flat
tables beyond.
"""
import numpy as np
import pytest

from skip_texts import ACGT
from test_jump_search import NEVER, unique_from

N = 4_096
W = 240
JMIN = 8


def _text():
    rng = np.random.default_rng(6262)
    t = ACGT[rng.integers(0, 4, size=N)]
    t[3_000:3_300] = t[500:800]                                  # a long repeat: two rows to the end
    return t


TEXT = _text()
UNIQ = unique_from(TEXT)
CASES = [("task", 1, 64), ("task-mid", 1, 64), ("task", 2, 64), ("task-mid", 2, 64), ("task-mid", 2, 192)]
IDS = [f"{b}-k{k}d{d}" for b, k, d in CASES]


def left_at_jump(K, k, m, ends, ftab):
    """Bases left when the kernel first sees the exact read TEXT[e-m:e] on one
    row, per e in ends; 0 when it never does.  ftab: the jump start in effect."""
    ends = np.atleast_1d(np.asarray(ends, dtype=np.int64))
    rem = m % k
    steps = (m - rem) // k
    f = K.ftab_auto_bases(N + 1, k, 1 << 40) // k if ftab and not rem else 0
    if steps < f:
        f = 0
    u = UNIQ[ends]
    pos = np.maximum(f, -(-np.maximum(u - rem, 0) // k))
    return np.where((u <= m) & (pos < steps), (steps - pos) * k, 0)


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    kfmi_mod.set_devices([])
    yield kfmi_mod
    _defaults(kfmi_mod)


def _defaults(K):
    K.set_devices([])
    K.set_split_class(0)
    K.set_jump_min(K.JUMP_MIN_DEFAULT)
    K.set_jump_lines(1)
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.fixture(scope="module")
def world(gpu):
    cache = {}

    def index(k, d):
        if (k, d) not in cache:
            cache[(k, d)] = gpu.Index.build(TEXT.tobytes(), k=k, d=d)
        return cache[(k, d)]

    yield index
    for i in cache.values():
        i.close()


def _oracle(oracle_mod, world, k, d, q):
    img = world(1, 64).image() if q.shape[1] % k else world(k, d).image()
    return oracle_mod.search(img, q)[0]


def _same(got, want, what):
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]) // 2)


def _reads(starts, m):
    return np.ascontiguousarray(TEXT[np.asarray(starts, dtype=np.int64)[:, None] + np.arange(m)[None, :]])


def _clear_starts(m, count, rng):
    """Starts of reads that end clear of both copies of the repeat."""
    e = np.concatenate([np.arange(m, 480), np.arange(840, 2_990)])
    return rng.permutation(e)[:count] - m


def _mutate(q, col, rng):
    out = q.copy()
    rows = np.arange(q.shape[0])
    out[rows, col] = ACGT[(np.searchsorted(ACGT, out[rows, col]) + rng.integers(1, 4, size=q.shape[0])) % 4]
    return out


def _settings(gpu, ftab, skip):
    """ftab on: every table by the auto settings, or the jump alone on the
    skip-less walk; ftab off: the explicit jump with or without the skip table."""
    gpu.set_ftab("auto" if ftab else 0)
    if ftab and skip:
        gpu.set_skip("auto")
        gpu.set_jump("auto")
        assert gpu.jump_in_effect() == 2
    else:
        gpu.set_skip(1 if skip else 0)
        gpu.set_jump(1)
        assert gpu.jump_in_effect() == 1


def _all_forms(gpu, idx, q, backend, want, what, nums=None):
    """Lines off, on, and on with the window's loads never split, each in the
    small tables' form and in the forced form of tables past the translation
    reach (set_split_class(4): with lines = 1 and reads of up to 192 bases
    every load of the round trip goes out per 16-lane group; longer reads take
    the flat tables' form there, by the library's read-length rule, so for them
    this combination repeats lines = 0), against `want`; lines off first, so
    `want` (the oracle) also vouches for the form the others are compared with."""
    for lines in (0, 1, 2):
        gpu.set_jump_lines(lines)
        for cls in (0, 4):
            gpu.set_split_class(cls)
            for num in nums or (q.shape[0],):
                got = gpu.search_array(idx, q[:num], backend)
                assert idx.jump_line_bytes() > 0
                _same(got, want[:2 * num], (what, "lines", lines, "class", cls, "reads", num))
    gpu.set_split_class(0)
    gpu.set_jump_lines(1)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_every_residue_and_both_ends(gpu, oracle_mod, world, backend, k, d):
    """Reads starting at 16 consecutive text positions -- the window's end e is
    n - start, so every dword of a line's ISA half and every shift of its text
    half -- from the text's first base (e = n, the last line), up to its last
    (the first lines), and from inside; a read that would begin before position
    0; lengths on both kernels and up to the longest fused read."""
    idx = world(k, d)
    rng = np.random.default_rng(31 + k)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.set_jump_min(JMIN)
        for m in (40, 99, 100, 128, 129, 150, 200, 247, 248, 256):
            starts = np.concatenate([np.arange(16), np.arange(N - m - 15, N - m + 1), 1_000 + np.arange(16),
                                     2_041 + np.arange(16)])
            left = left_at_jump(gpu, k, m, starts + m, ftab=True)
            assert (left >= JMIN).all(), (m, int(left.min()))
            edge = [np.concatenate([ACGT[rng.integers(0, 4, size=cut)], TEXT[:m - cut]]) for cut in (1, 2, 15, 16, 17)]
            q = np.ascontiguousarray(np.concatenate([_reads(starts, m), np.stack(edge)]))
            want = _oracle(oracle_mod, world, k, d, q)
            for skip in (True, False):
                _settings(gpu, True, skip)
                _all_forms(gpu, idx, q, backend, want, (m, skip))
    finally:
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [False, True], ids=["skip-off", "skip-on"])
@pytest.mark.parametrize("backend,k,d", CASES[1:4], ids=IDS[1:4])
def test_windows_around_W_in_one_wave(gpu, oracle_mod, world, backend, k, d, skip):
    """Without a jump start the rows of this text become unique after 6 to 10
    bases, so reads of about 248 bases jump with W - 2 .. W + 2 bases left:
    lanes of both forms in one wave, asserted from brute force.  Exact reads,
    and reads with a substitution at either end of the window."""
    idx = world(k, d)
    rng = np.random.default_rng(41 + k)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.set_jump_min(JMIN)
        seen = set()
        for m in range(244, 253):
            starts = _clear_starts(m, 64, rng)
            left = left_at_jump(gpu, k, m, starts + m, ftab=False)
            assert (left >= JMIN).all(), (m, int(left.min()))
            seen |= set(int(x) for x in left)
            if 248 <= m <= 249:
                assert (left <= W).any() and (left > W).any(), (m, sorted(set(left.tolist())))
            base = _reads(starts, m)
            q = np.ascontiguousarray(np.concatenate([base, _mutate(base, left - 1, rng), _mutate(base, left - 2, rng),
                                                     _mutate(base, np.zeros(64, dtype=np.int64), rng)]))
            want = _oracle(oracle_mod, world, k, d, q)
            _settings(gpu, False, skip)
            _all_forms(gpu, idx, q, backend, want, (m, skip))
            got, rec = gpu.search_trace(idx, base, backend)      # lines 1, class 0: what the kernel did
            _same(got, want[:2 * 64], (m, skip, "trace"))
            did = gpu.decode_trace(rec)
            assert (did["jump_outcome"] == 0).all() and np.array_equal(did["jump_nb"], left), (m, skip)
            assert np.array_equal(did["jump_line"], (left <= W).astype(np.int64)), (m, skip)
        assert set(range(W - 2, W + 3, k)) <= seen, sorted(seen)
    finally:
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [False, True], ids=["skip-off", "skip-on"])
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_substitutions_repeat_and_batch_edges(gpu, oracle_mod, world, backend, k, d, skip):
    """One substituted base per read: at the window's first and last base --
    the bases nearest the two ends of the line's text half, whose last slot is
    at most 15 past the window's -- one base inside either of them, and on both
    sides of the dword boundaries nearest either end (read column c lies in
    slot n - start - c - 1).  Reads inside the repeat never reach one row.
    Batches of 1, 63, 64, 65 and 257 reads."""
    idx = world(k, d)
    rng = np.random.default_rng(51 + k)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.set_jump_min(JMIN)
        for m in (100, 150, 250):
            starts = _clear_starts(m, 48, rng)
            left = left_at_jump(gpu, k, m, starts + m, ftab=True)
            assert (left >= 64).all(), (m, int(left.min()))
            base = _reads(starts, m)
            hi = (N - starts - 1) % 16                           # column in slot = 0 mod 16, next to the window's start
            lo = left - 1 - (15 - (N - starts - left) % 16)      # column in slot = 15 mod 16, next to its end
            cols = [np.zeros(48, dtype=np.int64), np.ones(48, dtype=np.int64), left - 1, left - 2, hi, hi + 1, lo, lo - 1,
                    left, left + 1]                              # the last two: past the window, in the steps taken
            for c in cols:
                assert (c >= 0).all() and (c < m).all()
            rep = _reads([500, 560, 800 - m, 3_000, 3_300 - m], m)
            assert (left_at_jump(gpu, k, m, [800, 3_300], ftab=True) == 0).all()
            q = np.ascontiguousarray(np.concatenate([base] + [_mutate(base, c, rng) for c in cols] + [rep]))
            want = _oracle(oracle_mod, world, k, d, q)
            _settings(gpu, True, skip)
            _all_forms(gpu, idx, q, backend, want, (m, skip), nums=(q.shape[0], 1, 63, 64, 65, 257))
    finally:
        _defaults(gpu)
