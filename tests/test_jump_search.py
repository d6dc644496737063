"""Searches with the text jump (DESIGN.md 5a'') equal the CPU oracle and the
pure walk (set_ftab(0)), bit for bit: every read length from 1 to 272, the
batch edges, reads with one substitution in every phase of the walk and of the
compared window, the text's ends, a long repeat, the threshold on both sides,
with the skip table and without it.

That the reads take the jump is asserted on the host from brute force: for an
exact read, `unique_from` gives how many of its last bases make it occur once
in the text, and `jump_point` the K-step at which the kernel then sees one row;
the test requires at least jump_min bases to be left there.
"""
import numpy as np
import pytest

from skip_texts import ACGT

PLAIN = ("task", "task-mid")
N = 3_021                      # n + 1 is no multiple of 64, 192 or 448
NEVER = 1 << 20


def _text():
    rng = np.random.default_rng(5151)
    t = ACGT[rng.integers(0, 4, size=N)]
    t[2_000:2_300] = t[500:800]                                  # a long repeat: two rows to the end
    return t


TEXT = _text()


def unique_from(t):
    """u[e] = fewest bases j with t[e-j:e] occurring once in t (NEVER if none up to 30:
    a base-4 number of 30 digits still fits an int64)."""
    code = np.searchsorted(ACGT, t).astype(np.int64)
    u = np.full(t.size + 1, NEVER, dtype=np.int64)
    for j in range(1, 31):
        h = np.zeros(t.size - j + 1, dtype=np.int64)             # h[s] = t[s:s+j] as a base-4 number
        for r in range(j):
            h = h * 4 + code[r:r + h.size]
        _, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
        once = cnt[inv] == 1
        e = np.arange(h.size) + j
        new = once & (u[e] == NEVER)
        u[e[new]] = j
    return u


UNIQ = unique_from(TEXT)


def jump_point(K, k, m, ends, rows=N + 1):
    """(pos, left) per exact read t[e-m:e], e in ends: the first K-step position
    at which the kernel sees it on one row, and the bases left there; pos -1 and
    left 0 when it never does."""
    ends = np.atleast_1d(np.asarray(ends, dtype=np.int64))
    rem = m % k
    steps = (m - rem) // k
    f = 0 if rem else K.ftab_auto_bases(rows, k, 1 << 40) // k  # the remainder table replaces the ftab
    if steps < f:
        f = 0
    u = UNIQ[ends]
    pos = np.maximum(f, -(-np.maximum(u - rem, 0) // k))
    ok = (u <= m) & (pos < steps)
    return np.where(ok, pos, -1), np.where(ok, (steps - pos) * k, 0)


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
    """The CPU oracle on the index's own image; for m % K != 0 the true
    interval, which is the K = 1 oracle's."""
    img = world(1, 64).image() if q.shape[1] % k else world(k, d).image()
    return oracle_mod.search(img, q)[0]


def _same(got, want, what):
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]) // 2)


def _walk(gpu, idx, q, backend):
    gpu.set_ftab(0)
    gpu.set_skip(0)
    gpu.set_jump(0)
    out = gpu.search_array(idx, q, backend)
    gpu.set_ftab("auto")
    gpu.set_skip("auto")
    gpu.set_jump("auto")
    return out


def _exact_ends(m, count, seed, need_left, K, k):
    """Ends e of `count` exact reads t[e-m:e] outside the repeat's reach that
    are on one row with at least need_left bases left (all reads when 0)."""
    rng = np.random.default_rng(seed)
    ends = rng.permutation(np.arange(m, N + 1))
    if need_left:
        ends = ends[jump_point(K, k, m, ends)[1] >= need_left]
        assert ends.size >= count, (m, int(ends.size))
    return np.asarray(ends[:count], dtype=np.int64)


def _reads(ends, m):
    return np.ascontiguousarray(TEXT[(ends - m)[:, None] + np.arange(m)[None, :]])


CASES = [(b, k, d) for b in PLAIN for k in (1, 2) for d in (64,)] + [("task-mid", 2, 192), ("task", 1, 192)]
IDS = [f"{b}-k{k}d{d}" for b, k, d in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_every_length(gpu, oracle_mod, world, backend, k, d):
    """Exact substrings at every m from 1 to 272 with jump_min = 8: from m = 40
    on every read is asserted to reach the jump."""
    idx = world(k, d)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        idx.free_gpu()
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() > 0 and idx.skip_bytes() > 0
        gpu.set_jump_min(8)
        for m in range(1, 273):
            ends = _exact_ends(m, 24, seed=m, need_left=8 if m >= 40 else 0, K=gpu, k=k)
            q = _reads(ends, m)
            got = gpu.search_array(idx, q, backend)
            assert idx.jump_bytes() > 0
            _same(got, _oracle(oracle_mod, world, k, d, q), (m, "jump != oracle"))
            _same(got, _walk(gpu, idx, q, backend), (m, "jump != walk"))
    finally:
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES[:4], ids=IDS[:4])
def test_batch_edges(gpu, oracle_mod, world, backend, k, d):
    idx = world(k, d)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        ends = _exact_ends(100, 1_000, seed=7, need_left=64, K=gpu, k=k)
        q = _reads(ends, 100)
        want = _oracle(oracle_mod, world, k, d, q)
        _same(_walk(gpu, idx, q, backend), want, "walk != oracle")
        for num in (1, 63, 64, 65, 255, 256, 257, 1_000):
            got = gpu.search_array(idx, q[:num], backend)
            assert idx.jump_bytes() > 0
            _same(got, want[:2 * num], num)
    finally:
        _defaults(gpu)


def _mutate(q, col, rng):
    out = q.copy()
    rows = np.arange(q.shape[0])
    out[rows, col] = ACGT[(np.searchsorted(ACGT, out[rows, col]) + rng.integers(1, 4, size=q.shape[0])) % 4]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [0, "auto"], ids=["skip-off", "skip-on"])
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_substitutions_ends_repeat_and_threshold(gpu, oracle_mod, world, backend, k, d, skip):
    """m = 100 and 150 (the 8- and the 16-word kernel).  One substitution per
    read in the ftab's bases, the narrowing steps, the first, the last and the
    17th / 16th base of the compared window (a word boundary of it); reads at
    both ends of the text, one that would start before position 0, reads inside
    the repeat; jump_min at the commonest remaining length and one step to
    either side.  With the skip table and, under set_jump(1), without it.
    The jump_min cases check results only: a jump returns what the walk returns,
    so they hold that both sides of the threshold are exact, not on which side
    of it a lane jumps -- the kernel's `>= jump_min` itself is held by
    tests/test_walk_trace.py, from the kernel's own records."""
    idx = world(k, d)
    rng = np.random.default_rng(77 + k)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        for m in (100, 150):
            ends = _exact_ends(m, 96, seed=m + k, need_left=64, K=gpu, k=k)
            base = _reads(ends, m)
            left = jump_point(gpu, k, m, ends)[1]
            assert (left >= 64).all()
            first = left - 1                                     # read column of the window's first base
            f_bases = gpu.ftab_auto_bases(N + 1, k, 1 << 40)
            uniq = UNIQ[ends]
            parts = [base,
                     _mutate(base, np.full(96, m - 1 - f_bases // 2), rng),          # inside the ftab's bases
                     _mutate(base, m - np.maximum(uniq - 1, f_bases + 1), rng),      # a narrowing step (or the next)
                     _mutate(base, first, rng), _mutate(base, np.zeros(96, dtype=np.int64), rng),
                     _mutate(base, first - 16, rng), _mutate(base, first - 15, rng),
                     _mutate(base, first - 31, rng), _mutate(base, first - 32, rng)]
            edge = [TEXT[:m], TEXT[N - m:], TEXT[1:m + 1], TEXT[N - m - 1:N - 1]]    # both ends of the stream
            for cut in (1, 2, 3, 4, 17):                         # would start `cut` bases before position 0
                edge.append(np.concatenate([ACGT[rng.integers(0, 4, size=cut)], TEXT[:m - cut]]))
            for s in (500, 560, 800 - m, 2_000, 2_300 - m):      # inside the repeat: two rows to the end
                edge.append(TEXT[s:s + m])
            parts.append(np.stack(edge))
            q = np.ascontiguousarray(np.concatenate(parts))
            assert (jump_point(gpu, k, m, [m, N, m + 1, N - 1])[1] >= 64).all()     # the edge reads reach the jump
            assert (jump_point(gpu, k, m, [560 + m, 2_300])[0] == -1).all()         # and the repeat's never do
            want = _oracle(oracle_mod, world, k, d, q)
            _same(_walk(gpu, idx, q, backend), want, (m, "walk != oracle"))
            common = int(np.bincount(left).argmax())
            for jmin in (64, common - k, common, common + k, 1):
                gpu.set_jump_min(jmin)
                if skip == 0:                                    # jump on, skip off: only the explicit setting
                    gpu.set_skip(0)
                    gpu.set_jump(1)
                    assert gpu.jump_in_effect() == 1 and gpu.skip_in_effect() == 0
                got = gpu.search_array(idx, q, backend)
                assert idx.jump_bytes() > 0, (m, jmin)
                _same(got, want, (m, jmin, skip))
                gpu.set_skip("auto")
                gpu.set_jump("auto")
            gpu.set_jump_min(gpu.JUMP_MIN_DEFAULT)
    finally:
        _defaults(gpu)


@pytest.mark.gpu
def test_stream_and_group(gpu, oracle_mod, world):
    idx = world(2, 64)
    try:
        _defaults(gpu)
        gpu.set_backend("task-mid")
        ends = _exact_ends(100, 700, seed=9, need_left=64, K=gpu, k=2)
        q = _reads(ends, 100)
        want = _oracle(oracle_mod, world, 2, 64, q)
        idx.free_gpu()
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() > 0
        _same(gpu.search_stream(idx, q, chunk=300), want, "stream")
        gpu.set_devices([0, 0])
        _same(gpu.search_array(idx, q, "task-mid"), want, "group")
        assert idx.jump_bytes() > 0
    finally:
        _defaults(gpu)
        idx.free_gpu()
