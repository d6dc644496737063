"""Every reader of a folded jump-start table (DESIGN.md 5a'''') against the CPU
oracle, bit for bit: the forward search with the text jump, the same upload
after set_jump(0) (the no-jump kernel decodes the folded entries), strand
searches, the seed search, reads over 256 bases (the pack path), reads with
m % K != 0 (the remainder table, no jump start), reads shorter than the table's
bases, and the coop kernels' decode.

The lengths run from the table's N bases up past jump_min + N: a lane whose
entry carries a position but has fewer than jump_min bases left must walk on
from [L, L + 1).  Every batch holds, within its first wave, at least 16 exact
reads whose N-mer is unique in the text (one-row entries: folded lanes) and 16
whose N-mer is repeated, asserted from brute force; reads with a substitution
in the window of a folded lane, whose jump fails and whose result is the walk's
own empty interval; and reads that would start before position 0.
"""
import numpy as np
import pytest

import test_jump_search as tjs
from skip_texts import ACGT

TEXT = tjs.TEXT
CASES = [("task", 1, 64), ("task-mid", 2, 64), ("task-mid", 2, 192)]
IDS = [f"{b}-k{k}d{d}" for b, k, d in CASES]


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    kfmi_mod.set_devices([])
    yield kfmi_mod
    _defaults(kfmi_mod)


def _defaults(K):
    tjs._defaults(K)
    K.set_jump_lines(1)
    K.set_ftab_fold(1)
    K.set_ftab_fold_bound(None)


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


def _same(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]) // 2)


def _mutate(q, col, rng):
    out = q.copy()
    rows = np.arange(q.shape[0])
    out[rows, col] = ACGT[(np.searchsorted(ACGT, out[rows, col]) + rng.integers(1, 4, size=q.shape[0])) % 4]
    return out


def batch(m, nb, seed):
    """Reads of m bases for a table of nb bases: 32 exact reads whose last nb
    bases occur once in the text and 32 whose last nb bases are repeated,
    alternating, so that the first wave holds 16 and more of either; then the
    unique ones with a substitution in their first bases (the jump's window
    when one is tried), the repeated ones with one, and reads that would start
    before position 0.  Below nb bases no table is used: any reads do."""
    rng = np.random.default_rng(seed)
    ends = rng.permutation(np.arange(m, tjs.N + 1))
    ends = ends[(ends < 500) | ((ends > 830) & (ends < 2_000)) | (ends > 2_330)]   # outside the long repeat's reach
    reads = lambda e: np.ascontiguousarray(TEXT[(e - m)[:, None] + np.arange(m)[None, :]])
    if m < nb:                                                   # no jump start: any reads
        return np.ascontiguousarray(np.concatenate([reads(ends[:64]), _mutate(reads(ends[:16]), np.zeros(16, dtype=np.int64), rng)]))
    u = tjs.UNIQ[ends]
    uniq, rep = ends[u <= nb][:32], ends[u > nb][:32]
    assert uniq.size == 32 and rep.size == 32, (m, int(uniq.size), int(rep.size))
    first = np.stack([uniq, rep], axis=1).ravel()                # alternating: the first wave holds 32 of each class
    wave = tjs.UNIQ[first[:64]] <= nb
    assert wave.sum() >= 16 and (~wave).sum() >= 16
    parts = [reads(first)]
    if m > nb:
        win = m - nb                                             # the bases left after the table
        for col in sorted({0, win - 1, win // 2}):
            parts.append(_mutate(reads(uniq), np.full(uniq.size, col), rng))
        parts.append(_mutate(reads(rep), np.zeros(rep.size, dtype=np.int64), rng))
    cuts = [c for c in (1, 2, 5) if c < m]
    if cuts:
        parts.append(np.stack([np.concatenate([ACGT[rng.integers(0, 4, size=c)], TEXT[:m - c]]) for c in cuts]))
    return np.ascontiguousarray(np.concatenate(parts))


def lengths(K, k):
    nb = K.ftab_auto_bases(tjs.N + 1, k, 1 << 40)
    jm = K.JUMP_MIN_DEFAULT
    ms = set(range(nb, jm + nb + k + 1, k)) | {100, 150, 200, 272}
    ms |= {nb - k, nb + 1, 101} if k > 1 else {nb - 1}           # shorter than the table; m % K != 0
    return nb, sorted(x for x in ms if x >= 1)


def _oracle(oracle_mod, world, k, d, q):
    img = world(1, 64).image() if q.shape[1] % k else world(k, d).image()
    return oracle_mod.search(img, q)[0]


def _upload_folded(K, idx, backend):
    """A fresh upload under the auto settings: the table is folded."""
    _defaults(K)
    K.set_backend(backend)
    idx.free_gpu()
    K.transfer_to_gpu(idx, None, None)
    assert idx.ftab_entries()[1], "the auto table of this upload is folded"


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_forward_readers_every_length(gpu, oracle_mod, world, backend, k, d):
    """The jump kernel and, after set_jump(0) on the same upload, the no-jump
    kernel; at every length the reads that jump with the entry's position are
    counted from brute force."""
    idx = world(k, d)
    nb, ms = lengths(gpu, k)
    try:
        _upload_folded(gpu, idx, backend)
        saw_short_left = saw_jump = False
        for m in ms:
            q = batch(m, nb, 1000 + m)
            want = _oracle(oracle_mod, world, k, d, q)
            _same(gpu.search_array(idx, q, backend), want, (m, "jump"))
            gpu.set_jump(0)
            _same(gpu.search_array(idx, q, backend), want, (m, "no-jump kernel"))
            gpu.set_jump("auto")
            assert idx.ftab_entries()[1]                          # still the same, folded copy
            if m % k == 0 and m >= nb:
                left = m - nb
                saw_short_left |= 0 < left < gpu.JUMP_MIN_DEFAULT
                saw_jump |= left >= gpu.JUMP_MIN_DEFAULT
        assert saw_short_left and saw_jump
    finally:
        idx.free_gpu()
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_forms_and_batch_edges(gpu, oracle_mod, world, backend, k, d):
    """Both set_jump_lines forms x set_split_class(0 | 4), each on its own upload
    (the class also picks the fold pass's gather form), over the batch edges."""
    idx = world(k, d)
    nb, _ = lengths(gpu, k)
    try:
        for cls in (0, 4):
            _defaults(gpu)
            gpu.set_split_class(cls)
            gpu.set_backend(backend)
            idx.free_gpu()
            gpu.transfer_to_gpu(idx, None, None)
            assert idx.ftab_entries()[1]
            for lines in (0, 1):
                gpu.set_jump_lines(lines)
                for m in (nb + gpu.JUMP_MIN_DEFAULT, 100, 200):
                    q = batch(m, nb, 2000 + m)
                    want = _oracle(oracle_mod, world, k, d, q)
                    for num in (1, 63, 64, 65, q.shape[0]):
                        _same(gpu.search_array(idx, q[:num], backend), want[:2 * num], (cls, lines, m, num))
    finally:
        idx.free_gpu()
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_strand_and_seed_readers(gpu, world, backend, k, d):
    """The strand kernels and the seed walk decode the folded entries: against
    the host's own strand and seed searches."""
    idx = world(k, d)
    nb, ms = lengths(gpu, k)
    try:
        _upload_folded(gpu, idx, backend)
        for m in [x for x in ms if x >= nb]:
            q = batch(m, nb, 3000 + m)
            for strands in (gpu.STRAND_REV, gpu.STRAND_BOTH):
                if m % k == 0:
                    _same(gpu.search_array(idx, q, backend, strands=strands),
                          gpu.search_cpu_array(idx, q, strands=strands), (m, "strands", strands))
            if m <= 256:
                got = gpu.search_seeds_array(idx, q, backend, max_seeds=4)
                want = gpu.search_seeds_array(idx, q, backend, max_seeds=4, cpu=True)
                _same(got[0], want[0], (m, "seed intervals"))
                _same(got[1], want[1], (m, "seed spans"))
        assert idx.ftab_entries()[1]
    finally:
        idx.free_gpu()
        _defaults(gpu)


@pytest.mark.gpu
def test_coop_reader(gpu, oracle_mod, world):
    """The coop kernels go through the same decode.  A coop upload builds no
    text-jump tables, so its own table is never folded; the results equal the
    oracle before and after a task-mid upload of the same handle folded its."""
    k, d = 2, 64
    idx = world(k, d)
    nb, ms = lengths(gpu, k)
    try:
        _upload_folded(gpu, idx, "task-mid")
        for m in [x for x in ms if x % k == 0 and x >= nb]:
            q = batch(m, nb, 4000 + m)
            want = _oracle(oracle_mod, world, k, d, q)
            _same(gpu.search_array(idx, q, "coop-mid"), want, (m, "coop-mid"))
            assert not idx.ftab_entries()[1]
            _same(gpu.search_array(idx, q, "task-mid"), want, (m, "task-mid again"))
            assert idx.ftab_entries()[1]
    finally:
        idx.free_gpu()
        _defaults(gpu)
