"""Searches with the skip table (DESIGN.md 5a') equal the CPU oracle and the
same search under set_skip(0), bit for bit: every task backend, K, d, text,
read length, batch size and setting, with reads that reach the fallback from
every phase of the walk.
"""
import numpy as np
import pytest

from skip_texts import ACGT, texts

PLAIN = ("task", "task-mid")
ALT = ("task-ac", "task-ac-mid")
LENGTHS = (15, 16, 17, 31, 32, 33, 100, 101, 150, 256)
N_READS = 1_024


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
    K.set_ftab_budget(None)
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.fixture(scope="module")
def world(gpu):
    """Indexes built on first use and kept for the module."""
    cache = {}

    def index(name, k, d):
        if (name, k, d) not in cache:
            cache[(name, k, d)] = gpu.Index.build(texts()[name].tobytes(), k=k, d=d)
        return cache[(name, k, d)]

    yield index
    for i in cache.values():
        i.close()


def _reads(t, m, seed):
    """N_READS reads of m bases: sampled from the text (some from the 'dup'
    text's repeated segment); the same with one base changed at each of the
    positions 0, 7, 8, 40, m-17, m-16, m-1 that the length has; the text's
    first 21 windows; reads with N and lowercase bases; random ones."""
    rng = np.random.default_rng(seed)
    win = np.arange(m)[None, :]
    parts = []
    st = rng.integers(0, t.size - m + 1, size=560)
    parts.append(t[st[:, None] + win])
    lo, hi = max(0, 700 - m // 2), min(t.size - m, 1_000)
    st = rng.integers(lo, hi + 1, size=64)                   # across and inside [700, 1000)
    parts.append(t[st[:, None] + win])
    for pos in sorted({0, 7, 8, 40, m - 17, m - 16, m - 1}):
        if not 0 <= pos < m:
            continue
        st = rng.integers(0, t.size - m + 1, size=32)
        mut = t[st[:, None] + win].copy()
        mut[:, pos] = ACGT[(np.searchsorted(ACGT, mut[:, pos]) + rng.integers(1, 4, size=32)) % 4]
        parts.append(mut)
    parts.append(t[np.arange(21)[:, None] + win])            # invalid entries near the text start
    st = rng.integers(0, t.size - m + 1, size=48)
    odd = t[st[:, None] + win].copy()
    odd[:16, rng.integers(0, m)] = ord("N")
    odd[16:32] = np.char.lower(odd[16:32].view("S1")).view(np.uint8)
    odd[32:, rng.integers(0, m, size=3)] = np.frombuffer(b"nRx", np.uint8)
    parts.append(odd)
    q = np.concatenate(parts)
    assert q.shape[0] <= N_READS
    fill = ACGT[rng.integers(0, 4, size=(N_READS - q.shape[0], m))]
    return np.ascontiguousarray(np.concatenate([q, fill]))


def _oracle(oracle_mod, index, name, idx, backend, k, d, q):
    """The CPU oracle on the index's own image (the AltCounters one for those
    backends); for m % K != 0 the true interval, which is the K = 1 oracle's.
    Where (n + 1) % d == 0 the oracle refuses reads whose interval reaches row
    n + 1 (the reference reads past its index there): the plain backends return
    the true interval, which the K = 1 oracle gives on an image with another d;
    the reference defines no AltCounters result there (None: compared with
    set_skip(0) only)."""
    if q.shape[1] % k:
        img = index(name, 1, 64).image()
    elif backend in ALT:
        img = idx.alt_counters()[0].image()
    else:
        img = idx.image()
    try:
        return oracle_mod.search(img, q)[0]
    except ValueError:
        if backend in ALT:
            if (texts()[name].size + 1) % d:
                raise
            return None
        assert (texts()[name].size + 1) % 448
        return oracle_mod.search(index(name, 1, 448).image(), q)[0]


def _same(got, want, what):
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]) // 2)


CASES = [(b, k, d) for b in PLAIN + ALT for k in (1, 2) for d in (64, 192)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned", "plain", "atail", "dup"])
@pytest.mark.parametrize("backend,k,d", CASES, ids=[f"{b}-k{k}d{d}" for b, k, d in CASES])
def test_skip_equals_walk_equals_oracle(gpu, oracle_mod, world, backend, k, d, name):
    t = texts()[name]
    idx = world(name, k, d)
    table = 8 * (t.size + 1)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        idx.free_gpu()                                       # a fresh upload under the auto settings
        for m in LENGTHS:
            q = _reads(t, m, seed=m * 31 + k)
            if backend in ALT and m % k:                     # AltCounters semantics take no remainder
                with pytest.raises(gpu.KfmiError) as e:
                    gpu.search_array(idx, q, backend)
                assert e.value.code == 33, m
                continue
            gpu.set_ftab(0)
            gpu.set_skip(0)
            off = gpu.search_array(idx, q, backend)          # the pure walk of every K-step
            want = _oracle(oracle_mod, world, name, idx, backend, k, d, q)
            if want is not None:
                _same(off, want, (m, "walk != oracle"))
            for what, ftab, skip, split in (("ftab 0, skip on", 0, 1, 0), ("ftab 8, skip on", 8, 1, 0),
                                            ("auto", "auto", "auto", 0), ("auto, split class 4", "auto", "auto", 4)):
                gpu.set_ftab(ftab)
                gpu.set_skip(skip)
                gpu.set_split_class(split)
                for num in (N_READS, 1_003, 1) if what == "auto" else (N_READS,):
                    got = gpu.search_array(idx, q[:num], backend)
                    assert idx.skip_bytes() == table, (m, what)      # a silently absent table cannot pass
                    _same(got, off[:2 * num], (m, what, num))
                gpu.set_split_class(0)
    finally:
        _defaults(gpu)


@pytest.mark.gpu
def test_budget_too_small_leaves_the_table_out(gpu, world):
    t = texts()["plain"]
    idx = world("plain", 2, 64)
    q = _reads(t, 100, seed=3)
    try:
        _defaults(gpu)
        gpu.set_skip(0)
        want = gpu.search_array(idx, q, "task-mid")
        gpu.set_skip("auto")
        for budget, there in ((16 * (t.size + 1) - 1, False), (16 * (t.size + 1), True)):
            idx.free_gpu()
            gpu.set_ftab_budget(budget)
            gpu.transfer_to_gpu(idx, None, None)             # the upload succeeds either way
            assert idx.skip_bytes() == (8 * (t.size + 1) if there else 0), budget
            _same(gpu.search_array(idx, q, "task-mid"), want, budget)
            assert idx.skip_bytes() == (8 * (t.size + 1) if there else 0), budget
    finally:
        _defaults(gpu)


@pytest.mark.gpu
def test_device_group_two_replicas(gpu, world):
    t = texts()["dup"]
    idx = world("dup", 2, 64)
    q = _reads(t, 100, seed=4)
    try:
        _defaults(gpu)
        gpu.set_skip(0)
        want = gpu.search_array(idx, q, "task-mid")
        gpu.set_skip("auto")
        gpu.set_devices([0, 0])
        _same(gpu.search_array(idx, q, "task-mid"), want, "group")
        assert idx.skip_bytes() == 2 * 8 * (t.size + 1)      # one table per member
    finally:
        _defaults(gpu)
        idx.free_gpu()


@pytest.mark.gpu
def test_search_stream(gpu, world):
    t = texts()["plain"]
    idx = world("plain", 2, 64)
    q = _reads(t, 100, seed=5)
    try:
        _defaults(gpu)
        gpu.set_backend("task-mid")
        gpu.set_skip(0)
        want = gpu.search_array(idx, q, "task-mid")
        gpu.set_skip("auto")
        idx.free_gpu()
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.skip_bytes() == 8 * (t.size + 1)
        _same(gpu.search_stream(idx, q, chunk=300), want, "stream")
        _same(gpu.search_stream(idx, q), want, "stream, one chunk")
    finally:
        _defaults(gpu)
