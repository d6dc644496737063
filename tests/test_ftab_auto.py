"""The jump-start table as a default: the auto rule, the table
built level by level during the upload, and the searches that use it.

CPU: kfmi_ftab_auto_bases is host arithmetic.  GPU: the default (auto) search
equals the same search under set_ftab(0) and the CPU oracle, bit for bit.
"""
import numpy as np
import pytest

ACGT = np.frombuffer(b"ACGT", np.uint8)
GIB = 1 << 30


def table_bytes(n):
    return 8 * 4 ** n


# --------------------------------------------------------------------------
# CPU: the auto rule
# --------------------------------------------------------------------------

def test_auto_rule_examples(kfmi_mod):
    f = kfmi_mod.ftab_auto_bases
    rows3g = 3_000_000_001
    # 8 * 4^16 B = 32 GiB is a quarter of 128 GiB (137.4 GB) free
    for k in (2, 4):
        assert f(rows3g, k, 128 * GIB // 4) == 16
        assert f(rows3g, k, 1 << 62) == 16                      # never deeper than 16 bases
        assert f(rows3g, k, 128 * GIB // 4 - 1) == 16 - k       # one step down: 14 or 12
        assert f(rows3g, k, table_bytes(16 - k) - 1) == 16 - 2 * k   # two steps down
    assert f(rows3g, 1, 1 << 62) == 16
    assert f(rows3g, 1, table_bytes(16) - 1) == 15
    assert f(rows3g, 3, 1 << 62) == 15                          # the largest multiple of 3
    assert f(rows3g, 3, table_bytes(15) - 1) == 12
    assert f(rows3g, 3, table_bytes(12) - 1) == 9
    # config #1: 64 Mbase, 4^13 <= 2 * rows < 4^14
    assert f(64_000_001, 2, 1 << 62) == 12
    assert f(64_000_001, 1, 1 << 62) == 13
    assert f(64_000_001, 3, 1 << 62) == 12
    assert f(64_000_001, 4, 1 << 62) == 12
    # the 200,001-base text of the GPU tests below
    assert [f(200_002, k, 1 << 62) for k in (1, 2, 3, 4)] == [9, 8, 9, 8]
    # off: tiny indexes, no budget, a budget below the smallest table, K the kernels do not have
    for k in (1, 2, 3, 4):
        for rows in (0, 1, 7):
            assert f(rows, k, 1 << 62) == 0
        assert f(rows3g, k, 0) == 0
        assert f(rows3g, k, table_bytes(k) - 1) == 0
        assert f(rows3g, k, table_bytes(k)) == k
    assert [f(8, k, 1 << 62) for k in (1, 2, 3, 4)] == [2, 2, 0, 0]
    assert f(rows3g, 0, 1 << 62) == 0 and f(rows3g, 5, 1 << 62) == 0


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_auto_rule_is_the_largest_that_fits(kfmi_mod, k):
    rng = np.random.default_rng(k)
    for _ in range(400):
        rows = int(2 ** rng.uniform(3, 32))
        budget = int(2 ** rng.uniform(0, 38))
        n = kfmi_mod.ftab_auto_bases(rows, k, budget)
        assert n % k == 0 and 0 <= n <= 16
        if n:
            assert 4 ** n <= 2 * rows and table_bytes(n) <= budget
        up = n + k
        if up <= 16:                                            # the next one must fail a limit
            assert 4 ** up > 2 * rows or table_bytes(up) > budget, (rows, budget, n)


def test_set_ftab_values(kfmi_mod):
    K = kfmi_mod
    try:
        for v in ("auto", 0, 1, 16, K.FTAB_AUTO):
            K.set_ftab(v)
        for v in (17, 1 << 20):
            with pytest.raises(K.KfmiError) as e:
                K.set_ftab(v)
            assert e.value.code == 33
    finally:
        K.set_ftab("auto")


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------

PLAIN = ("task-mid", "coop-mid", "task")
ALT = ("task-ac", "task-ac-mid")
N_TEXT = 200_001
AUTO_N = {1: 9, 2: 8, 4: 8}


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    yield kfmi_mod
    kfmi_mod.set_ftab_budget(None)
    kfmi_mod.set_ftab("auto")


def _texts():
    rng = np.random.default_rng(716)
    rnd = ACGT[rng.integers(0, 4, size=N_TEXT)]
    # the text's first suffixes sort right after "$": rows 1 .. K, block 0
    dollar0 = rnd.copy()
    dollar0[:24] = ord("A")
    # (n + 1) % d == 0 for d = 64 and d = 192
    aligned = ACGT[rng.integers(0, 4, size=192 * 1042 - 1)]
    return {"random": rnd, "dollar0": dollar0, "aligned": aligned}


@pytest.fixture(scope="module")
def world(gpu):
    """Texts, their indexes (built on first use) and K = 1 images for the oracle."""
    texts = _texts()
    cache = {}

    def index(name, k, d):
        if (name, k, d) not in cache:
            cache[(name, k, d)] = gpu.Index.build(texts[name].tobytes(), k=k, d=d)
        return cache[(name, k, d)]

    yield texts, index
    for i in cache.values():
        i.close()


def _reads(t, m, seed, n=1037):
    """n reads of m bases (a partial wave and a partial workgroup): two thirds
    occur in the text, the others are random (absent from it when m is long)."""
    rng = np.random.default_rng(seed)
    nocc = 2 * n // 3
    st = rng.integers(0, t.size - m + 1, size=nocc)
    occ = t[st[:, None] + np.arange(m)[None, :]]
    return np.ascontiguousarray(np.concatenate([occ, ACGT[rng.integers(0, 4, size=(n - nocc, m))]]))


def _search(gpu, idx, q, backend, ftab):
    gpu.set_ftab(ftab)
    return gpu.search_array(idx, q, backend)


def _oracle(oracle_mod, index, name, idx, backend, k, q):
    """The CPU oracle's intervals: on the index's own image (the AltCounters
    one for those backends), or for m % K != 0 the true interval, which is the
    K = 1 oracle's.  Where (n + 1) % d == 0 the oracle refuses reads whose
    interval reaches row n + 1 (the reference reads past its index there,
    SURVEY B5): the plain backends return the true interval, which the K = 1
    oracle gives on an image of the same text with another d; the reference
    defines no AltCounters result there (None: compared with set_ftab(0) only)."""
    if q.shape[1] % k:
        img = index(name, 1, 64).image()
    elif backend in ALT:
        img = idx.alt_counters()[0].image()
    else:
        img = idx.image()
    try:
        return oracle_mod.search(img, q)[0]
    except ValueError:
        if name != "aligned":
            raise
        if backend in ALT:
            return None
        return oracle_mod.search(index(name, 1, 448).image(), q)[0]


CASES = [(b, k, d) for b in PLAIN + ALT for k in (1, 2) for d in (64, 192)] + [("coop-grp", 4, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "dollar0", "aligned"])
@pytest.mark.parametrize("backend,k,d", CASES, ids=[f"{b}-k{k}d{d}" for b, k, d in CASES])
def test_default_equals_off_equals_oracle(gpu, oracle_mod, world, backend, k, d, name):
    texts, index = world
    t = texts[name]
    idx = index(name, k, d)
    n_auto = gpu.ftab_auto_bases(t.size + 1, k, 1 << 40)
    assert n_auto == AUTO_N[k]
    idx.free_gpu()                                   # a fresh upload under the auto setting
    gpu.set_ftab("auto")
    for m in (n_auto - 1, n_auto, n_auto + k, 100, 101):
        q = _reads(t, m, seed=m * 13 + k)
        if backend in ALT and m % k:                 # AltCounters semantics take no remainder
            for ftab in ("auto", 0):
                with pytest.raises(gpu.KfmiError) as e:
                    _search(gpu, idx, q, backend, ftab)
                assert e.value.code == 33, (m, ftab)
            continue
        got = _search(gpu, idx, q, backend, "auto")
        assert idx.ftab_bytes() == table_bytes(n_auto)
        off = _search(gpu, idx, q, backend, 0)
        assert np.array_equal(got, off), (m, "auto != off", int(np.flatnonzero(got != off)[0]) // 2)
        want = _oracle(oracle_mod, index, name, idx, backend, k, q)
        if want is not None:
            assert np.array_equal(got, want), (m, "auto != oracle", int(np.flatnonzero(got != want)[0]) // 2)
    gpu.set_ftab("auto")


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d,bases", [("coop-grp", 4, 64, 8), ("task-mid", 2, 192, 8), ("task-ac", 1, 64, 9)])
def test_level_wise_table_every_entry(gpu, oracle_mod, world, backend, k, d, bases):
    """Every entry of the auto table, two fresh builds: the `bases`-long read of
    each code searched with the table (one lookup, no step) equals the search
    without it and the oracle's."""
    texts, index = world
    idx = index("random", k, d)
    codes = np.arange(4 ** bases, dtype=np.uint32)
    q = ACGT[(codes[:, None] >> (2 * np.arange(bases - 1, -1, -1))[None, :]) & 3].copy()
    try:
        off = _search(gpu, idx, q, backend, 0)
        want, _ = oracle_mod.search(idx.alt_counters()[0].image() if backend in ALT else idx.image(), q)
        assert np.array_equal(off, want)
        for build in range(2):
            idx.free_gpu()
            got = _search(gpu, idx, q, backend, "auto")
            assert idx.ftab_bytes() == table_bytes(bases)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (backend, build, int(bad.size), int(bad[0] // 2))
    finally:
        gpu.set_ftab("auto")


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["task-mid", "coop-mid"])
def test_budget_steps_the_table_down_or_off(gpu, world, backend):
    texts, index = world
    t = texts["random"]
    idx = index("random", 2, 64)
    q = _reads(t, 100, seed=5)
    try:
        want = _search(gpu, idx, q, backend, 0)
        for budget, bases in ((table_bytes(8) - 1, 6), (table_bytes(6) - 1, 4), (0, 0), (table_bytes(2) - 1, 0),
                              (None, 8)):
            idx.free_gpu()
            gpu.set_ftab_budget(budget)
            got = _search(gpu, idx, q, backend, "auto")      # never an error
            assert idx.ftab_bytes() == (table_bytes(bases) if bases else 0), (budget, bases)
            assert np.array_equal(got, want), budget
    finally:
        gpu.set_ftab_budget(None)
        gpu.set_ftab("auto")


@pytest.mark.gpu
def test_table_bytes_after_upload(gpu, world):
    """The auto table is built by the upload, before any search, and is not
    part of device_bytes(); an upload under set_ftab(0) builds none, and an
    explicit count still builds at the first search."""
    texts, index = world
    idx = index("random", 2, 64)
    try:
        gpu.set_backend("task-mid")
        idx.free_gpu()
        assert idx.ftab_bytes() == 0
        gpu.set_ftab(0)
        gpu.transfer_to_gpu(idx, None, None)
        plain_bytes = idx.device_bytes()
        assert plain_bytes > 0 and idx.ftab_bytes() == 0
        idx.free_gpu()
        gpu.set_ftab("auto")
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.ftab_bytes() == table_bytes(8)
        assert idx.device_bytes() == plain_bytes
        q = _reads(texts["random"], 100, seed=9)
        want = _search(gpu, idx, q, "task-mid", 0)
        assert np.array_equal(_search(gpu, idx, q, "task-mid", 6), want)
        assert idx.ftab_bytes() == table_bytes(8) + table_bytes(6)
        # a device group: one table per member
        gpu.set_ftab("auto")
        gpu.set_devices([0, 0])
        try:
            assert np.array_equal(gpu.search_array(idx, q, "task-mid"), want)
            assert idx.ftab_bytes() == 2 * table_bytes(8)
        finally:
            gpu.set_devices([])
    finally:
        gpu.set_ftab("auto")
