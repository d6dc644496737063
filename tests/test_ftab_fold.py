"""Every entry of the folded jump-start table (DESIGN.md 5a'''') against a
brute-force suffix array: the decoded [L, R) is the pure walk's interval of the
entry's code (set_ftab(0)), and an entry carries a text position exactly when
its interval is one row -- then sa[L].  No leeway.  Where the table must stay
{L, R} -- the switch at 0, a lowered fit bound, a table built by an explicit
set_ftab(N) -- it does, and the searches equal the oracle all the same.
"""
import numpy as np
import pytest

import util
from skip_texts import ACGT
from test_jump_table import jump_texts

NAMES = ["aligned", "plain", "atail", "homopolymer", "short"]


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
    K.set_ftab_fold(1)
    K.set_ftab_fold_bound(None)
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.fixture(scope="module")
def brute():
    """name -> the text's suffix array (row 0 = the '$' suffix)."""
    out = {}
    for name, t in jump_texts().items():
        sa = np.asarray(util.suffix_array(t.tobytes() + b"$"), dtype=np.int64)
        assert sa.size == t.size + 1 and sa[0] == t.size
        out[name] = sa
    return out


def _code_reads(bases):
    """The read of every table index v: the entry of v is the interval of the
    code stream whose base m-1-r sits at bits 2r, so read base j is digit
    m-1-j of v."""
    v = np.arange(1 << (2 * bases), dtype=np.int64)
    cols = [(v >> (2 * (bases - 1 - j))) & 3 for j in range(bases)]
    code_to_base = np.empty(4, dtype=np.uint8)
    for b in ACGT:
        code_to_base[util.code_of(int(b))] = b
    return np.ascontiguousarray(code_to_base[np.stack(cols, axis=1)])


def _walked(K, idx, bases, backend):
    """[L, R) of every code by the pure walk on the same device copy."""
    K.set_ftab(0)
    K.set_skip(0)
    K.set_jump(0)
    out = K.search_array(idx, _code_reads(bases), backend).reshape(-1, 2).astype(np.int64)
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")
    return out


def _decode(K, n, raw, folded):
    """The library's own decode of every raw entry: ([L, R) int64 [N, 2], p int64 [N], -1 = none)."""
    dec = [K.ftab_fold_decode(n, int(x), int(y), folded) for x, y in raw]
    iv = np.array([(L, R) for L, R, _ in dec], dtype=np.int64).reshape(-1, 2)
    pos = np.array([-1 if p is None else p for _, _, p in dec], dtype=np.int64)
    return iv, pos


def _check_folded(K, idx, t, sa, backend, k, member=0):
    n = int(t.size)
    bases, folded, raw = idx.ftab_entries(member=member)
    assert bases == K.ftab_auto_bases(n + 1, k, 1 << 40) and raw.shape == (1 << (2 * bases), 2)
    assert folded, "an upload that built the auto table and the text jump's tables folds it"
    iv, pos = _decode(K, n, raw, True)
    want = _walked(K, idx, bases, backend)
    bad = np.flatnonzero((iv != want).any(axis=1))
    assert bad.size == 0, ("interval", int(bad.size), int(bad[0]), iv[bad[0]].tolist(), want[bad[0]].tolist())
    one = want[:, 1] - want[:, 0] == 1
    assert np.array_equal(pos >= 0, one), "a position exactly on the one-row entries"
    assert np.array_equal(pos[one], sa[want[one, 0]]), "the position is sa[L]"
    return int(one.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("backend", ["task", "task-mid"])
def test_every_entry(gpu, brute, backend, k, d, name):
    t = jump_texts()[name]
    idx = gpu.Index.build(t.tobytes(), k=k, d=d)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.transfer_to_gpu(idx, None, None)                     # the fold is part of the upload
        ones = _check_folded(gpu, idx, t, brute[name], backend, k)
        if name in ("aligned", "plain", "atail"):
            assert ones >= 16
        idx.free_gpu()
        with pytest.raises(gpu.KfmiError):
            idx.ftab_entries()
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k", [("task", 1), ("task-mid", 2)])
def test_split_class_4(gpu, brute, backend, k):
    """The fold pass's sa gather in its four-group form."""
    t = jump_texts()["plain"]
    idx = gpu.Index.build(t.tobytes(), k=k, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.set_split_class(4)
        gpu.transfer_to_gpu(idx, None, None)
        _check_folded(gpu, idx, t, brute["plain"], backend, k)
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
def test_device_group_folds_on_every_member(gpu, brute):
    t = jump_texts()["plain"]
    idx = gpu.Index.build(t.tobytes(), k=2, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend("task-mid")
        gpu.set_devices([0, 0])
        gpu.transfer_to_gpu(idx, None, None)
        n = int(t.size)
        tables = []
        for member in (0, 1):
            bases, folded, raw = idx.ftab_entries(member=member)
            assert folded, member
            tables.append(raw)
        assert np.array_equal(tables[0], tables[1])
        iv, pos = _decode(gpu, n, tables[0], True)
        one = pos >= 0
        assert one.sum() >= 16 and np.array_equal(iv[one, 1], iv[one, 0] + 1)
        assert np.array_equal(pos[one], brute["plain"][iv[one, 0]])
        gpu.set_devices([])
        idx.free_gpu()
        gpu.transfer_to_gpu(idx, None, None)                     # the single copy's table: entry for entry the same
        assert np.array_equal(idx.ftab_entries()[2], tables[0])
        _check_folded(gpu, idx, t, brute["plain"], "task-mid", 2)
    finally:
        idx.close()
        _defaults(gpu)


def _reads_of(t, m, count, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, t.size - m + 1, size=count)
    return np.ascontiguousarray(t[s[:, None] + np.arange(m)[None, :]])


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["switch-0", "lowered-bound"])
@pytest.mark.parametrize("backend,k", [("task", 1), ("task-mid", 2)])
def test_table_stays_as_the_parents(gpu, oracle_mod, backend, k, how):
    """With the switch at 0, or when a width does not fit the (lowered) bound,
    the raw table is {L, R} and the searches equal the oracle."""
    t = jump_texts()["plain"]
    idx = gpu.Index.build(t.tobytes(), k=k, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        if how == "switch-0":
            gpu.set_ftab_fold(0)
        else:
            gpu.set_ftab_fold_bound(2)                           # some entry of a random text is two rows or more
        gpu.transfer_to_gpu(idx, None, None)
        bases, folded, raw = idx.ftab_entries()
        assert not folded
        want = _walked(gpu, idx, bases, backend)
        assert (want[:, 1] - want[:, 0] >= 2).any()
        assert np.array_equal(raw.astype(np.int64), want)
        q = _reads_of(t, 100, 300, 77)
        assert np.array_equal(gpu.search_array(idx, q, backend), oracle_mod.search(idx.image(), q)[0])
        if how == "lowered-bound":                               # and at the width itself the fold goes through
            idx.free_gpu()
            gpu.set_ftab_fold_bound(int((want[:, 1] - want[:, 0]).max()) + 1)
            gpu.transfer_to_gpu(idx, None, None)
            assert idx.ftab_entries()[1]
            idx.free_gpu()
            gpu.set_ftab_fold_bound(int((want[:, 1] - want[:, 0]).max()))
            gpu.transfer_to_gpu(idx, None, None)
            assert not idx.ftab_entries()[1]
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
def test_explicit_table_is_never_folded(gpu, oracle_mod):
    """set_ftab(N) on a fresh upload builds its table at the first search; that
    table is never rewritten, also when N is the auto table's base count and
    the auto settings come back on the same copy."""
    t = jump_texts()["plain"]
    k = 2
    idx = gpu.Index.build(t.tobytes(), k=k, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend("task-mid")
        bases = gpu.ftab_auto_bases(t.size + 1, k, 1 << 40)
        gpu.set_ftab(bases)
        q = _reads_of(t, 100, 300, 78)
        want = oracle_mod.search(idx.image(), q)[0]
        assert np.array_equal(gpu.search_array(idx, q, "task-mid"), want)
        with pytest.raises(gpu.KfmiError):                       # no auto table yet
            idx.ftab_entries()
        gpu.set_ftab("auto")
        assert np.array_equal(gpu.search_array(idx, q, "task-mid"), want)
        b, folded, raw = idx.ftab_entries()                      # the auto rule finds the explicit table there
        assert b == bases and not folded
        assert np.array_equal(raw.astype(np.int64), _walked(gpu, idx, bases, "task-mid"))
    finally:
        idx.close()
        _defaults(gpu)
