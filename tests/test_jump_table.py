"""Every entry of the text jump's tables (DESIGN.md 5a'') against a brute-force
suffix array and the text: sa[row] == SA[row], isa[pos] == ISA[pos], and the
code stream holds base n - 1 - g at bits 2g, zeros past the text.  No leeway.
Where the tables must not exist -- AltCounters and coop backends, K = 4,
set_jump(0), a 'ref'-mode index that is no permutation -- they do not.
"""
import numpy as np
import pytest

import util
from skip_texts import ACGT, texts

CODE = np.array([util.code_of(x) for x in range(256)], dtype=np.uint32)


def jump_texts() -> dict:
    t = texts()
    rng = np.random.default_rng(909)
    return {"aligned": t["aligned"], "plain": t["plain"], "atail": t["atail"],
            "homopolymer": np.full(333, ord("A"), dtype=np.uint8),
            "short": ACGT[rng.integers(0, 4, size=11)]}          # shorter than one 16-base word


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
    K.set_alphabet(None)
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")


def _expect(t):
    n = t.size
    sa = np.asarray(util.suffix_array(t.tobytes() + b"$"), dtype=np.int64)
    assert sa.size == n + 1 and sa[0] == n
    isa = np.empty(n + 1, dtype=np.int64)
    isa[sa] = np.arange(n + 1)
    words = n // 16 + 2
    stream = np.zeros(16 * words, dtype=np.uint32)
    stream[:n] = CODE[t][::-1]                                   # base n - 1 - g at slot g
    text = np.zeros(words, dtype=np.uint32)
    for r in range(16):
        text |= stream[r::16] << np.uint32(2 * r)
    return sa.astype(np.uint32), isa.astype(np.uint32), text


@pytest.fixture(scope="module")
def expected():
    return {name: _expect(t) for name, t in jump_texts().items()}


def _bytes(n):
    return 8 * (n + 1) + 4 * (n // 16 + 2)


def _check_tables(idx, want, member=0):
    sa, isa, text = idx.jump_tables(member)
    for got, exp, what in ((sa, want[0], "sa"), (isa, want[1], "isa"), (text, want[2], "text")):
        assert got.shape == exp.shape, what
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (what, int(bad.size), int(bad[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned", "plain", "atail", "homopolymer", "short"])
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("backend", ["task", "task-mid"])
def test_every_entry(gpu, expected, backend, k, d, name):
    t = jump_texts()[name]
    idx = gpu.Index.build(t.tobytes(), k=k, d=d)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        assert gpu.jump_in_effect() == 2
        assert idx.jump_bytes() == 0
        gpu.transfer_to_gpu(idx, None, None)                     # the tables are part of the upload
        assert idx.jump_bytes() == _bytes(t.size)
        _check_tables(idx, expected[name])
        idx.free_gpu()
        assert idx.jump_bytes() == 0
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k", [("task", 1), ("task-mid", 2)])
def test_split_class_4(gpu, expected, backend, k):
    """The build's gathers and scatters in their four-group form."""
    t = jump_texts()["plain"]
    idx = gpu.Index.build(t.tobytes(), k=k, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.set_split_class(4)
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() == _bytes(t.size)
        _check_tables(idx, expected["plain"])
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
def test_no_tables_where_they_do_not_apply(gpu):
    t = jump_texts()["plain"]
    try:
        _defaults(gpu)
        for backend, k in (("task-ac", 2), ("task-ac-mid", 2), ("coop-mid", 2), ("coop", 1), ("task-grp", 4)):
            idx = gpu.Index.build(t.tobytes(), k=k, d=64)
            gpu.set_backend(backend)
            gpu.set_jump("auto")
            gpu.transfer_to_gpu(idx, None, None)
            assert idx.jump_bytes() == 0, (backend, k)
            gpu.set_jump(1)                                      # explicit on: still none, and no error
            q = t[np.arange(8)[:, None] + np.arange(100)[None, :]]
            gpu.search_array(idx, q, backend)
            assert idx.jump_bytes() == 0, (backend, k)
            with pytest.raises(gpu.KfmiError):
                idx.jump_tables()
            idx.close()
        # set_jump(0): the upload builds the skip table and not these
        idx = gpu.Index.build(t.tobytes(), k=2, d=64)
        gpu.set_backend("task-mid")
        gpu.set_jump(0)
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.skip_bytes() == 8 * (t.size + 1) and idx.jump_bytes() == 0
        # ... nor when the skip setting is not auto and in effect
        for ftab, skip in ((0, "auto"), (8, "auto"), ("auto", 0), ("auto", 1)):
            idx.free_gpu()
            gpu.set_jump("auto")
            gpu.set_ftab(ftab)
            gpu.set_skip(skip)
            assert gpu.jump_in_effect() == 0
            gpu.transfer_to_gpu(idx, None, None)
            assert idx.jump_bytes() == 0, (ftab, skip)
        idx.close()
    finally:
        _defaults(gpu)


@pytest.mark.gpu
def test_ref_mode_non_permutation_gets_none(gpu):
    """A 'ref'-mode index of a text with N runs and lowercase letters: its LF_K
    is no permutation of the rows, the build's check refuses it, the search
    runs on without the tables and equals the search under set_jump(0)."""
    rng = np.random.default_rng(11)
    pure = ACGT[rng.integers(0, 4, size=20_001)]
    mixed = pure.copy()
    mixed[1000:1300] = ord("N")
    mixed[5000:5050] = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, 50)]
    reads = pure[rng.integers(0, pure.size - 100, size=512)[:, None] + np.arange(100)]
    try:
        _defaults(gpu)
        gpu.set_alphabet("ref")
        good = gpu.Index.build(pure.tobytes(), k=2, d=64)
        bad = gpu.Index.build(mixed.tobytes(), k=2, d=64)
        gpu.set_backend("task-mid")
        gpu.transfer_to_gpu(good, None, None)
        assert good.jump_bytes() == _bytes(pure.size)           # A/C/G/T only: an ordinary index
        gpu.transfer_to_gpu(bad, None, None)
        assert bad.skip_bytes() == 8 * (mixed.size + 1) and bad.jump_bytes() == 0
        for mode in ("auto", 1):
            gpu.set_jump(mode)
            got = gpu.search_array(bad, reads, "task-mid")
            assert bad.jump_bytes() == 0
            gpu.set_jump(0)
            assert np.array_equal(got, gpu.search_array(bad, reads, "task-mid")), mode
        good.close()
        bad.close()
    finally:
        _defaults(gpu)


@pytest.mark.gpu
def test_device_group_builds_on_every_member(gpu, expected):
    t = jump_texts()["plain"]
    idx = gpu.Index.build(t.tobytes(), k=2, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend("task-mid")
        gpu.set_devices([0, 0])
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() == 2 * _bytes(t.size)
        for member in (0, 1):
            _check_tables(idx, expected["plain"], member)
        idx.free_gpu()
        assert idx.jump_bytes() == 0
    finally:
        idx.close()
        _defaults(gpu)


def test_auto_rule_and_setting(kfmi_mod):
    """Host arithmetic only: the budget on both sides of the build's peak, and
    the setting following the skip setting."""
    K = kfmi_mod
    f = K.jump_auto
    for rows in (2, 12, 4_096, 3_000_000_001):
        peak = 16 * rows + 4 * ((rows - 1) // 16 + 2)
        for k in (1, 2):
            assert f(rows, k, peak) and not f(rows, k, peak - 1), (rows, k)
        for k in (0, 3, 4):
            assert not f(rows, k, 1 << 62), (rows, k)
    assert not f(1, 2, 1 << 62) and not f(1 << 32, 2, 1 << 62)
    try:
        K.set_jump("auto")
        K.set_skip("auto")
        K.set_ftab("auto")
        assert K.jump_in_effect() == 2
        K.set_ftab(0)
        assert K.jump_in_effect() == 0
        K.set_ftab("auto")
        K.set_skip(1)
        assert K.jump_in_effect() == 0
        K.set_jump(1)
        K.set_skip(0)
        assert K.jump_in_effect() == 1
        K.set_jump(0)
        K.set_skip("auto")
        assert K.jump_in_effect() == 0
        with pytest.raises(K.KfmiError):
            K.set_jump(2)
        with pytest.raises(K.KfmiError):
            K.set_jump_min(0)
        assert K.jump_min() == K.JUMP_MIN_DEFAULT
    finally:
        K.set_jump("auto")
        K.set_skip("auto")
        K.set_ftab("auto")
