"""Every dword of the text jump's line table (DESIGN.md 5a''') against a
brute-force suffix array and the text, no leeway.  Line j serves the window
ends e in [16j, 16j + 16) of the reversed text's slots (slot g = base
n - 1 - g): dword t < 16 is ISA[n - (16j + t)], 0xFFFFFFFF where 16j + t > n;
dwords 16 .. 31 hold the slots [16j + 16 - 256, 16j + 16), lowest slot at bit 0
of dword 16, zero below slot 0 and from slot n on.  n // 16 + 2 lines, the last
one padding.  The host's arithmetic of a lane's reads (kfmi_jump_line_geometry)
is checked without a GPU against the same model.
"""
import numpy as np
import pytest

import util
from skip_texts import ACGT
from test_jump_table import CODE, jump_texts

S, W = 16, 240
NONE = 0xFFFFFFFF


def line_texts() -> dict:
    t = dict(jump_texts())
    rng = np.random.default_rng(1212)
    for n in (1_008, 1_009, 1_007):                              # n % 16 = 0, 1, 15
        t[f"mod{n % 16}"] = ACGT[rng.integers(0, 4, size=n)]
    return t


NAMES = ["aligned", "plain", "atail", "homopolymer", "short", "mod0", "mod1", "mod15"]


def model_lines(t):
    """uint32 [n // 16 + 2, 32] from the text alone."""
    n = t.size
    sa = np.asarray(util.suffix_array(t.tobytes() + b"$"), dtype=np.int64)
    isa = np.empty(n + 1, dtype=np.int64)
    isa[sa] = np.arange(n + 1)
    lines = n // S + 2
    out = np.zeros((lines, 32), dtype=np.uint32)
    e = S * np.arange(lines)[:, None] + np.arange(S)[None, :]
    out[:, :S] = np.where(e <= n, isa[np.clip(n - e, 0, n)], NONE)
    slot = np.zeros(256 + S * lines, dtype=np.uint32)            # slot g at index g + 256 - S
    slot[256 - S:256 - S + n] = CODE[t][::-1]
    for j in range(lines):
        half = slot[S * j:S * j + 256].reshape(16, 16)           # slots [16j + 16 - 256, 16j + 16)
        out[j, S:] = (half << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1, dtype=np.uint32)
    return out


@pytest.fixture(scope="module")
def expected():
    return {name: model_lines(t) for name, t in line_texts().items()}


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
    K.set_jump_lines(1)
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")


def _jump_bytes(n):
    return 8 * (n + 1) + 4 * (n // 16 + 2)


def _check_lines(idx, want, member=0):
    got = idx.jump_lines(member)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (int(bad.shape[0]), bad[0].tolist(), hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("backend", ["task", "task-mid"])
def test_every_dword(gpu, expected, backend, k, d, name):
    t = line_texts()[name]
    idx = gpu.Index.build(t.tobytes(), k=k, d=d)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        assert idx.jump_bytes() == 0 and idx.jump_line_bytes() == 0
        gpu.transfer_to_gpu(idx, None, None)                     # the lines are part of the upload
        assert idx.jump_bytes() == _jump_bytes(t.size)           # what it always was
        assert idx.jump_line_bytes() == 128 * (t.size // 16 + 2)
        _check_lines(idx, expected[name])
        idx.free_gpu()
        assert idx.jump_bytes() == 0 and idx.jump_line_bytes() == 0
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("lines", [0, 2])
@pytest.mark.parametrize("backend,k", [("task", 1), ("task-mid", 2)])
def test_split_class_4_and_the_knob(gpu, expected, backend, k, lines):
    """The build's gathers in their four-group form; the lines are built
    whatever set_jump_lines says."""
    t = line_texts()["plain"]
    idx = gpu.Index.build(t.tobytes(), k=k, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend(backend)
        gpu.set_split_class(4)
        gpu.set_jump_lines(lines)
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() == _jump_bytes(t.size)
        _check_lines(idx, expected["plain"])
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
def test_device_group_builds_on_every_member(gpu, expected):
    t = line_texts()["mod1"]
    idx = gpu.Index.build(t.tobytes(), k=2, d=64)
    try:
        _defaults(gpu)
        gpu.set_backend("task-mid")
        gpu.set_devices([0, 0])
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() == 2 * _jump_bytes(t.size)
        assert idx.jump_line_bytes() == 2 * 128 * (t.size // 16 + 2)
        for member in (0, 1):
            _check_lines(idx, expected["mod1"], member)
        idx.free_gpu()
        assert idx.jump_line_bytes() == 0
    finally:
        idx.close()
        _defaults(gpu)


@pytest.mark.gpu
def test_no_lines_where_there_are_no_tables(gpu):
    t = line_texts()["plain"]
    try:
        _defaults(gpu)
        for backend, k in (("task-ac", 2), ("coop-mid", 2), ("task-grp", 4)):
            idx = gpu.Index.build(t.tobytes(), k=k, d=64)
            gpu.set_backend(backend)
            gpu.transfer_to_gpu(idx, None, None)
            assert idx.jump_bytes() == 0 and idx.jump_line_bytes() == 0, (backend, k)
            with pytest.raises(gpu.KfmiError):
                idx.jump_lines()
            idx.close()
        idx = gpu.Index.build(t.tobytes(), k=2, d=64)
        gpu.set_backend("task-mid")
        gpu.set_jump(0)
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.jump_bytes() == 0 and idx.jump_line_bytes() == 0
        idx.close()
    finally:
        _defaults(gpu)


def test_host_arithmetic(kfmi_mod):
    """n from 1 to 600: the lines' place and count, and for windows at both
    ends of the text, at every residue of e and at nb = 1, W - 1, W the dwords
    a lane reads -- its ISA entry, its window's first dword and shift, and a
    dword count that covers the window and nothing past its end, all inside
    the lane's own line."""
    K = kfmi_mod
    rng = np.random.default_rng(3)
    for n in range(1, 601):
        ps = {n, 1, min(n, 16), min(n, 17), n // 2 + 1} | set(int(x) for x in rng.integers(1, n + 1, size=4))
        for p in ps:
            nbs = {1, p, min(p, W), min(p, W - 1), min(p, 100)} | set(int(x) for x in rng.integers(1, min(p, W) + 1, size=3))
            for nb in nbs:
                if nb > W:
                    continue
                off, count, isa_dw, text_dw, shift, ndw = K.jump_line_geometry(n, p, nb)
                rows, words = n + 1, n // 16 + 2
                assert off == -(-(2 * rows + words) // 32) * 32 and count == n // 16 + 2
                e = n - p + nb                                   # the window is the slots [e - nb, e)
                j = e // S
                assert j < count - 1 and isa_dw == 32 * j + e % S
                first = S * j + S - 256                          # slot at bit 0 of the line's dword 16
                s = e - nb - first
                assert 0 <= s and s + nb <= 256
                assert text_dw == 32 * j + 16 + s // 16 and shift == 2 * (s % 16)
                last = text_dw + ndw - 1                         # the last dword read
                assert ndw >= 1 and last <= 32 * j + 31
                assert 16 * (last - 32 * j - 16) < s + nb <= 16 * (last - 32 * j - 16 + 1)
    for bad in ((10, 11, 1), (10, 5, 6), (300, 300, W + 1), (10, 5, 0)):
        with pytest.raises(K.KfmiError):
            K.jump_line_geometry(*bad)
    try:
        for mode in (0, 2, 1):
            K.set_jump_lines(mode)
            assert K.jump_lines() == mode
        with pytest.raises(K.KfmiError):
            K.set_jump_lines(3)
    finally:
        K.set_jump_lines(1)
