"""Which derived tables each search entry point builds on demand, under every
combination of the ftab / skip / jump settings that resolves differently.

The shortcuts check themselves, so a search returns the same intervals whether
or not it was handed a table: only the tables' byte counts show which ones an
entry point asked for.  Every cell uploads a fresh handle under set_ftab(0)
(skip and jump then resolve to off: the copy starts with no table), switches
the setting, runs one entry point once and reads the three byte counts.  The
forward forms (search, search_trace, the forward stream, the group search)
take the text jump; the strand and seed searches and the stream's strand leg
never do, whatever the setting says.

K = 2, d = 64, task-mid, one 4,096-base text; 64 reads of 40 bases and 64 of 41
(one base through the remainder table, which clears the ftab for the search
but does not keep it from being built).  The budget is 1 << 62, so no table
is left out for lack of memory.
"""
import ctypes

import numpy as np
import pytest

import seed_ref as sr
from skip_texts import ACGT

pytestmark = pytest.mark.gpu

N = 4_096
ROWS = N + 1
LENGTHS = (40, 41)
FORMS = ("search", "trace", "strands-rev", "seeds", "stream", "stream-both", "group")
#            ftab    skip    jump
SETTINGS = {
    "ftab8": (8, "auto", "auto"),
    "skip1": ("auto", 1, 0),
    "jump1": ("auto", 0, 1),
    "auto": ("auto", "auto", "auto"),
    "off": (0, "auto", "auto"),
}
# The tables on the device after the one call: f = jump-start table, s = skip
# table, j = the text jump's tables.  The same at both read lengths.
EXPECT = {
    #               ftab8  skip1  jump1  auto   off
    "search":      ("f--", "fs-", "f-j", "fsj", "---"),
    "trace":       ("f--", "fs-", "f-j", "fsj", "---"),
    "strands-rev": ("f--", "fs-", "f--", "fs-", "---"),
    "seeds":       ("f--", "fs-", "f--", "fs-", "---"),
    "stream":      ("f--", "fs-", "f-j", "fsj", "---"),
    "stream-both": ("f--", "fs-", "f--", "fs-", "---"),
    "group":       ("f--", "fs-", "f-j", "fsj", "---"),
}


def _defaults(K):
    K.set_devices([])
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    K.set_device(0)
    _defaults(K)
    K.set_ftab_budget(1 << 62)
    rng = np.random.default_rng(1515)
    text = ACGT[rng.integers(0, 4, size=N)]
    base = {k: K.Index.build(text.tobytes(), k=k, d=64) for k in (1, 2)}
    img1 = base[1].image()
    search = lambda q: oracle_mod.search(img1, q)[0]   # noqa: E731  the true interval at any m
    reads, want = {}, {}
    for m in LENGTHS:
        st = rng.integers(0, N - m + 1, size=64)
        q = np.ascontiguousarray(text[st[:, None] + np.arange(m)[None, :]])
        reads[m] = q
        want[m] = {
            "fwd": search(q),
            "rev": search(sr.tasks_of(q, sr.REV)),
            "both": search(sr.tasks_of(q, sr.BOTH)),
            "seeds": sr.reference(search, q, 2, 2)[0],
        }
        for a in (q, *want[m].values()):
            a.setflags(write=False)
    yield K, base[2].image(), reads, want
    _defaults(K)
    K.set_ftab_budget(None)
    for i in base.values():
        i.close()


def _bytes(idx):
    return idx.ftab_bytes(), idx.skip_bytes(), idx.jump_bytes()


def _run(K, form, idx, q, switch):
    """Uploads what `form` needs under set_ftab(0), checks that the copy has no
    table, switches the setting and runs the entry point once; returns
    (intervals, name of the expected ones)."""
    n = q.shape[0]
    handles = []

    def up(cls, *a):
        handles.append(cls(*a))
        return handles[-1]

    try:
        K.set_ftab(0)
        if form == "group":
            try:
                K.set_devices([0, 0])
            except K.KfmiError:
                pytest.skip("no device group of one device twice")
        if form in ("stream", "stream-both"):
            K.transfer_to_gpu(idx, None, None)
            assert _bytes(idx) == (0, 0, 0)
            switch()
            if form == "stream":
                return K.search_stream(idx, q), "fwd"
            return K.search_stream(idx, q, strands=K.STRAND_BOTH), "both"
        Q = up(K.Queries.from_array, q)
        R = up(K.Results.alloc, 2 * n if form == "seeds" else n)
        K.transfer_to_gpu(idx, Q, R)
        if form == "seeds":
            S = up(K.Results.alloc, 2 * n)
            K.transfer_to_gpu(idx, None, S)
        assert _bytes(idx) == (0, 0, 0)
        switch()
        name = "fwd"
        if form in ("search", "group"):
            K.search(idx, Q, R)
        elif form == "trace":
            rec = np.zeros((n, 4), dtype=np.uint32)
            assert K.load().kfmi_search_trace(idx.ptr, Q.ptr, R.ptr, rec.ctypes.data_as(ctypes.c_void_p)) == 0
        elif form == "strands-rev":
            K.search_strands(idx, Q, R, K.STRAND_REV)
            name = "rev"
        else:
            K.search_seeds(idx, Q, R, S, 2, K.STRAND_FWD)
            name = "seeds"
        K.transfer_to_cpu(R)
        out = R.array().copy()
        return (out.reshape(n, 2, 2) if form == "seeds" else out), name
    finally:
        for h in handles:
            h.close()


@pytest.mark.parametrize("m", LENGTHS)
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("form", FORMS)
def test_tables_built(world, form, setting, m):
    K, image, reads, want = world
    ftab, skip, jump = SETTINGS[setting]
    members = 2 if form == "group" else 1

    def switch():
        K.set_ftab(ftab)
        K.set_skip(skip)
        K.set_jump(jump)

    idx = K.Index.from_image(image)
    try:
        K.set_backend("task-mid")
        got, name = _run(K, form, idx, reads[m], switch)
        seen = _bytes(idx)
        print(form, setting, m, "ftab/skip/jump bytes:", seen)
        flags = EXPECT[form][list(SETTINGS).index(setting)]
        bases = 8 if ftab == 8 else K.ftab_auto_bases(ROWS, 2, 1 << 62)
        sizes = (8 << (2 * bases), 8 * ROWS, 8 * ROWS + 4 * (N // 16 + 2))
        assert seen == tuple(members * size if flag != "-" else 0 for flag, size in zip(flags, sizes)), flags
        assert np.array_equal(got, want[m][name])
    finally:
        _defaults(K)
        idx.close()
