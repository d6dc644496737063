"""The walk trace's bit for the folded jump start (kstep_fmi.h, bit 31 of word 2)
against brute force, on the read mixes of tests/test_ftab_fold_search.py: it is
set exactly for the reads that tried their jump at the K-step where the table
left them and whose entry is one row -- their jump took the position from the
entry and issued no SA load -- and clear for every read when the switch is 0.
Every other bit of every record is the same under either switch, and every
field equals tests/walk_model.py, which knows nothing of the fold: the fold
changes which load supplies the position and nothing else.
"""
from functools import lru_cache

import numpy as np
import pytest

import test_ftab_fold_search as tfs
import test_jump_search as tjs
import walk_model as wm

CASES = [("task", 1, 64), ("task-mid", 2, 64), ("task-mid", 2, 192)]
IDS = [f"{b}-k{k}d{d}" for b, k, d in CASES]


@lru_cache(maxsize=None)
def world():
    return wm.World(tjs.TEXT)


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    kfmi_mod.set_devices([])
    yield kfmi_mod
    tfs._defaults(kfmi_mod)


def expected_bit(k, q, nb, jump_min):
    """From brute force: (the model's fields, the reads whose jump uses the
    entry's position)."""
    w = world()
    iv = w.intervals(q)
    mod = wm.play(w, k, q, ftab_steps=nb // k, skip=True, jump=True, jump_min=jump_min, lines=1, cls=0, iv=iv)
    m = q.shape[1]
    if m % k or m < nb:                                          # the remainder table, or no table: no entry at all
        return mod, np.zeros(q.shape[0], dtype=np.int64)
    one_row = iv[1][:, nb] - iv[0][:, nb] == 1                   # the entry of the read's last nb bases
    bit = (mod["jump_tried"] == 1) & (mod["jump_pos"] == nb // k) & one_row
    assert not ((mod["jump_tried"] == 1) & (mod["jump_pos"] == nb // k) & ~one_row).any()
    return mod, bit.astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("backend,k,d", CASES, ids=IDS)
def test_bit_and_nothing_else(gpu, backend, k, d):
    K = gpu
    idx = K.Index.build(tjs.TEXT.tobytes(), k=k, d=d)
    nb, ms = tfs.lengths(K, k)
    ms = [m for m in ms if m <= 256]                             # what the traced kernel serves
    jm = K.JUMP_MIN_DEFAULT
    try:
        recs = {}
        for fold in (1, 0):
            tfs._defaults(K)
            K.set_ftab_fold(fold)
            K.set_backend(backend)
            idx.free_gpu()
            K.transfer_to_gpu(idx, None, None)
            assert idx.ftab_entries()[1] == bool(fold)
            for m in ms:
                recs[(fold, m)] = K.search_trace(idx, tfs.batch(m, nb, 1000 + m), backend)
        set_total = below_total = 0
        for m in ms:
            q = tfs.batch(m, nb, 1000 + m)
            mod, bit = expected_bit(k, q, nb, jm)
            (iv1, r1), (iv0, r0) = recs[(1, m)], recs[(0, m)]
            assert np.array_equal(iv1, iv0), m
            assert np.array_equal(iv1.reshape(-1, 2)[:, 0], mod["L"]) and np.array_equal(iv1.reshape(-1, 2)[:, 1], mod["R"]), m
            got1, got0 = K.trace_start_folded(r1), K.trace_start_folded(r0)
            assert not got0.any(), (m, "switch 0", int(got0.sum()))
            bad = np.flatnonzero(got1 != bit)
            assert bad.size == 0, (m, "reads", int(bad.size), "first", int(bad[0]), "kernel", int(got1[bad[0]]))
            masked = r1.copy()
            masked[:, 2] &= np.uint32(0x7FFFFFFF)
            assert np.array_equal(masked, r0), (m, "a record differs beyond the bit")
            dec = K.decode_trace(r1)
            for f in wm.FIELDS:
                assert np.array_equal(dec[f], mod[f]), (m, f)
            set_total += int(bit.sum())
            # folded entries whose lane has too few bases left to jump: they walk from [L, L + 1)
            if m % k == 0 and nb < m < nb + jm:
                w = world().intervals(q)
                below_total += int((w[1][:, nb] - w[0][:, nb] == 1).sum())
                assert not bit.any()
        assert set_total >= 16 * 8 and below_total >= 16
    finally:
        idx.close()
        tfs._defaults(K)
