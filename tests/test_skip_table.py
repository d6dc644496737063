"""Every entry of the skip table (DESIGN.md 5a') against a brute-force suffix
array: row i with p = SA[i] has an entry iff p >= 16, and then
row == ISA[p - 16] and code == the 16 text bases before p, base p-1-r at bits
2r.  No leeway: on these plain layouts every entry is exact.
"""
import numpy as np
import pytest

import util
from skip_texts import texts

NONE = 0xFFFFFFFF
CODE = np.array([util.code_of(x) for x in range(256)], dtype=np.uint64)


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    kfmi_mod.set_devices([])
    yield kfmi_mod
    kfmi_mod.set_skip("auto")
    kfmi_mod.set_ftab("auto")


@pytest.fixture(scope="module")
def expected():
    """name -> (valid, row, code) per BWT row, computed once."""
    out = {}
    for name in ("aligned", "plain", "atail"):
        t = texts()[name]
        n = t.size
        sa = np.asarray(util.suffix_array(t.tobytes() + b"$"), dtype=np.int64)
        assert sa.size == n + 1 and sa[0] == n
        isa = np.empty(n + 1, dtype=np.int64)
        isa[sa] = np.arange(n + 1)
        valid = sa >= 16
        p = np.where(valid, sa, 16)
        row = isa[p - 16]
        codes = CODE[t]
        code = np.zeros(n + 1, dtype=np.uint64)
        for r in range(16):
            code |= codes[p - 1 - r] << np.uint64(2 * r)
        out[name] = (valid, row, code)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned", "plain", "atail"])
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("backend", ["task", "task-mid"])
def test_every_entry(gpu, expected, backend, k, d, name):
    t = texts()[name]
    idx = gpu.Index.build(t.tobytes(), k=k, d=d)
    try:
        gpu.set_backend(backend)
        gpu.set_ftab("auto")
        gpu.set_skip("auto")
        gpu.transfer_to_gpu(idx, None, None)          # the table is part of the upload
        assert idx.skip_bytes() == 8 * (t.size + 1)
        steps, tab = idx.skip_table()
        assert steps == 16 // k
        valid, row, code = expected[name]
        got_valid = tab[:, 0] != NONE
        bad = np.flatnonzero(got_valid != valid)
        assert bad.size == 0, ("validity", int(bad.size), int(bad[0]))
        bad = np.flatnonzero(valid & (tab[:, 0] != row))
        assert bad.size == 0, ("row", int(bad.size), int(bad[0]))
        bad = np.flatnonzero(valid & (tab[:, 1] != code))
        assert bad.size == 0, ("code", int(bad.size), int(bad[0]))
        idx.free_gpu()
        assert idx.skip_bytes() == 0
    finally:
        idx.close()
        gpu.set_skip("auto")
        gpu.set_ftab("auto")
