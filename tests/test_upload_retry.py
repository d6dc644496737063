"""transferCPUtoGPU when the device has no room for the old copy of an index
and its replacement together: the old copy is freed and the upload runs again
(kstep_fmi.h, transferCPUtoGPU; DESIGN.md 5a'', "The other rows").

The lack of room is forced, not made: kfmi_fail_index_uploads(n) lets the next
n index uploads fail as a full card makes them fail -- a real hipMalloc that
cannot succeed, so the runtime's last error is left as a full card leaves it --
without taking any memory.

  one refusal    the retry succeeds: the new copy is there, results unchanged;
  two refusals   KFMI_E_DEVICE_ALLOC (31), the handle is left without a device
                 copy, and the next upload works and searches (a stale last
                 error would make it fail with 32).
"""
import numpy as np
import pytest

from skip_texts import texts


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    _defaults(kfmi_mod)
    yield kfmi_mod
    _defaults(kfmi_mod)


def _defaults(K):
    K.fail_index_uploads(0)
    K.set_device(0)
    K.set_devices([])
    K.set_split_class(0)
    K.set_fused(True)
    K.set_alphabet(None)
    K.set_ftab_budget(None)
    K.set_jump_min(K.JUMP_MIN_DEFAULT)
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")
    K.set_backend("task-mid")


@pytest.mark.gpu
@pytest.mark.parametrize("tables", ["auto", 0], ids=["tables", "no-tables"])
def test_replacing_upload_frees_the_old_copy_when_both_do_not_fit(gpu, tables):
    t = texts()["plain"]
    rng = np.random.default_rng(31)
    reads = np.ascontiguousarray(t[rng.integers(0, t.size - 100, size=500)[:, None] + np.arange(100)])
    idx = gpu.Index.build(t.tobytes(), k=2, d=64)
    try:
        _defaults(gpu)
        gpu.set_ftab(tables)
        want = gpu.search_array(idx, reads, "task-mid")
        mid = idx.device_bytes()
        assert mid > 0
        gpu.set_backend("task")
        gpu.transfer_to_gpu(idx, None, None)
        task = idx.device_bytes()
        assert task > mid                                        # the two layouts differ in size
        assert np.array_equal(gpu.search_array(idx, reads, "task"), want)

        # one refusal: the old copy goes, the second attempt lays the new one out
        gpu.set_backend("task-mid")
        gpu.fail_index_uploads(1)
        gpu.transfer_to_gpu(idx, None, None)
        assert idx.device_bytes() == mid
        assert np.array_equal(gpu.search_array(idx, reads, "task-mid"), want)

        # two refusals: an error, no device copy; then an upload as if nothing had happened
        gpu.set_backend("task")
        gpu.fail_index_uploads(2)
        with pytest.raises(gpu.KfmiError) as e:
            gpu.transfer_to_gpu(idx, None, None)
        assert e.value.code == 31
        assert idx.device_bytes() == 0 and idx.ftab_bytes() == 0 and idx.jump_bytes() == 0
        gpu.transfer_to_gpu(idx, None, None)                     # the knob is spent
        assert idx.device_bytes() == task
        assert np.array_equal(gpu.search_array(idx, reads, "task"), want)

        # a first upload that is refused has no old copy to free: one attempt, one error
        idx.free_gpu()
        gpu.fail_index_uploads(1)
        with pytest.raises(gpu.KfmiError) as e:
            gpu.transfer_to_gpu(idx, None, None)
        assert e.value.code == 31
        assert np.array_equal(gpu.search_array(idx, reads, "task"), want)
    finally:
        idx.close()
        _defaults(gpu)
