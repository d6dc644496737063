"""The launch plan on the host: kfmi_launch_plan -- launch_plan (kfmi_plan.h),
the rule every search form asks for its staging, and fetch_form<G>
(kfmi_kernels.h), the rule launch_task and launch_seeds ask for the kernel's
fetch form -- against tests/seed_walk_model.py over the whole cross product of
layouts, K, d, table-size classes, read lengths, strand modes, the fused knob,
ASCII or host-packed reads and the skip table, for seed searches and searches.

Seed and strand launches are held to expected_launch as tests/test_seed_trace.py
holds the device's word 3 to it; the forward search, whose trace records carry no
launch identity, to expected_forward_launch.  The pack launch is written out here
from DESIGN.md "launch plan".  No device and no handle: the accessor takes
values.  tests/test_seed_trace.py ties the same accessor to what the kernels
report they ran.
"""
import itertools

import pytest

import seed_walk_model as swm

LAYOUTS = ("task", "task-mid")
CLASSES = (1, 2, 4)
LENGTHS = (34, 100, 101, 128, 129, 256, 257)
STRANDS = (swm.FWD, swm.REV, swm.BOTH)
NOT_IMPLEMENTED, BAD_ARGUMENT = 19, 33
FTAB_STEPS = 5          # expected_launch's word-3 fields that the plan does not decide take any value


def words(k, m):
    """Code words of a read's K-steps, 16 bases each."""
    return ((m - m % k) // k + 16 // k - 1) // (16 // k)


def refusal(K, *args, **kw):
    with pytest.raises(K.KfmiError) as e:
        K.launch_plan(*args, **kw)
    return e.value.code


def expected_pack(k, m, strands, fused, ascii):
    """None where the kernel packs the ASCII rows itself; else the forward pack
    where there are ASCII rows to pack, or the strand pack from what is there."""
    in_kernel = ascii and fused and m - m % k <= 256 and (strands == swm.FWD or m % k == 0)
    if in_kernel:
        return swm.PACK_NONE
    if strands == swm.FWD:
        return swm.PACK_FORWARD if ascii else swm.PACK_NONE
    return swm.PACK_STRANDS_ASCII if ascii else swm.PACK_STRANDS_WORDS


@pytest.mark.parametrize("layout,k", list(itertools.product(LAYOUTS, (1, 2))), ids=lambda v: str(v))
def test_plan_is_the_model(kfmi_mod, layout, k):
    K = kfmi_mod
    assert K.PLAN_KERNELS[:5] == K.TRACE_KERNELS
    assert K.PLAN_KERNELS[swm.TASK_FUSED_KERNEL:] == ("task_kernel fused", "task_kernel tables", "task_kernel jump",
                                                      "task_kernel words", "coop_kernel")
    assert K.PLAN_PACKS == ("none", "forward", "strands from ascii", "strands from words")
    checked = refused = 0
    for d, cls, m, strands, fused, ascii, skip, seeds in itertools.product(
            swm.D_ALL, CLASSES, LENGTHS, STRANDS, (True, False), (True, False), (True, False), (True, False)):
        what = (layout, k, d, "class", cls, "m", m, "strands", strands, "fused", fused, "ascii", ascii, "skip", skip,
                "seeds" if seeds else "search")
        args = (layout, k, d, cls, m)
        kw = dict(seeds=seeds, strands=strands, ascii=ascii, fused=fused, skip=skip)
        long_words = words(k, m) > 16                            # m - m % k > 256: no kernel keeps them in registers
        if not seeds and strands == swm.FWD:
            for jump, traced in itertools.product((False, True), (False, True)):
                want = swm.expected_forward_launch(layout, k, d, cls, m, fused, ascii, skip, jump, traced)
                if want == NOT_IMPLEMENTED:
                    assert refusal(K, *args, jump=jump, traced=True, **kw) == NOT_IMPLEMENTED, what
                    refused += 1
                else:
                    assert K.launch_plan(*args, jump=jump, traced=traced, **kw) == want, (what, jump, traced)
                    checked += 1
            continue
        if seeds and long_words:                                 # kfmi_search_seeds refuses reads of over 256 bases itself
            assert refusal(K, *args, **kw) == BAD_ARGUMENT, what
            assert refusal(K, *args, traced=True, **kw) == BAD_ARGUMENT, what
            refused += 2
            continue
        want = None if long_words else swm.expected_launch(layout, k, d, cls, m, strands, fused and ascii, FTAB_STEPS, skip, seeds)
        got = K.launch_plan(*args, **kw)
        assert got["pack"] == expected_pack(k, m, strands, fused, ascii), (what, got)
        if want is None:                                         # the plain walk of the task columns: no traced form
            assert not seeds
            assert got == {"form": swm.expected_form(layout, k, d, cls, 0), "maxw": 0, "words_maxw": 0 if long_words else
                           swm.registers(k, m), "pack": got["pack"], "kernel": swm.TASK_WORDS_KERNEL}, what
            assert refusal(K, *args, traced=True, **kw) == NOT_IMPLEMENTED, what
            refused += 1
        else:
            in_kernel = want["kernel"] in (swm.SEED_KERNEL, swm.SEED_STRANDS_KERNEL, swm.TASK_STRANDS_KERNEL)
            assert got["form"] == want["form"] and got["kernel"] == want["kernel"], (what, got, want)
            assert (got["maxw"], got["words_maxw"]) == ((want["maxw"], 0) if in_kernel else (0, want["maxw"])), (what, got)
            assert K.launch_plan(*args, traced=True, **kw) == got, what          # the traced twin launches the same
        checked += 1
    assert checked > 3000 and refused > 300, (checked, refused)


def test_plan_refuses_what_the_calls_refuse(kfmi_mod):
    """The three refusals of the plan by name, and the entry points' own for
    what has no seed or traced kernel."""
    K = kfmi_mod
    # traced forward without fused packing: the knob off, host-packed reads, reads of over 256 bases
    assert refusal(K, "task-mid", 2, 64, 1, 100, fused=False, traced=True) == NOT_IMPLEMENTED
    assert refusal(K, "task-mid", 2, 64, 1, 100, ascii=False, traced=True) == NOT_IMPLEMENTED
    assert refusal(K, "task-mid", 2, 64, 1, 258, traced=True) == NOT_IMPLEMENTED
    assert K.launch_plan("task-mid", 2, 64, 1, 100, traced=True)["kernel"] == swm.TASK_TABLES_KERNEL
    # traced strands on the plain walk of words: packs first, and no skip table or too many words for it
    assert refusal(K, "task-mid", 2, 64, 1, 100, strands=swm.BOTH, fused=False, traced=True) == NOT_IMPLEMENTED
    assert refusal(K, "task-mid", 2, 64, 1, 101, strands=swm.REV, traced=True) == NOT_IMPLEMENTED
    assert refusal(K, "task-mid", 2, 64, 1, 300, strands=swm.REV, skip=True, traced=True) == NOT_IMPLEMENTED
    assert K.launch_plan("task-mid", 2, 64, 1, 101, strands=swm.REV, skip=True, traced=True)["kernel"] == swm.TASK_WORDS_SKIP_KERNEL
    # seeds of more than 16 words
    assert refusal(K, "task-mid", 1, 64, 1, 257, seeds=True) == BAD_ARGUMENT
    assert refusal(K, "task-mid", 2, 64, 1, 258, seeds=True, strands=swm.BOTH) == BAD_ARGUMENT
    assert K.launch_plan("task-mid", 2, 64, 1, 257, seeds=True) == {"form": 8, "maxw": 16, "words_maxw": 0, "pack": swm.PACK_NONE,
                                                                   "kernel": swm.SEED_KERNEL}
    # no seed or traced kernels: cooperative and AltCounters backends, K = 4; their searches plan as ever
    for backend, k in (("coop", 2), ("coop-mid", 1), ("task-ac", 2), ("task-ac-mid", 2), ("task-grp", 4)):
        assert refusal(K, backend, k, 64, 1, 100, seeds=True) == NOT_IMPLEMENTED, backend
        assert refusal(K, backend, k, 64, 1, 100, traced=True) == NOT_IMPLEMENTED, backend
        assert refusal(K, backend, k, 64, 1, 100, strands=swm.BOTH, traced=True) == NOT_IMPLEMENTED, backend
    assert K.launch_plan("coop-mid", 2, 64, 1, 100) == {"form": 0, "maxw": 8, "words_maxw": 0, "pack": swm.PACK_NONE,
                                                        "kernel": swm.COOP_KERNEL}
    got = K.launch_plan("coop-mid", 2, 64, 1, 100, strands=swm.BOTH)          # no fused strand kernel: the strand pack first
    assert (got["maxw"], got["words_maxw"], got["pack"], got["kernel"]) == (0, 8, swm.PACK_STRANDS_ASCII, swm.COOP_KERNEL)
    assert K.launch_plan("task-grp", 4, 64, 1, 100, strands=swm.REV)["pack"] == swm.PACK_STRANDS_ASCII
    # what no kernel is built for, and what is no call
    assert refusal(K, "task-mid", 2, 96, 1, 100) == BAD_ARGUMENT
    assert refusal(K, "task-mid", 2, 64, 3, 100) == BAD_ARGUMENT
    assert refusal(K, "task-mid", 2, 64, 1, 100, strands=4) == BAD_ARGUMENT
