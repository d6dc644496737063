"""The derived tables' settings resolved against each other (kstep_fmi.h), host
only: ftab -> skip -> text jump.  Auto skip is in effect exactly when the ftab
setting is auto, auto jump exactly when the skip setting resolves to auto and
in effect, and an explicit value stands whatever the others say.  The settings
are per calling thread.
"""
import itertools
import os
import threading

import pytest

FTAB = (0, 8, "auto")
MODE = (0, 1, "auto")


def _expected(ftab, skip, jump):
    s = skip if skip != "auto" else (2 if ftab == "auto" else 0)
    j = jump if jump != "auto" else (2 if s == 2 else 0)
    return s, j


def _restore(K):
    K.set_jump("auto")
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.mark.parametrize("ftab,skip,jump", list(itertools.product(FTAB, MODE, MODE)),
                         ids=lambda v: str(v))
def test_truth_table(kfmi_mod, ftab, skip, jump):
    K = kfmi_mod
    try:
        K.set_ftab(ftab)
        K.set_skip(skip)
        K.set_jump(jump)
        assert (K.skip_in_effect(), K.jump_in_effect()) == _expected(ftab, skip, jump)
    finally:
        _restore(K)


def test_order_of_the_calls_does_not_matter(kfmi_mod):
    """The resolution reads the three settings when asked, not when they are set."""
    K = kfmi_mod
    try:
        for ftab, skip, jump in itertools.product(FTAB, MODE, MODE):
            K.set_jump(jump)
            K.set_skip(skip)
            K.set_ftab(ftab)
            assert (K.skip_in_effect(), K.jump_in_effect()) == _expected(ftab, skip, jump), (ftab, skip, jump)
    finally:
        _restore(K)


def _in_thread(fn):
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    return out[0]


def test_settings_are_per_thread(kfmi_mod):
    K = kfmi_mod

    def read():
        return K.skip_in_effect(), K.jump_in_effect()

    def set_and_read():
        K.set_ftab(0)
        K.set_skip(0)
        K.set_jump(0)
        return read()

    try:
        before = _in_thread(read)                       # a thread that never set anything: the defaults
        if not any(os.environ.get(v) for v in ("KFMI_FTAB", "KFMI_SKIP", "KFMI_JUMP")):
            assert before == (2, 2)
        K.set_ftab(8)
        K.set_skip(1)
        K.set_jump(1)
        assert read() == (1, 1)
        assert _in_thread(read) == before               # not the first thread's settings
        K.set_ftab(0)
        K.set_skip("auto")
        K.set_jump("auto")
        assert read() == (0, 0)
        assert _in_thread(read) == before
        K.set_skip(1)
        K.set_jump(1)
        assert _in_thread(set_and_read) == (0, 0)       # nor does another thread's setting reach this one
        assert read() == (1, 1)
    finally:
        _restore(K)
