"""The skip table's auto rule and setting (DESIGN.md 5a'), host arithmetic only:
kfmi_skip_auto, and the resolved setting following the ftab setting.
"""
import pytest


def test_auto_rule(kfmi_mod):
    f = kfmi_mod.skip_auto
    rows3g = 3_000_000_001
    for k in (1, 2):
        # the budget on both sides of 16 * rows (the table and its transient twin)
        assert f(rows3g, k, 16 * rows3g)
        assert f(rows3g, k, 16 * rows3g + 1)
        assert f(rows3g, k, 1 << 62)
        assert not f(rows3g, k, 16 * rows3g - 1)
        assert not f(rows3g, k, 0)
        for rows in (8, 9, 4_096, 200_002):
            assert f(rows, k, 16 * rows) and not f(rows, k, 16 * rows - 1), rows
        # tiny indexes get none (as they get no ftab), nor do row counts past 32 bits
        for rows in (0, 1, 7):
            assert not f(rows, k, 1 << 62), rows
        assert f((1 << 32) - 1, k, 1 << 62) and not f(1 << 32, k, 1 << 62)
    # K = 3 / 4 (and K the kernels do not have): off whatever the budget
    for k in (0, 3, 4, 5):
        for rows in (8, 200_002, rows3g):
            assert not f(rows, k, 1 << 62), (k, rows)


def test_setting_follows_ftab(kfmi_mod):
    K = kfmi_mod
    try:
        K.set_skip("auto")
        K.set_ftab("auto")
        assert K.skip_in_effect() == 2          # auto, in effect
        for bases in (0, 8, 16):                # an explicit ftab setting names its own walk: no skip
            K.set_ftab(bases)
            assert K.skip_in_effect() == 0, bases
        K.set_skip(1)                           # explicit on: whatever the ftab setting
        for bases in (0, 8, "auto"):
            K.set_ftab(bases)
            assert K.skip_in_effect() == 1, bases
        K.set_skip(0)
        for bases in (0, 8, "auto"):
            K.set_ftab(bases)
            assert K.skip_in_effect() == 0, bases
        K.set_skip(K.SKIP_AUTO)
        assert K.skip_in_effect() == 2
        for v in (2, 17, 1 << 20):
            with pytest.raises(K.KfmiError) as e:
                K.set_skip(v)
            assert e.value.code == 33
        assert K.skip_in_effect() == 2          # a refused value changes nothing
    finally:
        K.set_skip("auto")
        K.set_ftab("auto")
