"""The folded form of a jump-start entry (DESIGN.md 5a'''', kfmi_device.h
ftab_entry_at) as host arithmetic: encode and decode through the library's own
helper, the round trip of every kind of entry, and the fit rule on both sides
of its bound.  No device.
"""
import pytest

NS = [7, 3020, 2**31 - 2, 2**31 - 1, 2**31, 3_000_000_000, 2**32 - 3]
NONE = 0xFFFFFFFF


def _rows_L(n):
    """Rows L of one-row entries worth trying: the first, the last, one inside."""
    return sorted({0, 1, n // 2, n - 1, n})


@pytest.mark.parametrize("n", NS)
def test_one_row_entries_round_trip(kfmi_mod, n):
    K = kfmi_mod
    for L in _rows_L(n):
        for p in (0, 1, n - 1, n):
            x, y = K.ftab_fold_encode(n, L, L + 1, p)
            assert x == L and y == NONE - p
            assert K.ftab_fold_decode(n, x, y) == (L, L + 1, p), (n, L, p)
    with pytest.raises(K.KfmiError):                             # no position past the text
        K.ftab_fold_encode(n, 0, 1, n + 1)


@pytest.mark.parametrize("n", NS)
def test_other_widths_round_trip(kfmi_mod, n):
    K = kfmi_mod
    bound = K.ftab_fold_bound(n)
    assert bound == NONE - n
    rows = n + 1
    widest = min(bound - 1, rows)                                # the largest width that fits, or the whole index
    if 2 >= bound:                                               # n = 2^32 - 3: only empty and one-row entries fit
        with pytest.raises(K.KfmiError):
            K.ftab_fold_encode(n, 0, 2)
    for w in sorted(w for w in {0, 2, widest} if w != 1 and w < bound):
        for L in sorted({0, 1, rows - w}):
            if L < 0 or L + w > rows:
                continue
            x, y = K.ftab_fold_encode(n, L, L + w)
            assert (x, y) == (L, w)
            assert K.ftab_fold_decode(n, x, y) == (L, L + w, None), (n, L, w)


@pytest.mark.parametrize("n", NS)
def test_fit_rule_on_both_sides_of_its_bound(kfmi_mod, n):
    K = kfmi_mod
    bound = K.ftab_fold_bound(n)
    assert K.ftab_fold_fits(n, 0) and K.ftab_fold_fits(n, bound - 1)
    assert not K.ftab_fold_fits(n, bound) and not K.ftab_fold_fits(n, bound + 1)
    K.ftab_fold_encode(n, 0, bound - 1)
    with pytest.raises(K.KfmiError):                             # a width one over: the fold is refused
        K.ftab_fold_encode(n, 0, bound)
    # the width just under the bound is no position, the bound itself would read as p = n
    assert K.ftab_fold_decode(n, 5, bound - 1) == (5, 5 + bound - 1, None)
    assert K.ftab_fold_decode(n, 5, bound) == (5, 6, n)
    # below 2^31 every interval of the index fits; above, only some texts
    assert (bound - 1 >= n + 1) == (n < 2**31 - 1), n


def test_unfolded_entries_are_taken_as_they_are(kfmi_mod):
    K = kfmi_mod
    for n in NS:
        for L, R in ((0, n + 1), (3, 4), (9, 9), (n, n + 1)):
            assert K.ftab_fold_decode(n, L, R, folded=False) == (L, R, None)


def test_switch(kfmi_mod):
    K = kfmi_mod
    try:
        K.set_ftab_fold(0)
        assert K.ftab_fold() == 0
        K.set_ftab_fold(1)
        assert K.ftab_fold() == 1
        with pytest.raises(K.KfmiError):
            K.set_ftab_fold(2)
    finally:
        K.set_ftab_fold(1)
        K.set_ftab_fold_bound(None)
