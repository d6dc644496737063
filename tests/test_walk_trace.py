"""What every read's walk took, lane by lane: kfmi_search_trace's records
(kstep_fmi.h) against tests/walk_model.py, field for field and without
tolerance -- the ordinary K-steps, the skip lookups that matched and that did
not, the one text jump (whether, at which step, with how many bases left, from
a line or from the flat tables, how it ended), the steps the jump start
covered and jump_split as the kernel received it -- and the traced intervals
against search_array's and the CPU oracle's, bit for bit.

The shortcuts of skip_walk check themselves, so a shortcut that never fires
returns the intervals of one that always does; these tests are the ones that
tell the two apart.  Each plan below is a list of batches (reads of one length
under one group of settings); tests/test_walk_model.py runs the same plans on
the host, vouches for the model against the oracle and holds that every event
class a plan is about has its reads, so that no test here passes on an empty
class.
"""
from functools import lru_cache

import numpy as np
import pytest

import test_jump_lines_search as tjl
import test_jump_search as tjs
import walk_model as wm
from skip_texts import ACGT

CASES = [("task", 1, 64), ("task-mid", 1, 64), ("task", 2, 64), ("task-mid", 2, 64), ("task-mid", 2, 192)]
IDS = [f"{b}-k{k}d{d}" for b, k, d in CASES]
W = wm.W_LINE


def _text_mod16_1():
    rng = np.random.default_rng(7373)
    t = ACGT[rng.integers(0, 4, size=2_513)]                     # n % 16 == 1: one base in the stream's last word
    t[1_500:1_800] = t[300:600]                                  # a long repeat: two rows to the end
    return t


# name -> (text, start of the repeat's first copy, start of its second; 300 bases each)
TEXTS = {"n3021": (tjs.TEXT, 500, 2_000), "n4096": (tjl.TEXT, 500, 3_000), "n2513": (_text_mod16_1(), 300, 1_500)}
REP = 300


@lru_cache(maxsize=None)
def world(name):
    return wm.World(TEXTS[name][0])


ALL = dict(ftab=True, skip=True, jump=True, jump_min=8, lines=1, cls=0)


def _st(**kw):
    return dict(ALL, **kw)


TABLES = [("all", ALL), ("jump-off", _st(jump=False)), ("skip-off", _st(skip=False)), ("ftab-off", _st(ftab=False)),
          ("all-off", _st(ftab=False, skip=False, jump=False))]
FORMS = [(f"lines{ln}-class{c}", _st(lines=ln, cls=c)) for ln in (0, 1, 2) for c in (0, 4)]


def _reads(t, starts, m):
    return np.ascontiguousarray(t[np.asarray(starts, dtype=np.int64)[:, None] + np.arange(m)[None, :]])


def _clear_starts(name, m, count, rng):
    """Starts of reads whose last bases lie outside both copies of the repeat."""
    t, a, b = TEXTS[name]
    e = np.arange(m, t.size + 1)
    for s in (a, b):
        e = e[(e < s + 12) | (e > s + REP + 30)]
    assert count is None or e.size >= count, (name, m, int(e.size))
    return rng.permutation(e)[:count] - m


def _mutate(q, col, rng):
    out = q.copy()
    rows = np.arange(q.shape[0])
    out[rows, col] = ACGT[(np.searchsorted(ACGT, out[rows, col]) + rng.integers(1, 4, size=q.shape[0])) % 4]
    return out


def _before_zero(t, m, cuts, rng):
    """Reads that would begin `cut` bases before position 0."""
    return np.stack([np.concatenate([ACGT[rng.integers(0, 4, size=c)], t[:m - c]]) for c in cuts])


def _left(name, k, q, f_steps):
    """Bases left when each read is first on one row (-1: never), by the model."""
    return wm.play(world(name), k, q, ftab_steps=f_steps)["row1_left"]


# ---- the plans: lists of (label, reads, settings) --------------------------------------------------------------

def plan_lengths(name, k, fb, rng):
    """Every length at which the code takes another path: around jump_min and
    the jump start's bases, the word boundaries, MAXW 8 | 16, the longest read;
    16 consecutive starts at the text's first bases, up to its last, and inside."""
    t = TEXTS[name][0]
    ms = sorted({1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 99, 100, 128, 129, 150, 192, 193, 256, fb, fb + k} |
                ({fb - k} if fb > k else set()))
    for m in ms:
        starts = np.concatenate([np.arange(16), np.arange(t.size - m - 15, t.size - m + 1), 1_000 + np.arange(16),
                                 _clear_starts(name, m, 48, rng)])
        q = _reads(t, starts, m)
        yield f"m{m}", q, ALL
        yield f"m{m}-jump-off", q, _st(jump=False)                # the skip lookups down to the last that fits
        if m <= 33:
            yield f"m{m}-ftab-off", q, _st(ftab=False)
            yield f"m{m}-ftab-off-jump-off", q, _st(ftab=False, jump=False)


def plan_launch_rule(name, k, fb, rng):
    """Reads of 191, 192 and 193 bases under every form: with the lines' grouped
    form (lines 1, class 4) the launch drops the lines from 193 bases on."""
    t = TEXTS[name][0]
    for m in (191, 192, 193):
        q = _reads(t, _clear_starts(name, m, 32, rng), m)
        for label, st in FORMS:
            yield f"m{m}-{label}", q, st


def plan_windows(name, k, fb, rng):
    """No jump start: reads of about 248 bases are on one row with W - 4 .. W + 4
    bases left, so lanes of both forms share a wave; exact, and with the window's
    nearest and farthest base substituted."""
    t = TEXTS[name][0]
    for m in range(244, 253):
        base = _reads(t, _clear_starts(name, m, 64, rng), m)
        left = _left(name, k, base, 0)
        assert (left >= 8).all()
        q = np.concatenate([base, _mutate(base, left - 1, rng), _mutate(base, np.zeros(64, dtype=np.int64), rng)])
        yield f"m{m}", q, _st(ftab=False)
        if m in (247, 248, 249):
            yield f"m{m}-skip-off", q, _st(ftab=False, skip=False)
            yield f"m{m}-lines2", q, _st(ftab=False, lines=2)
            yield f"m{m}-class4", q, _st(ftab=False, cls=4)       # over 192 bases: the flat tables for every lane


def _inside(left, k):
    """A jump_min strictly inside the batch's `left` with at least 16 lanes at it and 16 one unit below."""
    v, c = np.unique(left[left > 0], return_counts=True)
    cnt = dict(zip(v.tolist(), c.tolist()))
    ok = [x for x in cnt if cnt[x] >= 16 and cnt.get(x - k, 0) >= 16 and v.min() < x < v.max()]
    assert ok, cnt
    return max(ok)


def plan_jump_min(name, k, fb, rng):
    """jump_min at its default, at 1, and at a value inside the batch's range of
    bases left, so that lanes on both sides of the threshold share a wave: one
    with exactly jump_min bases left jumps, one with jump_min - K looks up the
    skip table or steps."""
    t = TEXTS[name][0]
    for m in (100, 101):
        cand = _clear_starts(name, m, None, rng)                  # at most 96 reads per value of `left`: a flat batch
        left = _left(name, k, _reads(t, cand, m), 0)
        keep = np.concatenate([np.flatnonzero(left == v)[:96] for v in np.unique(left[left > 0])])
        q = _reads(t, cand[rng.permutation(keep)], m)
        mid = _inside(_left(name, k, q, 0), k)
        for jm in (8, 1, mid):
            yield f"m{m}-ftab-off-min{jm}", q, _st(ftab=False, jump_min=jm)
        common = int(np.bincount(_left(name, k, q, 0 if m % k else fb // k)).argmax())
        for jm in (common, common + k):
            yield f"m{m}-min{jm}", q, _st(jump_min=jm)
    for m in (14, 15, 16, 17, 18):                                # the default threshold itself
        q = _reads(t, _clear_starts(name, m, 128, rng), m)
        yield f"m{m}-ftab-off", q, _st(ftab=False)
        yield f"m{m}-ftab-off-skip-off", q, _st(ftab=False, skip=False)


def plan_substitutions(name, k, fb, rng):
    """One substituted base per read: at the window's nearest and farthest base
    and one inside either, on both sides of the dword boundaries next to them,
    in the second skip window, and just past the window, in the steps already
    taken (no jump at all, or one somewhere else)."""
    t = TEXTS[name][0]
    n = t.size
    for m in (100, 150):
        starts = _clear_starts(name, m, 32, rng)
        base = _reads(t, starts, m)
        left = _left(name, k, base, 0 if m % k else fb // k)
        assert (left >= 64).all()
        hi = (n - starts - 1) % 16                                # column in stream slot 0 mod 16, by the window's far end
        lo = left - 1 - (15 - (n - starts - left) % 16)           # column in slot 15 mod 16, by its near end
        cols = [np.zeros(32, dtype=np.int64), np.ones(32, dtype=np.int64), left - 1, left - 2, hi, hi + 1, lo, lo - 1,
                left - 16, left - 17, left, left + 1]
        for c in cols:
            assert (c >= 0).all() and (c < m).all()
        q = np.concatenate([base] + [_mutate(base, c, rng) for c in cols])
        for label, st in TABLES + FORMS[:2] + FORMS[3:]:
            yield f"m{m}-{label}", q, st


def plan_ends(name, k, fb, rng):
    """16 consecutive starts (every residue of a line, every shift) at the text's
    first base, up to its last, and inside; reads that would begin before position
    0, which the jump refuses before its loads."""
    t = TEXTS[name][0]
    for m in (40, 100, 150):
        starts = np.concatenate([np.arange(16), np.arange(t.size - m - 15, t.size - m + 1), 1_000 + np.arange(16)])
        q = np.concatenate([_reads(t, starts, m), _before_zero(t, m, range(1, 25), rng)])
        for label, st in TABLES + FORMS[:2] + FORMS[3:]:
            yield f"m{m}-{label}", q, st


def plan_repeat(name, k, fb, rng):
    """Reads inside the repeat never reach one row: after the jump start, plain
    steps and nothing else.  Reads that begin before the second copy and end in
    it leave the repeat partway and jump late."""
    t, a, b = TEXTS[name]
    for m in (100, 150):
        inside = np.concatenate([s + np.arange(0, REP - m + 1, 8) for s in (a, b)])
        partway = b - np.arange(1, 41)
        q = _reads(t, np.concatenate([inside, partway]), m)
        for label, st in TABLES:
            yield f"m{m}-{label}", q, st


def plan_batch_edges(name, k, fb, rng):
    """Batches of 1, 63, 64, 65 and 257 reads of a mixed population."""
    t = TEXTS[name][0]
    m = 100
    base = _reads(t, _clear_starts(name, m, 120, rng), m)
    left = _left(name, k, base, fb // k)
    q = np.concatenate([base, _mutate(base, left - 1, rng)[:60], _mutate(base, left - 20, rng)[:60],
                        _before_zero(t, m, range(1, 18), rng)])
    assert q.shape[0] == 257
    for num in (1, 63, 64, 65, 257):
        yield f"first{num}", q[:num], ALL
        yield f"last{num}-ftab-off", q[257 - num:], _st(ftab=False)


# plan -> (generator, the event classes it is about, fewest reads per class)
PLANS = {
    "lengths": (plan_lengths, ("taken_line", "jump_start", "jump_start_exact", "no_jump_start", "no_jump", "skip_hit",
                              "skip_last"), 16),
    "launch_rule": (plan_launch_rule, ("rule_kept", "rule_dropped", "taken_line", "taken_flat"), 16),
    "windows": (plan_windows, ("window_W", "window_W_plus_K", "taken_line", "taken_flat", "differed", "skip_hit",
                               "skip_miss"), 16),
    "jump_min": (plan_jump_min, ("at_jump_min", "below_jump_min", "taken_line", "skip_hit"), 16),
    "substitutions": (plan_substitutions, ("differed", "skip_hit", "skip_miss", "taken_line", "taken_flat", "no_jump"), 16),
    "ends": (plan_ends, ("refused", "taken_line", "taken_flat", "skip_hit"), 16),
    "repeat": (plan_repeat, ("steps_only", "taken_line", "jump_start"), 16),
    "batch_edges": (plan_batch_edges, ("taken_line", "differed", "refused", "skip_hit", "skip_miss"), 1),
}


@lru_cache(maxsize=None)
def batches(plan, name, k, fb):
    """The plan's batches on one text, with the model's fields for each."""
    rng = np.random.default_rng(4 * sum(map(ord, plan + name)) + k)
    out = []
    for label, q, st in PLANS[plan][0](name, k, fb, rng):
        q = np.ascontiguousarray(q)
        m = q.shape[1]
        f_steps = fb // k if st["ftab"] and fb % k == 0 else 0
        mod = wm.play(world(name), k, q, ftab_steps=f_steps, skip=st["skip"], jump=st["jump"], jump_min=st["jump_min"],
                      lines=st["lines"], cls=st["cls"])
        out.append((label, q, st, mod))
    return out


def class_counts(plan, name, k, fb):
    tot = {}
    for label, q, st, mod in batches(plan, name, k, fb):
        for c, mask in wm.classes(mod, k, st, q.shape[1]).items():
            tot[c] = tot.get(c, 0) + int(mask.sum())
    return tot


# ---- the GPU side ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    kfmi_mod.set_devices([])
    yield kfmi_mod
    tjl._defaults(kfmi_mod)


@pytest.fixture(scope="module")
def indexes(gpu):
    cache = {}

    def index(name, k, d):
        if (name, k, d) not in cache:
            cache[(name, k, d)] = gpu.Index.build(TEXTS[name][0].tobytes(), k=k, d=d)
        return cache[(name, k, d)]

    yield index
    for i in cache.values():
        i.close()


def apply_settings(K, st):
    K.set_ftab("auto" if st["ftab"] else 0)
    if st["ftab"] and st["skip"] and st["jump"]:
        K.set_skip("auto")
        K.set_jump("auto")
        assert K.jump_in_effect() == 2 and K.skip_in_effect() == 2
    else:
        K.set_skip(1 if st["skip"] else 0)
        K.set_jump(1 if st["jump"] else 0)
    K.set_jump_min(st["jump_min"])
    K.set_jump_lines(st["lines"])
    K.set_split_class(st["cls"])


def check_batch(K, oracle_mod, indexes, name, backend, k, d, label, q, st, mod):
    """One batch on the GPU: intervals three ways, then every field of every record."""
    idx = indexes(name, k, d)
    apply_settings(K, st)
    got, rec = K.search_trace(idx, q, backend)
    if st["skip"]:
        assert idx.skip_bytes() > 0, label
    if st["jump"]:
        assert idx.jump_bytes() > 0 and idx.jump_line_bytes() > 0, label
    plain = K.search_array(idx, q, backend)
    img = indexes(name, 1, 64).image() if q.shape[1] % k else idx.image()
    want = oracle_mod.search(img, q)[0]
    assert np.array_equal(got, plain), (label, "trace != search_array", int(np.flatnonzero(got != plain)[0]) // 2)
    assert np.array_equal(got, want), (label, "trace != oracle", int(np.flatnonzero(got != want)[0]) // 2)
    dec = K.decode_trace(rec)
    assert tuple(dec) == wm.FIELDS == K.TRACE_FIELDS
    for f in wm.FIELDS:
        bad = np.flatnonzero(dec[f] != mod[f])
        assert bad.size == 0, (label, f, "reads", int(bad.size), "first", int(bad[0]), "kernel", int(dec[f][bad[0]]),
                               "model", int(mod[f][bad[0]]), {g: int(dec[g][bad[0]]) for g in wm.FIELDS},
                               {g: int(mod[g][bad[0]]) for g in wm.FIELDS})


PARAMS = [(p, n, b, k, d) for p in PLANS for n in TEXTS for b, k, d in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("plan,name,backend,k,d", PARAMS, ids=[f"{p}-{n}-{b}-k{k}d{d}" for p, n, b, k, d in PARAMS])
def test_walk_trace(gpu, oracle_mod, indexes, plan, name, backend, k, d):
    fb = gpu.ftab_auto_bases(TEXTS[name][0].size + 1, k, 1 << 40)
    try:
        tjl._defaults(gpu)
        gpu.set_backend(backend)
        counts = class_counts(plan, name, k, fb)
        for c in PLANS[plan][1]:
            assert counts.get(c, 0) >= PLANS[plan][2], (plan, c, counts.get(c, 0))
        for label, q, st, mod in batches(plan, name, k, fb):
            check_batch(gpu, oracle_mod, indexes, name, backend, k, d, label, q, st, mod)
    finally:
        tjl._defaults(gpu)


@pytest.mark.gpu
def test_refusals_on_the_device(gpu, indexes):
    """What has no traced kernel is refused, with the seed search's code, before
    anything is written: coop and AltCounters backends, K = 4, a device group,
    reads too long for the fused packing and fused packing off."""
    t = TEXTS["n3021"][0]
    q = _reads(t, np.arange(40), 100)
    idx = indexes("n3021", 2, 64)
    not_impl = 19
    try:
        tjl._defaults(gpu)
        for backend in ("coop", "coop-mid", "task-ac", "task-ac-mid"):
            with pytest.raises(gpu.KfmiError) as e:
                gpu.search_trace(idx, q, backend)
            assert e.value.code == not_impl, backend
        with pytest.raises(gpu.KfmiError) as e:
            gpu.search_trace(idx, _reads(t, np.arange(8), 300), "task-mid")
        assert e.value.code == not_impl
        gpu.set_fused(False)
        with pytest.raises(gpu.KfmiError) as e:
            gpu.search_trace(idx, q, "task-mid")
        assert e.value.code == not_impl
        gpu.set_fused(True)
        gpu.set_devices([0, 0])
        with pytest.raises(gpu.KfmiError) as e:
            gpu.search_trace(idx, q, "task-mid")
        assert e.value.code == not_impl
        gpu.set_devices([])
        i4 = gpu.Index.build(t.tobytes(), k=4, d=64)
        try:
            with pytest.raises(gpu.KfmiError) as e:
                gpu.search_trace(i4, q, "task-grp")
            assert e.value.code == not_impl
        finally:
            i4.close()
        got, rec = gpu.search_trace(idx, q, "task-mid")          # and the handles still serve
        assert np.array_equal(got, gpu.search_array(idx, q, "task-mid"))
    finally:
        gpu.set_fused(True)
        tjl._defaults(gpu)
        idx.free_gpu()
