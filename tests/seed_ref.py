"""Seed search: the reference restatement, the texts and the reads shared by
test_seeds_host.py and test_seeds_gpu.py.

The reference restates the definition of kstep_fmi.h (section 2, seed search)
on top of two things only: a `search` callable that returns the suffix-array
interval of every row of a uint8 [N, len] array -- the tests pass the CPU
oracle on the K = 1 image of the text -- and strand_reads.revcomp_def for the
reverse strand.  It calls no search function of the library."""
import numpy as np

from skip_texts import ACGT
from strand_reads import revcomp_def

FWD, REV, BOTH = 1, 2, 3
TWO_STRANDS = (4_000, 4_400)     # main_text(): these bases' reverse complement is in the text too


def main_text() -> np.ndarray:
    """The text of test_strands_lengths.sweep_text(), built again here: 20,011
    random bases ((n + 1) % 64 != 0), two copied segments (wide intervals deep
    into a read) and 400 bases that are the reverse complement of 400 others."""
    rng = np.random.default_rng(2027)
    t = ACGT[rng.integers(0, 4, size=20_011)].copy()
    t[9_000:10_500] = t[2_000:3_500]
    t[15_000:15_800] = t[6_000:6_800]
    t[12_000:12_400] = revcomp_def(t[None, 4_000:4_400])[0]
    return t


def ac_text() -> np.ndarray:
    """300 bases over A and C only: G and T never occur, so a unit with one of
    them does not occur either."""
    return ACGT[np.random.default_rng(61).integers(0, 2, size=300)].copy()


def _change(q: np.ndarray, rows, pos, rng) -> None:
    """Another base at q[rows, pos]."""
    q[rows, pos] = ACGT[(np.searchsorted(ACGT, q[rows, pos]) + rng.integers(1, 4, size=len(rows))) % 4]


def _spread(m: int, i: int, c: int, rng) -> list:
    """c distinct positions (as many as the length has) for changed read i: by
    turns the last base (the walk's first unit), base 0 (its last), m - 17, one
    of the last 16 bases, then uniformly random ones."""
    want = [m - 1, 0, m - 17, m - 1 - int(rng.integers(0, 16)), int(rng.integers(0, m))]
    out = []
    for p in want[i % len(want):] + want[:i % len(want)] + [int(x) for x in rng.permutation(m)]:
        if 0 <= p < m and p not in out:
            out.append(p)
        if len(out) == min(c, m):
            break
    return out


def main_reads(t: np.ndarray, m: int, seed: int, n_reads: int = 192) -> np.ndarray:
    """n_reads reads of m bases in equal quarters -- unchanged, one, two and
    three changed bases, the last quarter with N and lowercase bytes mixed in --
    each quarter half windows of the text and half reverse complements of
    windows, then the read that ends the text, the one that starts it and the
    reverse complement of each (so either strand has both edge reads).  The
    unchanged windows come from TWO_STRANDS, whose reverse complement is in the
    text as well: they match in full on either strand, so a quarter of the
    tasks of each strand has one full-length record."""
    assert n_reads % 8 == 0 and 1 <= m <= TWO_STRANDS[1] - TWO_STRANDS[0]
    rng = np.random.default_rng(seed)
    g = n_reads // 4
    win = np.arange(m)[None, :]
    st = rng.integers(0, t.size - m + 1, size=n_reads)
    st[:g] = rng.integers(TWO_STRANDS[0], TWO_STRANDS[1] - m + 1, size=g)
    q = t[st[:, None] + win].copy()
    for c in (1, 2, 3):
        for i in range(g):
            r = c * g + i
            for p in _spread(m, i, c, rng):
                _change(q, [r], p, rng)
    for i in range(g):                                       # the last quarter: other bytes on top
        r = 3 * g + i
        if i % 3 == 0:
            q[r, int(rng.integers(0, m))] = ord("N")
        elif i % 3 == 1:
            q[r] = np.char.lower(q[r:r + 1].view("S1")).view(np.uint8)
        else:
            q[r, int(rng.integers(0, m))] = ord("n")
    q[1::2] = revcomp_def(q[1::2])
    ends = np.stack([t[t.size - m:], t[:m]])
    return np.ascontiguousarray(np.concatenate([q, ends, revcomp_def(ends)]))


def ac_reads(t: np.ndarray, m: int, seed: int, n_reads: int = 64) -> np.ndarray:
    """Windows of the A / C text; three reads in four carry one to three G or T
    bytes, by turns at the last base (at odd m and K = 2 the remainder unit),
    at base 0 and anywhere."""
    rng = np.random.default_rng(seed)
    st = rng.integers(0, t.size - m + 1, size=n_reads)
    q = t[st[:, None] + np.arange(m)[None, :]].copy()
    for r in range(n_reads):
        if r % 4 == 0:
            continue
        for p in _spread(m, r, 1 + r % 3, rng):
            q[r, p] = ord("GT"[int(rng.integers(0, 2))])
    return np.ascontiguousarray(q)


def tasks_of(reads: np.ndarray, strands: int) -> np.ndarray:
    """The ns * N tasks of a strand mode: BOTH puts read q on rows 2q (as
    written) and 2q + 1 (reverse strand)."""
    if strands == FWD:
        return np.ascontiguousarray(reads)
    if strands == REV:
        return revcomp_def(reads)
    both = np.empty((2 * reads.shape[0], reads.shape[1]), np.uint8)
    both[0::2], both[1::2] = reads, revcomp_def(reads)
    return both


def reference(search, tasks: np.ndarray, k: int, s: int):
    """The definition, task by task in lockstep: (intervals, spans, skips), the
    first two uint32 [T, s, 2] with unused slots zero, skips[t] the units of
    task t that did not occur on their own.

    Every pass of the outer loop gives each unfinished task its next segment
    (or skips one unit): the substring ending at e grows by one unit at a time
    while it occurs.  All tasks that try the same substring length in a pass go
    to `search` as one array, so a case costs a few calls per length."""
    T, m = tasks.shape
    rem = m % k
    iv, sp = np.zeros((T, s, 2), np.uint32), np.zeros((T, s, 2), np.uint32)
    cnt, skips, e = np.zeros(T, np.int64), np.zeros(T, np.int64), np.full(T, m, np.int64)
    while True:
        act = np.flatnonzero((e > 0) & (cnt < s))
        if act.size == 0:
            return iv, sp, skips
        ea = e[act]
        first = np.where((ea == m) & (rem > 0), rem, k)       # the unit ending at e
        trial = first.copy()                                  # the length tried next
        got = np.zeros(act.size, np.int64)                    # the longest length that occurs
        lr = np.zeros((act.size, 2), np.uint32)
        alive = np.ones(act.size, bool)
        while alive.any():
            for ln in np.unique(trial[alive]):
                sel = np.flatnonzero(alive & (trial == ln))
                rows = act[sel]
                sub = tasks[rows[:, None], (e[rows] - ln)[:, None] + np.arange(ln)[None, :]]
                r = np.asarray(search(np.ascontiguousarray(sub))).reshape(-1, 2)
                ok = r[:, 1] > r[:, 0]
                good = sel[ok]
                got[good], lr[good] = ln, r[ok]
                trial[good] += k
                alive[sel[~ok]] = False
                alive[good[ea[good] == ln]] = False           # reached base 0
        hit = got > 0
        rows = act[hit]
        iv[rows, cnt[rows]] = lr[hit]
        sp[rows, cnt[rows], 0] = ea[hit] - got[hit]
        sp[rows, cnt[rows], 1] = got[hit]
        cnt[rows] += 1
        e[rows] -= got[hit]
        miss = act[~hit]
        skips[miss] += 1
        e[miss] -= first[~hit]


def counts(iv: np.ndarray, sp: np.ndarray) -> np.ndarray:
    """Records per task (a record has len > 0)."""
    return np.count_nonzero(sp[:, :, 1], axis=1)


def assert_main_not_vacuous(m: int, ref8, ref2, what) -> None:
    """What the main text's tasks of one strand must show before any device is
    asked (ref8, ref2: reference() at s = 8 and 2), for m >= 48."""
    iv, sp, _ = ref8
    n, c = iv.shape[0], counts(iv, sp)
    whole = (c == 1) & (sp[:, 0, 0] == 0) & (sp[:, 0, 1] == m)
    assert 4 * np.count_nonzero(whole) >= n, (what, "one full-length record", int(np.count_nonzero(whole)), n)
    assert 4 * np.count_nonzero(c >= 2) >= n, (what, "two or more records", int(np.count_nonzero(c >= 2)), n)
    iv2, sp2, _ = ref2
    capped = (counts(iv2, sp2) == 2) & (sp2[:, 1, 0] > 0)
    assert capped.any(), (what, "no task hits the cap at S = 2")
    wide = iv[:, :, 1].astype(np.int64) - iv[:, :, 0] > 1
    assert wide.any(), (what, "no record with R - L > 1")


def assert_ac_not_vacuous(ref, s: int, what) -> None:
    """On the A / C text some task skips a unit, and some task that skipped one
    ends with fewer than s records."""
    iv, sp, skips = ref
    assert (skips > 0).any(), (what, "no unit skipped")
    assert ((skips > 0) & (counts(iv, sp) < s)).any(), (what, "no task short of records after a skip")
