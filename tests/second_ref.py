"""Second placement / mapping quality: the model, the text, the reads and the
non-vacuity conditions shared by test_second_host.py and test_second_gpu.py.

The model restates the definitions of kstep_fmi.h ("second placement / mapping
quality") in numpy.  Candidates are verify_ref.candidates', row 0 of each is
align_ref.row0's (through align_ref.Aligned); nothing of the library is called.
second_records() forms both words of every task's second record for any cut of
S, max_occ, band and max_second from word x of given hits; quality() forms the
quality records.

The suite's other texts hold exact copies only, so this file builds its own:
4,099 seeded random bases (n % 16 = 3) with a 400-base segment planted again as
  * an exact copy,
  * a copy with two substitutions 100 bases apart (at 40 and 140 of the segment,
    so that a 256-base read can cross one of them alone),
  * a copy with one base deleted at 160 and, 80 bases on, one inserted,
a poly-A run of 80 bases -- longer than every max_occ used and than a quarter
of the longest read, so that a piece seed of any length >= 100 / 4 lies inside
it -- and 270 bases of a 5-base tandem repeat: a read inside it has exact
places 5, 10, .. bases from the reported one, inside 3w and outside 2w at band
3, which is what the |b - X| <= 2w exclusion has to tell apart.

Reads of one length, each followed by its reverse complement: windows across
every planted difference from every copy at several offsets, the same with one
base of their own changed, windows of unique regions, of the poly-A run and its
flank, of the tandem repeat, and the windows at the origins 0 .. 15 and
n - m - 15 .. n - m, where X lies within 2w of a text end.

Seeds: seed_ref.reference's greedy seeds at S = 8 on the CPU oracle, and piece
seeds at PIECES = 4 from the model's own suffix array."""
import numpy as np

import align_ref as ar
import seed_ref as sr
import verify_ref as vr
from skip_texts import ACGT
from strand_reads import code_of, revcomp_def

NONE, EDIT_MASK, MULTI, SCORED_SHIFT, INF = ar.NONE, ar.EDIT_MASK, ar.MULTI, ar.SCORED_SHIFT, ar.INF
TRUNC = 0x00080000
MAPQ_MAX, MAPQ_PER_EDIT, MAPQ_TRUNCATED = 60, 10, 3
LENGTHS = (16, 17, 100, 128, 129, 256)
BANDS = (0, 1, 3, 15)
PIECES = 4
N = 4_099
SEG, SEG_LEN = 400, 400
EXACT, SUBST, INDEL = 1_200, 2_000, 2_800
SUBS, DEL_AT, INS_AT = (40, 140), 160, 240
POLY_A, POLY_LEN = 3_400, 80
TANDEM, TANDEM_LEN, UNIT = 3_600, 270, 5
BIG = 1 << 40


def second_bounds(m: int):
    return (0, 1, m)


def text() -> np.ndarray:
    rng = np.random.default_rng(2_626)
    t = ACGT[rng.integers(0, 4, size=N)].copy()
    seg = t[SEG:SEG + SEG_LEN].copy()
    t[EXACT:EXACT + SEG_LEN] = seg
    sub = seg.copy()
    for p in SUBS:
        sub[p] = ACGT[(int(np.searchsorted(ACGT, sub[p])) + 1 + p % 3) % 4]
    t[SUBST:SUBST + SEG_LEN] = sub
    new = ACGT[(int(np.searchsorted(ACGT, seg[INS_AT])) + 2) % 4]           # neither seg[INS_AT] ...
    if new == seg[INS_AT - 1]:                                               # ... nor the base before it
        new = ACGT[(int(np.searchsorted(ACGT, seg[INS_AT])) + 1) % 4]
    ind = np.concatenate([seg[:DEL_AT], seg[DEL_AT + 1:INS_AT], np.asarray([new], np.uint8), seg[INS_AT:]])
    assert ind.size == SEG_LEN
    t[INDEL:INDEL + SEG_LEN] = ind
    t[POLY_A:POLY_A + POLY_LEN] = ord("A")
    t[POLY_A - 1] = t[POLY_A + POLY_LEN] = ord("C")
    unit = np.frombuffer(b"ACGTC", np.uint8)
    t[TANDEM:TANDEM + TANDEM_LEN] = np.tile(unit, TANDEM_LEN // UNIT)
    t[TANDEM - 1] = t[TANDEM + TANDEM_LEN] = ord("G")
    return np.ascontiguousarray(t)


def reads_for(t: np.ndarray, m: int, seed: int) -> np.ndarray:
    """The reads of one length (see the module's text), reverse complements behind the forward reads."""
    n = t.size
    rng = np.random.default_rng(seed)
    win = np.arange(m)
    out = []
    if m <= SEG_LEN:
        starts = set()
        for d in SUBS + (DEL_AT, INS_AT):
            for a in (d - m // 2, d - m // 4, d - (3 * m) // 4, d - 10):
                starts.add(min(max(a, 0), SEG_LEN - m))
        for base in (SEG, EXACT, SUBST, INDEL):
            for a in sorted(starts):
                out.append(t[base + a + win])
        for base in (SEG, SUBST, INDEL):                              # one base of their own changed
            for a in sorted(starts)[::2]:
                r = t[base + a + win].copy()[None, :]
                sr._change(r, [0], 5 if m > 5 else 0, rng)
                out.append(r[0])
    for o in (30, 900, 1_700, 2_500, 3_300):                          # unique regions
        out.append(t[o + win])
    for o in (POLY_A - m // PIECES, POLY_A + 3, POLY_A + POLY_LEN - m // 2):   # the poly-A run and its flanks
        out.append(t[min(max(o, 0), n - m) + win])
    for o in (TANDEM, TANDEM + 2, TANDEM + TANDEM_LEN - m - UNIT, TANDEM - 7):  # the tandem repeat
        out.append(t[min(max(o, 0), n - m) + win])
    for o in list(range(16)) + list(range(n - m - 15, n - m + 1)):    # X within 2w of a text end
        out.append(t[o + win])
    out = np.stack(out)
    return np.ascontiguousarray(np.concatenate([out, revcomp_def(out)]))


def piece_bounds(m: int, pieces: int) -> list:
    ln = m // pieces
    return [(j * ln, ln if j < pieces - 1 else m - (pieces - 1) * ln) for j in range(pieces)]


def piece_seeds(w: vr.World, tasks: np.ndarray, pieces: int):
    """(intervals, spans) uint32 [T, pieces, 2]: the rows of every piece of every
    task in the model's suffix array ('$' suffix first), by binary search on the
    sorted len-mers; a piece of no bases stays an ignored slot (0, 0)."""
    T, m = tasks.shape
    iv, sp = np.zeros((T, pieces, 2), np.uint32), np.zeros((T, pieces, 2), np.uint32)
    padded = np.concatenate([ACGT[w.codes], np.full(m + 1, 1, np.uint8)])   # past the text: below every base
    for j, (start, ln) in enumerate(piece_bounds(m, pieces)):
        if ln == 0:
            continue
        mers = np.ascontiguousarray(padded[w.sa[:, None] + np.arange(ln)[None, :]]).view("S%d" % ln).reshape(-1)
        assert (mers[1:] >= mers[:-1]).all()
        pat = np.ascontiguousarray(ACGT[code_of(tasks[:, start:start + ln])]).view("S%d" % ln).reshape(-1)
        iv[:, j, 0] = np.searchsorted(mers, pat, "left")
        iv[:, j, 1] = np.searchsorted(mers, pat, "right")
        sp[:, j] = (start, ln)
    return iv, sp


def truncated(w: vr.World, m: int, iv: np.ndarray, sp: np.ndarray, s: int, occ: int) -> np.ndarray:
    """bool [T]: some slot < s that is not ignored has min(R, rows) - L > occ."""
    rows = w.n + 1
    L, R = iv[:, :s, 0].astype(np.int64), iv[:, :s, 1].astype(np.int64)
    start, ln = sp[:, :s, 0].astype(np.int64), sp[:, :s, 1].astype(np.int64)
    used = (R > L) & (L < rows) & (ln != 0) & (start + ln <= m)
    return (used & (np.minimum(R, rows) - L > occ)).any(axis=1)


class Seeded:
    """One seed set of the tasks of a length: its records, candidates at max_occ 8 and their rows."""

    def __init__(self, w: vr.World, m: int, tasks: np.ndarray, iv: np.ndarray, sp: np.ndarray, bands=BANDS, occ=8):
        self.w, self.m, self.iv, self.sp, self.S = w, m, iv, sp, iv.shape[1]
        self.a = ar.Aligned(w, tasks, vr.candidates(w, tasks, iv, sp, occ), bands=bands)

    def trunc(self, s: int, occ: int) -> np.ndarray:
        return truncated(self.w, self.m, self.iv, self.sp, s, occ)


def far_best(a: ar.Aligned, hits_x: np.ndarray, s: int, occ: int, band: int, exclude: bool = True):
    """(E2, B2_min, B2_max, counted, placed) of every task: E2 = BIG where no far
    pair exists.  exclude=False drops the |b - X| <= 2w exclusion: every valid
    cell of a counted candidate takes part -- what the record must not be."""
    c, T = a.c, a.T
    X = np.asarray(hits_x, np.uint32).astype(np.int64)
    placed = X != NONE
    sel = (c.slot[a.sc] < s) & (c.rank[a.sc] < occ)
    t, o, A = c.task[a.sc][sel], c.origin[a.sc][sel], a.cand_rows(band)[sel]
    can = placed[t] & (np.abs(o - X[t]) > band)
    counted = np.bincount(t[can], minlength=T).astype(np.int64)
    b = o[:, None] + np.arange(-band, band + 1, dtype=np.int64)[None, :]
    far = (A < INF) & placed[t][:, None]
    far &= (np.abs(b - X[t][:, None]) > 2 * band) if exclude else can[:, None]
    E2, bmin, bmax = np.full(T, BIG, np.int64), np.full(T, BIG, np.int64), np.full(T, -1, np.int64)
    if t.size:
        np.minimum.at(E2, t, np.where(far, A, BIG).min(axis=1))
        at = far & (A == E2[t][:, None])
        np.minimum.at(bmin, t, np.where(at, b, BIG).min(axis=1))
        np.maximum.at(bmax, t, np.where(at, b, -1).max(axis=1))
    return E2, bmin, bmax, counted, placed


def second_records(a: ar.Aligned, hits_x: np.ndarray, s: int, occ: int, band: int, max_second: int, trunc: np.ndarray,
                   rows=slice(None), exclude: bool = True) -> np.ndarray:
    """uint32 [T, 2]: the second record of every task (hits_x: word x of the T
    hits; trunc: truncated() of the same s and occ)."""
    E2, bmin, bmax, counted, placed = far_best(a, hits_x, s, occ, band, exclude)
    ok = placed & (E2 < BIG) & (E2 <= max_second)
    tail = np.where(placed, np.where(trunc, TRUNC, 0) | (counted << SCORED_SHIFT), 0)
    out = np.empty((a.T, 2), np.uint32)
    out[:, 0] = np.where(ok, bmin, NONE)
    out[:, 1] = np.where(ok, E2 | np.where(bmax - bmin > 2 * band, MULTI, 0), 0) | tail
    return out[rows]


def quality(hits: np.ndarray, second: np.ndarray, strands: int, max_second: int) -> np.ndarray:
    """uint32 [T, 2]: (q, gap) of every task from its hit, its second and, in BOTH mode, the read's other strand."""
    h, s2 = np.asarray(hits, np.uint32).reshape(-1, 2).astype(np.int64), np.asarray(second, np.uint32).reshape(-1, 2).astype(np.int64)
    T = h.shape[0]
    E, placed = h[:, 1] & EDIT_MASK, h[:, 0] != NONE
    C = np.full(T, int(max_second) + 1, np.int64)
    C = np.where(s2[:, 0] != NONE, np.minimum(C, s2[:, 1] & EDIT_MASK), C)
    trunc = (s2[:, 1] & TRUNC) != 0
    same_rev = np.zeros(T, bool)
    if strands == sr.BOTH:
        u = np.arange(T) ^ 1
        C = np.where(h[u, 0] != NONE, np.minimum(C, E[u]), C)
        trunc = trunc | trunc[u]
        same_rev = (h[u, 0] != NONE) & (E[u] == E) & (np.arange(T) % 2 == 1)
    gap = np.where(same_rev, 0, np.maximum(C - E, 0))
    gap = np.minimum(gap, 0xFFFFFFFF)
    q = np.minimum(MAPQ_MAX, MAPQ_PER_EDIT * gap)
    q = np.where(trunc, np.minimum(q, MAPQ_TRUNCATED), q)
    out = np.zeros((T, 2), np.uint32)
    out[:, 0], out[:, 1] = np.where(placed, q, 0), np.where(placed, gap, 0)
    return out


def assert_not_vacuous(w: vr.World, m: int, g: Seeded, p: Seeded, what) -> None:
    """What the tasks of one (K, length >= 100) must show at band 3 on the model
    alone, by the greedy seeds (S = 8) and by the piece seeds each on its own;
    the last condition ties the two sets together."""
    band, seen = 3, {}
    per = {}
    for name, x in (("greedy", g), ("piece", p)):
        hits = ar.records(x.a, x.S, 8, band, m)
        E = ar.edits_of(hits)
        E2, bmin, bmax, counted, placed = far_best(x.a, hits[:, 0], x.S, 8, band)
        sec = second_records(x.a, hits[:, 0], x.S, 8, band, m, x.trunc(x.S, 8))
        low = second_records(x.a, hits[:, 0], x.S, 8, band, 1, x.trunc(x.S, 8))     # max_second = 1
        have = placed & (E2 < BIG)
        multi = (hits[:, 1] & MULTI) != 0
        # the header's consequences, on the model
        assert (E2[have] >= E[have]).all(), (what, name)
        assert np.array_equal(placed & have & (E2 == E), placed & multi), (what, name, "E2 = E <=> MULTI")
        assert (counted <= hits[:, 1] >> SCORED_SHIFT).all(), (what, name)
        cond = {
            "E2 = E + 1": have & (E2 == E + 1),
            "E2 = E + 2": have & (E2 == E + 2),
            "E2 = E with MULTI": have & (E2 == E) & multi,
            "no far pair": placed & ~have,
            "a far pair above max_second = 1, so no record": have & (E2 > 1) & (low[:, 0] == NONE) & (low[:, 1] >> SCORED_SHIFT > 0),
            "TRUNCATED": placed & ((sec[:, 1] & TRUNC) != 0),
            "counted < scored": placed & (counted < (hits[:, 1] >> SCORED_SHIFT)),
            "a second with MULTI": (sec[:, 0] != NONE) & ((sec[:, 1] & MULTI) != 0),
            "the exclusion changes the record":
                (sec != second_records(x.a, hits[:, 0], x.S, 8, band, m, x.trunc(x.S, 8), exclude=False)).any(axis=1),
        }
        for k, v in cond.items():
            seen[(name, k)] = bool(v.any())
        # a candidate with w < |o - X| <= 3w whose near cells hold less than its far ones
        c, a = x.a.c, x.a
        sel = c.slot[a.sc] < x.S
        t, o, A = c.task[a.sc][sel], c.origin[a.sc][sel], a.cand_rows(band)[sel]
        X = hits[:, 0].astype(np.int64)[t]
        b = o[:, None] + np.arange(-band, band + 1)[None, :]
        near = np.abs(b - X[:, None]) <= 2 * band
        ring = placed[t] & (np.abs(o - X) > band) & (np.abs(o - X) <= 3 * band)
        less = np.where(near, A, BIG).min(axis=1) < np.where(~near, A, BIG).min(axis=1)
        seen[(name, "near cells below far ones")] = bool((ring & less).any())
        per[name] = (E, have, E2)
    for k, v in seen.items():
        assert v, (what, "no task with", k)
    (Eg, haveg, _), (Ep, havep, E2p) = per["greedy"], per["piece"]
    assert ((Eg == 0) & ~haveg & havep & (E2p >= 1) & (E2p < BIG)).any(), (what, "no exact task that only piece seeds give a second")


_cache = {}


def world(K, oracle_mod) -> dict:
    """The World, the K = 1, 2 indexes and, per length, the reads, the tasks of
    BOTH and per K the greedy Seeded (S = 8) and the piece Seeded (the same for
    both K); the conditions are asserted here, on the model alone."""
    if _cache:
        return _cache
    t = text()
    w = vr.World(t)
    idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
    img1 = idx[1].image()
    search = lambda q: oracle_mod.search(img1, q)[0]   # noqa: E731
    cases = {}
    for m in LENGTHS:
        q = reads_for(t, m, 26_000 + m)
        both = sr.tasks_of(q, sr.BOTH)
        piv, psp = piece_seeds(w, both, PIECES)
        piece = Seeded(w, m, both, piv, psp)
        greedy = {}
        for k in (1, 2):
            iv, sp, _ = sr.reference(search, both, k, 8)
            greedy[k] = Seeded(w, m, both, iv, sp)
            if m >= 100:
                assert_not_vacuous(w, m, greedy[k], piece, (k, m))
        q.setflags(write=False)
        cases[m] = (q, both, greedy, piece)
    _cache.update(dict(world=w, text=t, idx=idx, cases=cases, search=search))
    return _cache
