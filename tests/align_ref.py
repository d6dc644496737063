"""Align seeds: the model, the reads and the non-vacuity conditions shared by
test_align_host.py and test_align_gpu.py.

The model restates the definition of kstep_fmi.h ("align seeds") in numpy on
the text's codes and a brute-force suffix array (verify_ref.World); it calls
nothing from the library.  The candidates are verify_ref.candidates' -- slots,
rows and the scored test are those of "verify seeds" -- and row0() runs the
banded recurrence for all of them at once, with a Python loop over the read's
rows only (the chain of skipped text bases inside a row is a running minimum
over the band).  records() forms both words of every task's record for any cut
of S, max_occ, band and max_edits.

Reads of one (text, length): verify_ref.reads_for, then, each followed by its
reverse complement:
  * one base deleted and one base inserted at each pinned read position of an
    otherwise exact, locally unique window (refilled from the text: the read
    keeps m bases);
  * a 3-base deletion and a 3-base insertion at m // 2;
  * one deletion at m // 3 together with one insertion at 2m // 3;
  * single indels in reads at the origins 0 .. 15 and n - m - 15 .. n - m, where
    band cells fall off the text: every such origin gets one deletion and one
    insertion, the pinned positions taken by turns over the origins (all eight
    positions at all 32 origins would be a thousand reads per length);
  * a single deletion and a single insertion inside the copied segment (two
    distant placements);
  * a window with a short tandem repeat spliced in: the two bases before read
    position 6 twice more."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import seed_ref as sr
import verify_ref as vr
from skip_texts import ACGT
from strand_reads import code_of, revcomp_def

NONE, EDIT_MASK, MULTI, SCORED_SHIFT = vr.NONE, vr.MISM_MASK, vr.MULTI, vr.SCORED_SHIFT
MAX_BAND = 15
LENGTHS = (1, 2, 3, 15, 16, 17, 33, 100, 101, 127, 128, 129, 255, 256)
BANDS = (0, 1, 2, 3, 8, 15)
SEEDS, STRANDS, OCCS = vr.SEEDS, vr.STRANDS, vr.OCCS
INF = 10_000                     # above every finite value (<= 256 + 15), small enough for int16 sums
PINNED = lambda m: (1, 15, 16, 17, m // 2, m - 17, m - 16, m - 2)   # noqa: E731


def edit_bounds(m: int):
    return (0, 1, m)


def pinned(m: int) -> list:
    return sorted({p for p in PINNED(m) if 1 <= p <= m - 2})


def other_base(t: np.ndarray, at: int, rng) -> int:
    """A base that is neither t[at] nor t[at - 1]."""
    no = {int(t[at]), int(t[at - 1])} if at > 0 else {int(t[at])}
    return int(rng.choice([int(b) for b in ACGT if int(b) not in no]))


def deleted(t: np.ndarray, a: int, m: int, p: int, k: int = 1) -> np.ndarray:
    """The window at a without the k text bases from a + p on, m bases: refilled
    at its right end, or at its left end where the text ends first."""
    if a + m + k <= t.size:
        return np.concatenate([t[a:a + p], t[a + p + k:a + m + k]])
    return np.concatenate([t[a - k:a + p - k], t[a + p:a + m]])


def inserted(t: np.ndarray, a: int, m: int, p: int, rng, k: int = 1) -> np.ndarray:
    """The window at a with k foreign bases before its base p, cut to m bases."""
    new = [other_base(t, a + p, rng)]
    while len(new) < k:
        new.append(int(ACGT[(int(np.searchsorted(ACGT, new[-1])) + 1 + int(rng.integers(0, 3))) % 4]))
    return np.concatenate([t[a:a + p], np.asarray(new, np.uint8), t[a + p:a + m - k]])


def indel_reads(t: np.ndarray, m: int, seed: int) -> np.ndarray:
    """The reads this file adds to verify_ref.reads_for (see the module's text), without their reverse complements."""
    n = t.size
    rng = np.random.default_rng(seed)
    src, dst, ln = vr.copy_of(t)
    away = (src + dst) // 2
    pins = pinned(m)
    out = []
    for p in pins:
        out.append(deleted(t, away, m, p))
        out.append(inserted(t, away, m, p, rng))
    if m >= 12:
        out.append(deleted(t, away, m, m // 2, 3))
        out.append(inserted(t, away, m, m // 2, rng, 3))
        two = np.concatenate([t[away:away + m // 3], t[away + m // 3 + 1:away + 2 * m // 3 + 1],
                              np.asarray([other_base(t, away + 2 * m // 3 + 1, rng)], np.uint8),
                              t[away + 2 * m // 3 + 1:away + m]])
        out.append(two)
    if pins:
        ends = list(range(16)) + list(range(n - m - 15, n - m + 1))
        for i, a in enumerate(ends):
            p = pins[i % len(pins)]
            out.append(deleted(t, a, m, p))
            out.append(inserted(t, a, m, p, rng))
        if m + 1 <= ln - 8:
            out.append(deleted(t, src + 5, m, m // 2))
            out.append(inserted(t, src + 5, m, m // 2, rng))
    if m >= 24:
        unit = t[away + 4:away + 6]
        out.append(np.concatenate([t[away:away + 6], unit, unit, t[away + 6:away + m - 4]]))
    for r in out:
        assert r.size == m
    return np.stack(out) if out else np.empty((0, m), np.uint8)


def reads_for(t: np.ndarray, m: int, seed: int) -> np.ndarray:
    extra = indel_reads(t, m, seed + 1)
    return np.ascontiguousarray(np.concatenate([vr.reads_for(t, m, seed), extra, revcomp_def(extra)]))


def row0(w: vr.World, pc: np.ndarray, o: np.ndarray, band: int) -> np.ndarray:
    """int16 [N, 2 * band + 1]: A(0, d), d = -band .. band, of N candidates (pc:
    their reads' codes [N, m]; o: their origins), INF for invalid cells.

    The work arrays are [cell, candidate] with the band's cells in the order r =
    band - d, so that the chain of skipped text bases (d + 1 -> d) runs forward.
    The text positions a candidate's cells stand at are laid out once, falling:
    q[y] = o + m + band - y, and cell (i, r) stands at q[m - i + r], so row i
    looks at the slice [m - i, m - i + 2 * band + 1).  Penalties of INF stand for
    the transitions and cells that do not exist; finite values stay below 300
    and sums below 3 * INF + 32, inside int16."""
    n, (N, m), B = w.n, pc.shape, 2 * band + 1
    q = o.astype(np.int64)[None, :] + (m + band) - np.arange(m + B, dtype=np.int64)[:, None]
    cell = np.where((q >= 0) & (q <= n), 0, INF).astype(np.int16)          # the cell is valid
    diag = np.where((q >= 0) & (q < n), 0, INF).astype(np.int16)           # ... and has a text base: j < n
    tw = np.where(diag == 0, w.codes[np.clip(q, 0, max(n - 1, 0))], 9).astype(np.int8)
    pt = np.ascontiguousarray(pc.T).astype(np.int8)
    r = np.arange(B, dtype=np.int16)[:, None]
    A = cell[:B].copy()                                                    # row m
    for i in range(m - 1, -1, -1):
        y = m - i
        base = A + (pt[i][None, :] != tw[y:y + B])                         # P[i] on T[j] ...
        base += diag[y:y + B]                                              # ... when j < n
        np.minimum(base[:-1], A[1:] + 1, out=base[:-1])                    # a read base with no text base: from d - 1
        base += cell[y:y + B]
        # text bases skipped: A(i, r) = min over r' <= r of base(r') + r - r' (every cell past a valid r' has j < n)
        base -= r
        np.minimum.accumulate(base, axis=0, out=base)
        base += r
        np.maximum(base, cell[y:y + B], out=base)                          # the chain does not enter an invalid cell
        A = np.minimum(base, INF)
    return np.ascontiguousarray(A[::-1].T)


class Rows:
    """Row 0 of every (task, origin) pair of one or more candidate lists, per band."""

    def __init__(self, w: vr.World, tasks: np.ndarray, cands, bands=None, fill=True):
        self.bands = BANDS if bands is None else bands
        self.w, self.n1 = w, w.n + 1
        keys = [c.task[c.why == vr.SCORED] * self.n1 + c.origin[c.why == vr.SCORED] for c in cands]
        self.keys = np.unique(np.concatenate(keys)) if keys else np.empty(0, np.int64)
        self.pc = code_of(tasks)[self.keys // self.n1]
        self.o = self.keys % self.n1
        self.rows = {}
        if fill:
            for b in self.bands:
                self.fill(b)

    def fill(self, band: int) -> None:
        self.rows[band] = row0(self.w, self.pc, self.o, band) if self.keys.size else np.empty((0, 2 * band + 1), np.int16)


class Aligned:
    """verify_ref.Cands with, per band, row 0 of every scored candidate."""

    def __init__(self, w: vr.World, tasks: np.ndarray, c: vr.Cands, bands=None, rows: Rows = None):
        self.c, self.T, self.n = c, c.T, w.n
        self.sc = np.flatnonzero(c.why == vr.SCORED)
        self.r = rows if rows is not None else Rows(w, tasks, [c], bands)
        self.back = np.searchsorted(self.r.keys, c.task[self.sc] * (w.n + 1) + c.origin[self.sc])
        self._best = {}

    def cand_rows(self, band: int) -> np.ndarray:
        """[scored candidates, 2 * band + 1]"""
        return self.r.rows[band][self.back].astype(np.int64)

    def best(self, s: int, occ: int, band: int):
        """(E, B_min, B_max, scored) of every task from its scored candidates in slots < s and ranks < occ."""
        if (s, occ, band) not in self._best:
            c, T, big = self.c, self.T, 1 << 40
            sel = (c.slot[self.sc] < s) & (c.rank[self.sc] < occ)
            t, o, A = c.task[self.sc][sel], c.origin[self.sc][sel], self.cand_rows(band)[sel]
            scored = np.bincount(t, minlength=T).astype(np.int64)
            E, bmin, bmax = np.full(T, big, np.int64), np.full(T, big, np.int64), np.full(T, -1, np.int64)
            if t.size:
                np.minimum.at(E, t, A.min(axis=1))
                at = A == E[t][:, None]
                b = o[:, None] + np.arange(-band, band + 1, dtype=np.int64)[None, :]
                np.minimum.at(bmin, t, np.where(at, b, big).min(axis=1))
                np.maximum.at(bmax, t, np.where(at, b, -1).max(axis=1))
            assert (E[scored > 0] < INF).all()
            self._best[(s, occ, band)] = (E, bmin, bmax, scored)
        return self._best[(s, occ, band)]


def records(a: Aligned, s: int, occ: int, band: int, max_edits: int, rows=slice(None)) -> np.ndarray:
    """uint32 [T, 2]: the record of every task from its scored candidates in
    slots < s and ranks < occ: E the least edits, B_min and B_max over every
    (candidate, d) that attains E, MULTI iff B_max - B_min > 2 * band."""
    E, bmin, bmax, scored = a.best(s, occ, band)
    ok = (scored > 0) & (E <= max_edits)
    assert (bmin[ok] >= 0).all() and (bmax[ok] <= a.n).all()
    out = np.empty((a.T, 2), np.uint32)
    out[:, 0] = np.where(ok, bmin, NONE)
    out[:, 1] = np.where(ok, E | np.where(bmax - bmin > 2 * band, MULTI, 0), 0) | (scored << SCORED_SHIFT)
    return out[rows]


def edits_of(rec: np.ndarray) -> np.ndarray:
    """int64 [T]: E of every record, -1 where x = NONE."""
    return np.where(rec[:, 0] == NONE, -1, (rec[:, 1] & EDIT_MASK).astype(np.int64))


def assert_not_vacuous(w: vr.World, m: int, a: Aligned, what) -> None:
    """What the tasks of one (text, K, length >= 48) must show on the model
    alone (a: BOTH at S = 8, max_occ = 8, every band)."""
    c = a.c
    e = {b: edits_of(records(a, 8, 8, b, m)) for b in (0, 1, 2, 3)}
    assert ((e[1] == 1) & (e[0] > 3)).any(), (what, "no task with E = 1 at band 1 and more than 3 at band 0")
    assert ((e[3] == 3) & ((e[2] > 3) | (e[2] < 0))).any(), (what, "no task with E = 3 at band 3 and more than 3 at band 2")
    assert ((e[1] == 2) & (e[0] > 3)).any(), (what, "no task with E = 2 from a deletion and an insertion")
    # invalid band cells at either text end, with E still 1
    r15 = a.cand_rows(15)
    t, o = c.task[a.sc], c.origin[a.sc]
    one = edits_of(records(a, 8, 8, 15, m))[t] == 1
    hit = r15.min(axis=1) == 1
    assert (one & hit & (o < 15)).any() and (r15[one & hit & (o < 15)] >= INF).any(), (what, "no clipped band at the text's start")
    assert (one & hit & (o + m > w.n - 15)).any(), (what, "no clipped band at the text's end")
    full = {b: records(a, 8, 8, b, m) for b in (1, 3)}
    for b, rec in full.items():
        assert ((rec[:, 0] != NONE) & ((rec[:, 1] & MULTI) != 0)).any(), (what, "no MULTI at band", b)
    # B_max > B_min without MULTI: a task whose record has no MULTI while two cells attain E at different begins
    r1 = a.cand_rows(1)
    E1 = edits_of(full[1])
    cells = (r1 == E1[t][:, None]).sum(axis=1)
    spread = np.zeros(a.T, bool)
    spread[t[cells > 1]] = True
    assert (spread & (full[1][:, 0] != NONE) & ((full[1][:, 1] & MULTI) == 0)).any(), (what, "no B_max > B_min without MULTI")
    # two slots on either side of an indel: two origins, both attain E = 1, one begin position
    best = r1.min(axis=1) == E1[t]
    lo, hi = np.full(a.T, 1 << 40, np.int64), np.full(a.T, -1, np.int64)
    np.minimum.at(lo, t[best], o[best])
    np.maximum.at(hi, t[best], o[best])
    slo, shi = np.full(a.T, 99, np.int64), np.full(a.T, -1, np.int64)
    np.minimum.at(slo, t[best], c.slot[a.sc][best])
    np.maximum.at(shi, t[best], c.slot[a.sc][best])
    bmin, bmax = np.full(a.T, 1 << 40, np.int64), np.full(a.T, -1, np.int64)
    at = r1 == E1[t][:, None]
    b = o[:, None] + np.arange(-1, 2)[None, :]
    np.minimum.at(bmin, t, np.where(at, b, 1 << 40).min(axis=1))
    np.maximum.at(bmax, t, np.where(at, b, -1).max(axis=1))
    assert ((E1 == 1) & (hi > lo) & (shi > slo) & (bmin == bmax)).any(), (what, "no two slots with one begin position")
    zero = records(a, 8, 8, 3, 0)
    assert ((zero[:, 0] == NONE) & (zero[:, 1] >> SCORED_SHIFT > 0)).any(), (what, "no NONE under max_edits = 0")


_cache = {}


def world(K, oracle_mod) -> dict:
    """Per text: the World, the K = 1, 2 indexes and, per length, the reads, the
    seed records of BOTH at S = 8 per K (seed_ref.reference on the CPU oracle),
    their candidates at max_occ = 8 and the aligned rows of every band; the
    conditions are asserted here, on the model alone.  Built once per session."""
    if _cache:
        return _cache
    out, jobs = {}, []
    for name, t in vr.texts().items():
        w = vr.World(t)
        idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
        img1 = idx[1].image()
        search = lambda q, img1=img1: oracle_mod.search(img1, q)[0]   # noqa: E731
        cases = {}
        for m in LENGTHS:
            q = reads_for(t, m, 17_000 + m)
            both = sr.tasks_of(q, sr.BOTH)
            per_k, seeds = {}, {}
            for k in (1, 2):
                iv, sp, _ = sr.reference(search, both, k, 8)
                seeds[k] = (iv, sp, vr.candidates(w, both, iv, sp, 8))
            rows = Rows(w, both, [seeds[k][2] for k in (1, 2)], fill=False)   # one table for both K
            jobs += [(m * (2 * b + 1) * rows.keys.size, rows, b) for b in BANDS]
            for k in (1, 2):
                iv, sp, c = seeds[k]
                for x in (iv, sp):
                    x.setflags(write=False)
                per_k[k] = (iv, sp, Aligned(w, both, c, rows=rows))
            q.setflags(write=False)
            cases[m] = (q, both, per_k)
        out[name] = dict(world=w, text=t, idx=idx, cases=cases, search=search)
    # the rows of every (text, length, band): numpy releases the interpreter lock, so a few threads share the work
    jobs.sort(key=lambda j: -j[0])
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        list(pool.map(lambda j: j[1].fill(j[2]), jobs))
    for name, x in out.items():
        for m, (q, both, per_k) in x["cases"].items():
            if m >= 48:
                for k in (1, 2):
                    assert_not_vacuous(x["world"], m, per_k[k][2], (name, k, m))
    _cache.update(out)
    return _cache
