"""Verify seeds: the model, the texts, the reads and the non-vacuity conditions
shared by test_verify_host.py and test_verify_gpu.py.

The model restates the definition of kstep_fmi.h ("verify seeds") in numpy on
three things only: the text's codes, a brute-force suffix array with the '$'
suffix first (util.suffix_array, as walk_model.World builds one) and seed
records -- seed_ref.reference's, or hand-made ones.  It calls nothing from the
library.

candidates() lists every candidate of every task once, at the largest S and
max_occ a test uses; records() cuts that list down to any smaller S and max_occ
(a slot's candidates are its first rows, a task's slots its first records) and
forms the two words of each task's record under any max_mism."""
import numpy as np

import seed_ref as sr
import util
from skip_texts import ACGT
from strand_reads import code_of, revcomp_def

NONE, MISM_MASK, MULTI, SCORED_SHIFT = 0xFFFFFFFF, 0xFFFF, 0x10000, 20
SCORED, OFF_START, OFF_END, NO_SUFFIX = 0, 1, 2, 3          # why a candidate was or was not scored
LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 99, 100, 101, 127, 128, 129, 255, 256)
SEEDS, STRANDS, OCCS = (1, 4, 8), (sr.FWD, sr.REV, sr.BOTH), (1, 2, 8)
SMALL = (1_005, 1_008, 1_009)                                # n % 16 = 13, 0, 1
SMALL_COPY = (100, 600, 300)                                 # t[600:900] = t[100:400]
MAIN_COPY = (2_000, 9_000, 1_500)                            # seed_ref.main_text()
PINNED = lambda m: (0, m - 1, 15, 16, 31, 32, m - 16, m - 17)   # noqa: E731


def mism_bounds(m: int):
    return (0, 1, m)


def small_text(n: int) -> np.ndarray:
    """n random bases with one 300-base copy, away from both ends."""
    t = ACGT[np.random.default_rng(5_000 + n).integers(0, 4, size=n)].copy()
    src, dst, ln = SMALL_COPY
    t[dst:dst + ln] = t[src:src + ln]
    return t


def texts() -> dict:
    out = {"main": sr.main_text()}
    for n in SMALL:
        out["n%d" % n] = small_text(n)
    return out


def copy_of(t: np.ndarray):
    return MAIN_COPY if t.size > 2_000 else SMALL_COPY


class World:
    """A text's codes and its suffix array, '$' suffix first: sa[0] = n."""

    def __init__(self, text: np.ndarray):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        self.n = int(self.text.size)
        self.codes = code_of(self.text).astype(np.uint8)
        self.sa = np.asarray(util.suffix_array(self.text.tobytes() + b"$"), dtype=np.int64)
        assert self.sa.size == self.n + 1 and self.sa[0] == self.n


def quarter_reads(t: np.ndarray, m: int, seed: int, n_reads: int) -> np.ndarray:
    """seed_ref.main_reads' recipe for a text without its two-strand region:
    equal quarters with 0, 1, 2 and 3 changed bases, the last with N and
    lowercase bytes on top, odd rows reverse complements."""
    rng = np.random.default_rng(seed)
    g = n_reads // 4
    st = rng.integers(0, t.size - m + 1, size=n_reads)
    q = t[st[:, None] + np.arange(m)[None, :]].copy()
    for c in (1, 2, 3):
        for i in range(g):
            for p in sr._spread(m, i, c, rng):
                sr._change(q, [c * g + i], p, rng)
    for i in range(g):
        r = 3 * g + i
        if i % 3 == 0:
            q[r, int(rng.integers(0, m))] = ord("N")
        elif i % 3 == 1:
            q[r] = np.char.lower(q[r:r + 1].view("S1")).view(np.uint8)
        else:
            q[r, int(rng.integers(0, m))] = ord("n")
    q[1::2] = revcomp_def(q[1::2])
    return np.ascontiguousarray(q)


def n_base(t: np.ndarray) -> int:
    return 192 if t.size > 2_000 else 64


def reads_for(t: np.ndarray, m: int, seed: int) -> np.ndarray:
    """The reads of one (text, length): the quartered base reads (the first
    n_base(t) rows: row r of quarter c = r // (n_base / 4) has c changed bases
    and was drawn from the forward strand when r is even), then, each followed
    by its reverse complement so that both strands see it:
      * exact reads at the 16 first and the 16 last origins (every window shift,
        origins 0 and n - m);
      * a prefix of the text behind 1 .. 17 foreign bases, a suffix of the text
        before 1 .. 17 foreign bases (the seed occurs, the origin lies off the
        text);
      * one substitution at each pinned base of an otherwise exact read;
      * exact reads inside the copied segment (two origins)."""
    n = t.size
    rng = np.random.default_rng(seed)
    base = sr.main_reads(t, m, seed, n_base(t))[:n_base(t)] if n > 2_000 else quarter_reads(t, m, seed, n_base(t))
    win = np.arange(m)
    extra = [t[o + win] for o in list(range(16)) + list(range(n - m - 15, n - m + 1))]
    for k in range(1, min(17, m - 1) + 1):
        foreign = ACGT[rng.integers(0, 4, size=k)]
        extra.append(np.concatenate([foreign, t[:m - k]]))
        extra.append(np.concatenate([t[n - (m - k):], foreign]))
    src, dst, ln = copy_of(t)
    away = (src + dst) // 2                                  # between the copies: unique windows
    for p in sorted({p for p in PINNED(m) if 0 <= p < m}):
        r = t[away + win].copy()[None, :]
        sr._change(r, [0], p, rng)
        extra.append(r[0])
    for o in (src + 3, src + ln - m - 2):
        if m <= ln - 8:
            extra.append(t[o + win])
    extra = np.stack(extra)
    return np.ascontiguousarray(np.concatenate([base, extra, revcomp_def(extra)]))


class Cands:
    """Every candidate of every task: task, slot, rank (its row's place in the
    slot), why (SCORED or the reason it was skipped), origin and mism (scored
    ones only)."""

    def __init__(self, T, rows):
        self.T = T
        a = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        self.task, self.slot, self.rank, self.why, self.origin, self.mism = (a[:, i] for i in range(6))


def candidates(w: World, tasks: np.ndarray, iv: np.ndarray, sp: np.ndarray, max_occ: int, sa=None) -> Cands:
    """The definition's candidates: slot s of task t with {L, R}, {start, len}
    gives the rows L .. below min(R, rows, L + max_occ); ignored when R <= L,
    L >= rows, len == 0 or start + len > m; row r: p = sa[r], o = p - start,
    scored iff sa[r] < rows, p >= start and o + m <= n."""
    n, rows = w.n, w.n + 1
    sa = w.sa if sa is None else sa
    T, m = tasks.shape
    pc = code_of(tasks)
    out = []
    for t in range(T):
        for s in range(iv.shape[1]):
            L, R, start, ln = int(iv[t, s, 0]), int(iv[t, s, 1]), int(sp[t, s, 0]), int(sp[t, s, 1])
            if R <= L or L >= rows or ln == 0 or start + ln > m:
                continue
            for k, r in enumerate(range(L, min(R, rows, L + max_occ))):
                p = int(sa[r])
                if p >= rows:
                    out.append((t, s, k, NO_SUFFIX, -1, -1))
                elif p < start:
                    out.append((t, s, k, OFF_START, -1, -1))
                elif p - start + m > n:
                    out.append((t, s, k, OFF_END, -1, -1))
                else:
                    o = p - start
                    out.append((t, s, k, SCORED, o, int(np.count_nonzero(pc[t] != w.codes[o:o + m]))))
    return Cands(T, out)


def records(c: Cands, s: int, occ: int, max_mism: int, rows=slice(None)) -> np.ndarray:
    """uint32 [T, 2]: the record of every task from its scored candidates in
    slots < s and ranks < occ -- the minimum of (mism, origin), MULTI iff two
    distinct origins attain that mism, scored << 20."""
    T, big = c.T, 1 << 40
    sel = (c.why == SCORED) & (c.slot < s) & (c.rank < occ)
    t, mm, o = c.task[sel], c.mism[sel], c.origin[sel]
    scored = np.bincount(t, minlength=T).astype(np.int64)
    assert scored.max(initial=0) <= 8 * 256
    best = np.full(T, big, np.int64)
    np.minimum.at(best, t, mm)
    at = mm == best[t]
    omin, omax = np.full(T, big, np.int64), np.full(T, -1, np.int64)
    np.minimum.at(omin, t[at], o[at])
    np.maximum.at(omax, t[at], o[at])
    ok = (scored > 0) & (best <= max_mism)
    out = np.empty((T, 2), np.uint32)
    out[:, 0] = np.where(ok, omin, NONE)
    out[:, 1] = np.where(ok, best | np.where(omax != omin, MULTI, 0), 0) | (scored << SCORED_SHIFT)
    return out[rows]


def strand_rows(strands: int):
    """The tasks of a strand mode among those of BOTH."""
    return {sr.FWD: slice(0, None, 2), sr.REV: slice(1, None, 2), sr.BOTH: slice(None)}[strands]


def assert_not_vacuous(w: World, m: int, reads: np.ndarray, c: Cands, seeds, what) -> None:
    """What the tasks of one (text, K, length >= 48) must show on the model
    alone (c: the candidates of BOTH at S = 8, max_occ = 8; seeds: the seed
    records (intervals, spans) they came from)."""
    full = records(c, 8, 8, m)
    got = full[:, 0] != NONE
    mism = full[:, 1] & MISM_MASK
    for v in (0, 1, 2, 3):
        assert (got & (mism == v)).any(), (what, "no task with mism", v)
    assert (got & ((full[:, 1] & MULTI) != 0)).any(), (what, "no MULTI")
    zero = records(c, 8, 8, 0)
    assert ((zero[:, 0] == NONE) & (zero[:, 1] >> SCORED_SHIFT > 0)).any(), (what, "no NONE under max_mism = 0")
    assert (c.why == OFF_START).any() and (c.why == OFF_END).any(), (what, "no candidate skipped at a text end")
    # two slots of one task that point at one origin, and no other origin as good: one origin, no MULTI
    sc = c.why == SCORED
    key = c.task[sc] * (w.n + 1) + c.origin[sc]
    order = np.lexsort((c.slot[sc], key))
    k2, s2, t2 = key[order], c.slot[sc][order], c.task[sc][order]
    twice = np.zeros(c.T, bool)
    twice[t2[1:][(k2[1:] == k2[:-1]) & (s2[1:] != s2[:-1])]] = True
    assert twice.any(), (what, "no two slots with one origin")
    assert (twice & got & ((full[:, 1] & MULTI) == 0)).any(), (what, "no such task without MULTI")
    # recall: every read of the one-changed-base quarter maps with <= 1 mismatch on the strand it was drawn from
    g = n_base(w.text) // 4
    r4 = records(c, 4, 8, m)
    for r in range(g, 2 * g):
        t = 2 * r + (r & 1)
        assert r4[t, 0] != NONE and (r4[t, 1] & MISM_MASK) <= 1, (what, "recall", r, r4[t].tolist())


_cache = {}


def world(K, oracle_mod) -> dict:
    """Per text: the World, the K = 1, 2 indexes and, per length, the reads, the
    seed records of BOTH at S = 8 per K (seed_ref.reference on the CPU oracle)
    and their candidates at max_occ = 8; the conditions are asserted here, on
    the model alone.  Built once per session."""
    if _cache:
        return _cache
    out = {}
    for name, t in texts().items():
        w = World(t)
        idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
        img1 = idx[1].image()
        search = lambda q, img1=img1: oracle_mod.search(img1, q)[0]   # noqa: E731
        cases = {}
        for m in LENGTHS:
            q = reads_for(t, m, 7_000 + m)
            both = sr.tasks_of(q, sr.BOTH)
            per_k = {}
            for k in (1, 2):
                iv, sp, _ = sr.reference(search, both, k, 8)
                c = candidates(w, both, iv, sp, 8)
                if m >= 48:
                    assert_not_vacuous(w, m, q, c, (iv, sp), (name, k, m))
                for a in (iv, sp):
                    a.setflags(write=False)
                per_k[k] = (iv, sp, c)
            q.setflags(write=False)
            cases[m] = (q, both, per_k)
        out[name] = dict(world=w, text=t, idx=idx, cases=cases, search=search)
    _cache.update(out)
    return _cache
