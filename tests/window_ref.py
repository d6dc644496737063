"""The model of "place windows / pairs" (kstep_fmi.h): numpy only, nothing
from the library.

Begins.e holds e(b) for EVERY begin position b = 0 .. n of every task, from the
full table A(i, j), 0 <= i <= m, 0 <= j <= n, of the definition: no window, no
max_edits and no scan bound enter it, so a window, a bound on the edits and the
scan bound of the kernel are all under test.  A row of the table is one
min-plus scan: A(i, j) = min over j' >= j of base(i, j') + (j' - j) with
base(i, j') = min(A(i+1, j'+1) + sub, A(i+1, j') + 1), which is a reversed
running minimum of base + j'.

place() cuts records out of it, mate_windows() and pair_hits() restate the
window arithmetic and the pair choice with Python integers and tuples.

world() builds, per text and read length, tasks in BOTH order with the windows
of every kind the tests use, and asserts on the model alone that the kinds are
there (assert_not_vacuous).  pair_table() is a hand-made table of records for
the pair choice with one pair per key of the order.  Nothing here needs a
device or the library."""
import numpy as np

import seed_ref as sr
import verify_ref as vr
from skip_texts import ACGT
from strand_reads import code_of, revcomp_def

NONE = 0xFFFFFFFF
EDITS = 0x0000FFFF
MULTI = 0x00010000
PROPER = 0x00020000
RESCUED = 0x00040000
MAX_LEN = 4096
LENGTHS = (1, 17, 32, 33, 64, 65, 100, 129, 256)
WINDOW_LENS = (1, 33, 400, MAX_LEN)


def edit_bounds(m: int):
    return (0, 1, 8, m)


class Begins:
    """e[t, b] = e(b) of task t for every b in 0 .. n."""

    def __init__(self, w: vr.World, tasks: np.ndarray):
        T, m = tasks.shape
        n = w.n
        pc = code_of(tasks).astype(np.int32)
        tc = w.codes.astype(np.int32)
        j = np.arange(n + 1, dtype=np.int32)[None, :]
        A = np.zeros((T, n + 1), np.int32)                 # row m: the end is free
        for i in range(m - 1, -1, -1):
            base = np.empty((T, n + 1), np.int32)
            base[:, :n] = np.minimum(A[:, 1:] + (pc[:, i:i + 1] != tc[None, :]), A[:, :n] + 1)
            base[:, n] = A[:, n] + 1                        # at n: a read base with no text base
            v = base + j
            A = np.minimum.accumulate(v[:, ::-1], axis=1)[:, ::-1] - j   # any number of skipped text bases first
        self.e, self.n, self.m, self.T = A, n, m, T
        assert (A[:, n] == m).all() and (A <= m).all() and (A >= 0).all()


def place(b: Begins, windows: np.ndarray, max_edits: int, rows=slice(None)) -> np.ndarray:
    """uint32 [T, 2] records of the tasks `rows` with windows [T, 2] = (lo, len)."""
    e = b.e[rows]
    win = np.asarray(windows, np.int64).reshape(-1, 2)
    assert win.shape[0] == e.shape[0] and (win[:, 1] <= MAX_LEN).all()
    out = np.zeros((e.shape[0], 2), np.uint32)
    out[:, 0] = NONE
    for t, (lo, ln) in enumerate(win):
        hi = min(lo + ln - 1, b.n)
        if ln == 0 or lo > hi:
            continue
        v = e[t, lo:hi + 1]
        E = int(v.min())
        if E > max_edits:
            continue
        at = np.flatnonzero(v == E)
        out[t] = (lo + at[0], E | (MULTI if at[-1] > at[0] else 0))
    return out


def concordant(bf: int, br: int, m: int, lo: int, hi: int) -> bool:
    return br >= bf and lo <= br + m - bf <= hi


def mate_windows(hits: np.ndarray, n: int, m: int, min_frag: int, max_frag: int, mode: int) -> np.ndarray:
    h = np.asarray(hits, np.uint32).reshape(-1, 2)
    assert h.shape[0] % 4 == 0
    out = np.zeros_like(h)
    for t in range(h.shape[0]):
        s, u = t & 1, 2 * ((t >> 1) ^ 1) + ((t & 1) ^ 1)
        assert u == t ^ 3
        bu, own = int(h[u, 0]), int(h[t, 0])
        if bu == NONE:
            continue
        if mode == 0 and own != NONE and (concordant(bu, own, m, min_frag, max_frag) if s else
                                          concordant(own, bu, m, min_frag, max_frag)):
            continue
        lo, hi = (bu + min_frag - m, bu + max_frag - m) if s else (bu + m - max_frag, bu + m - min_frag)
        lo, hi = max(lo, 0), min(hi, n)
        if lo <= hi:
            out[t] = (lo, hi - lo + 1)
    return out


def pair_keys(h4, r4, m: int, min_frag: int, max_frag: int) -> list:
    """Every admissible combination of one pair as (key, (f, s_f), (r, s_r)), sorted."""
    out = []
    for k, (f, r) in enumerate(((0, 3), (2, 1))):
        for sf, sr_ in ((0, 0), (0, 1), (1, 0)):
            a, b = (r4 if sf else h4)[f], (r4 if sr_ else h4)[r]
            if int(a[0]) == NONE or int(b[0]) == NONE:
                continue
            bf, br = int(a[0]), int(b[0])
            if not concordant(bf, br, m, min_frag, max_frag):
                continue
            out.append(((int(a[1] & EDITS) + int(b[1] & EDITS), sf + sr_, k, bf, br, sf), (f, sf), (r, sr_)))
    return sorted(out)


def pair_hits(hits: np.ndarray, rescued: np.ndarray, m: int, min_frag: int, max_frag: int) -> np.ndarray:
    h = np.asarray(hits, np.uint32).reshape(-1, 4, 2)
    r = np.asarray(rescued, np.uint32).reshape(-1, 4, 2)
    out = np.zeros_like(h)
    out[:, :, 0] = NONE
    for p in range(h.shape[0]):
        keys = pair_keys(h[p], r[p], m, min_frag, max_frag)
        if keys:
            for task, src in keys[0][1:]:
                rec = (r[p] if src else h[p])[task]
                out[p, task] = (rec[0], int(rec[1] & (EDITS | MULTI)) | PROPER | (RESCUED if src else 0))
            continue
        for q in range(2):
            own = [(int(h[p, 2 * q + s, 1] & EDITS), s) for s in range(2) if int(h[p, 2 * q + s, 0]) != NONE]
            if own:
                s = min(own)[1]
                out[p, 2 * q + s] = (h[p, 2 * q + s, 0], int(h[p, 2 * q + s, 1] & (EDITS | MULTI)))
    return out.reshape(-1, 2)


# ---- texts, reads and windows --------------------------------------------------------------------------------------

def texts() -> dict:
    """n % 16 = 13, 0, 1 (random, one 300-base copy each) and 1 (three tandem stretches and a copy)."""
    import align_worlds as aw
    out = {"n%d" % n: vr.small_text(n) for n in vr.SMALL}
    out["tandem"] = aw.texts()["tandem"]
    assert all(300 <= t.size <= 1_100 for t in out.values())
    return out


def low_texts() -> dict:
    import align_worlds as aw
    t = aw.texts()
    return {k: t[k] for k in ("allA", "cg", "p3")}


def foreign(t: np.ndarray, at: int, k: int, rng) -> np.ndarray:
    """k bases that differ from t[at] and from each other in turn."""
    out, prev = [], int(t[min(at, t.size - 1)])
    for _ in range(k):
        prev = int(rng.choice([b for b in ACGT if int(b) != prev]))
        out.append(prev)
    return np.asarray(out, np.uint8)


def deleted(t, o, m, p, k):
    """m bases of the window at o with k text bases skipped after read position p."""
    return np.concatenate([t[o:o + p], t[o + p + k:o + m + k]])


def inserted(t, o, m, p, k, rng):
    return np.concatenate([t[o:o + p], foreign(t, o + p, k, rng), t[o + p:o + m - k]])


def changed(t, o, m, k, rng):
    r = t[o:o + m].copy()
    for p in rng.choice(m, size=k, replace=False):
        r[p] = ACGT[(int(np.searchsorted(ACGT, r[p])) + int(rng.integers(1, 4))) % 4]
    return r


TIGHT_K = 3      # the tight scan-bound case: this many text bases skipped, max_edits the same


def case(name: str, t: np.ndarray, m: int, seed: int):
    """(reads [N, m], windows [2N, 2], tags): the tasks of BOTH and one window per
    task.  tags[t] names what task t was made for (the conditions look them up)."""
    n = t.size
    rng = np.random.default_rng(seed)
    reads, wins, tags = [], [], []

    def add(read, rc, lo, ln, tag, other=None):
        """read placed on the forward (rc = 0) or reverse strand with window (lo, ln); the other strand's task gets `other`."""
        reads.append(revcomp_def(read[None, :])[0] if rc else read)
        pair = [other if other is not None else (max(lo, 0), ln), (max(lo, 0), ln)]
        if not rc:
            pair.reverse()
        wins.extend(pair)
        tags.extend(["", tag] if rc else [tag, ""])

    room = n - 2 * m - 40
    assert room > 40
    i = 0
    for ln in WINDOW_LENS:
        for kind in ("exact", "subs1", "subs2", "subs8", "subs9", "del1", "ins1", "del18", "ins17", "first", "last"):
            o = int(rng.integers(20, 20 + room))
            rc = i % 2
            i += 1
            off = int(rng.integers(0, ln)) if ln <= 400 else min(o, 700)
            lo = o - off
            if kind == "exact":
                r = t[o:o + m]
            elif kind.startswith("subs"):
                k = int(kind[4:])
                if k > m:
                    continue
                r = changed(t, o, m, k, rng)
            elif kind.startswith("del"):
                k = int(kind[3:])
                if 3 * k > m:
                    continue
                r = deleted(t, o, m, m // 2, k)
            elif kind.startswith("ins"):
                k = int(kind[3:])
                if 3 * k > m:
                    continue
                r = inserted(t, o, m, m // 2, k, rng)
            elif kind == "first":
                r, lo = t[o:o + m], o
            else:
                r, lo = t[o:o + m], o - ln + 1
            add(r, rc, lo, ln, "%s/%d" % (kind, ln))
    # the text's ends: b = n in the window, windows that reach past n, the window (n, 1) whose only placement costs m
    add(t[n - m:], 0, n - m - 5, 33, "end")
    hang = min(3, m - 1)                                    # bases of the read that hang over the text's end
    add(np.concatenate([t[n - m + hang:], foreign(t, n - 1, hang, rng)]), 1, n - 40, 400, "past")
    add(t[:m], 0, n, 1, "only-n")
    add(t[:m], 1, n - 1, MAX_LEN, "at-n")
    add(t[:m], 0, 0, 33, "start")
    add(t[3:m + 3], 1, 0, 0, "len0", other=(0, 0))
    add(t[5:m + 5], 0, n + 1, 33, "beyond")                 # lo > n: no begin position
    # the tight scan-bound case: TIGHT_K text bases skipped, the placement begins at the window's last position
    if m >= 33:
        o = int(rng.integers(590, 640)) if name == "tandem" else int(rng.integers(60, 20 + room))   # no tandem stretch
        for rc in (0, 1):
            add(deleted(t, o, m, m // 2, TIGHT_K), rc, o - 32, 33, "tight")
    q = np.ascontiguousarray(np.stack([np.asarray(r, np.uint8) for r in reads]))
    w = np.asarray(wins, np.int64)
    assert q.shape[1] == m and w.shape == (2 * q.shape[0], 2) and (w >= 0).all()
    return q, w.astype(np.uint32), tags


def assert_not_vacuous(name: str, n: int, per_m: dict) -> None:
    """per_m[m] = (Begins, windows, tags): the kinds the module's text lists, on the model alone, over one text."""
    got = dict.fromkeys(("long indel", "multi", "first", "last", "b = n", "len 0", "tight", "E = max", "E = max + 1",
                         "window past n", "no begin position"), False)
    for m, (b, win, tags) in per_m.items():
        full = place(b, win, m)
        E = (full[:, 1] & EDITS).astype(np.int64)
        hit = full[:, 0] != NONE
        lo, ln = win[:, 0].astype(np.int64), win[:, 1].astype(np.int64)
        last = np.minimum(lo + ln - 1, n)
        for t, tag in enumerate(tags):
            kind = tag.split("/")[0]
            if kind in ("del18", "ins17") and hit[t] and E[t] == int(kind[3:]):
                got["long indel"] = True                    # an indel longer than the band of 15, placed at its cost
            if kind == "tight":
                rec = place(b, win, TIGHT_K)[t]
                assert rec[0] == last[t] and (rec[1] & EDITS) == TIGHT_K and not rec[1] & MULTI, (name, m, t, rec)
                # the placement uses m + TIGHT_K text bases: it ends at the scan end exactly
                assert b.e[t, last[t]] == TIGHT_K and last[t] + m + TIGHT_K <= n
                got["tight"] = True
        got["multi"] |= bool((hit & ((full[:, 1] & MULTI) != 0)).any())
        got["first"] |= bool((hit & (full[:, 0] == lo) & (ln > 1) & ((full[:, 1] & MULTI) == 0)).any())
        got["last"] |= bool((hit & (full[:, 0] == last) & (ln > 1) & (last > lo)).any())
        got["b = n"] |= bool(((ln > 0) & (lo <= n) & (lo + ln - 1 >= n)).any())
        got["window past n"] |= bool(((ln > 0) & (lo <= n) & (lo + ln - 1 > n)).any())
        got["no begin position"] |= bool(((ln > 0) & (lo > n)).any())
        got["len 0"] |= bool((ln == 0).any())
        for me in edit_bounds(m):
            at = place(b, win, me)
            got["E = max"] |= bool(((at[:, 0] != NONE) & ((at[:, 1] & EDITS) == me)).any()) and me not in (0,)
            got["E = max + 1"] |= bool(((at[:, 0] == NONE) & hit & (E == me + 1)).any())
    assert all(got.values()), (name, "not shown", [k for k, v in got.items() if not v])


_cache = {}


def world() -> dict:
    """Per text: World, and per length (reads, tasks, windows, tags, Begins).  Built once per session."""
    if _cache:
        return _cache
    for ti, (name, t) in enumerate(texts().items()):
        w = vr.World(t)
        cases = {}
        for m in LENGTHS:
            q, win, tags = case(name, t, m, 61_000 + 100 * ti + m)
            tasks = sr.tasks_of(q, sr.BOTH)
            cases[m] = (q, tasks, win, tags, Begins(w, tasks))
            q.setflags(write=False)
            win.setflags(write=False)
        assert_not_vacuous(name, w.n, {m: (c[4], c[2], c[3]) for m, c in cases.items()})
        _cache[name] = dict(world=w, text=t, cases=cases)
    return _cache


def short_case(m: int = 100, n: int = 57):
    """n < m: a text shorter than the reads; every e(b) = at least m - (n - b)."""
    t = vr.small_text(1_005)[:n].copy()
    w = vr.World(t)
    q = np.ascontiguousarray(np.stack([vr.small_text(1_005)[o:o + m] for o in (0, 3, 200, 400)]))
    tasks = sr.tasks_of(q, sr.BOTH)
    win = np.asarray([(0, 33), (0, MAX_LEN), (n, 1), (n - 3, 400), (5, 1), (0, 0), (n + 1, 5), (0, 100)], np.uint32)
    b = Begins(w, tasks)
    full = place(b, win, m)
    assert n < m and (full[[0, 1, 2, 3, 4, 7], 0] != NONE).all() and (full[[5, 6], 0] == NONE).all()
    assert (full[:, 1] & EDITS)[0] == m - n                 # read 0 is the text and 43 bases more
    return t, w, q, tasks, win, b


def batch_case(x: dict, m: int = 100, count: int = 513):
    """count reads of m bases, windows by turns 400 long, empty, and 1 .. 33 long: long scans next to idle lanes."""
    q0, _, win0, _, _ = x["cases"][m]
    pick = np.arange(count) % q0.shape[0]
    q = np.ascontiguousarray(q0[pick])
    tasks = sr.tasks_of(q, sr.BOTH)
    n = x["world"].n
    t = np.arange(2 * count)
    lo = (37 * t) % (n - 50)
    ln = np.where(t % 3 == 0, 400, np.where(t % 3 == 1, 0, 1 + t % 33))
    win = np.stack([lo, ln], axis=1).astype(np.uint32)
    return q, tasks, win, Begins(x["world"], tasks)


# ---- the pair choice: a hand-made table ------------------------------------------------------------------------------

def pair_table(m: int = 100, min_frag: int = 200, max_frag: int = 400):
    """(hits, rescued) [4P, 2] and, per pair, the name of what it shows; asserted on pair_keys alone."""
    N = (NONE, 0)
    rows = [
        # name, own hits of tasks 0..3, rescued records of tasks 0..3
        ("orientation 0", [(100, 1 | MULTI), N, N, (300, 2)], [N, N, N, N]),
        ("orientation 1", [N, (300, 0 | MULTI), (100, 3), N], [N, N, N, N]),
        ("rescued beats a worse own hit", [(100, 0), N, N, (250, 9)], [N, N, N, (320, 1)]),
        ("none: too far", [(100, 0), N, N, (500, 0)], [N, N, N, N]),
        ("none: wrong order", [(400, 0), N, N, (100, 0)], [N, N, N, N]),
        ("none: same strand", [(100, 2), N, (300, 1), N], [N, N, N, N]),
        ("none: two rescued records", [N, (700, 5), N, N], [(100, 0), N, N, (300, 0)]),
        ("none: no hit at all", [N, N, N, N], [N, N, (3, 0), N]),
        ("none: strand tie alone", [(100, 4), (900, 4), N, (900, 1 | 77 << 20)], [N, N, N, N]),
        ("key 2: sources", [(100, 2), N, N, (300, 2)], [N, N, N, (310, 2 | MULTI)]),
        ("key 3: orientation", [(100, 1), (320, 2), (110, 1), (300, 2)], [N, N, N, N]),
        ("key 4: B_f", [(100, 3), N, N, (310, 3)], [(90, 1), N, N, (300, 1)]),
        ("key 5: B_r", [(100, 3), N, N, (310, 3)], [(100, 1), N, N, (300, 1)]),
        ("key 5: B_r against s_f", [(100, 3), N, N, (300, 3)], [(100, 1), N, N, (310, 1)]),
        ("key 6: s_f", [(100, 3), N, N, (300, 3 | MULTI)], [(100, 1), N, N, (300, 1)]),
        ("fragment at min_frag", [(100, 0), N, N, (200, 0)], [N, N, N, N]),
        ("fragment at max_frag", [(100, 0), N, N, (400, 0)], [N, N, N, N]),
        ("fragment below min_frag", [(100, 0), N, N, (199, 0)], [N, N, N, N]),
        ("fragment above max_frag", [(100, 0), N, N, (401, 0)], [N, N, N, N]),
    ]
    hits = np.asarray([r for _, h, _ in rows for r in h], np.uint32)
    resc = np.asarray([r for _, _, s in rows for r in s], np.uint32)
    names = [r[0] for r in rows]
    want = pair_hits(hits, resc, m, min_frag, max_frag).reshape(-1, 4, 2)
    for p, name in enumerate(names):
        keys = pair_keys(hits.reshape(-1, 4, 2)[p], resc.reshape(-1, 4, 2)[p], m, min_frag, max_frag)
        proper = (want[p, :, 1] & PROPER) != 0
        if name.startswith(("none", "fragment below", "fragment above")):
            assert not keys and not proper.any(), name
        elif name.startswith("key"):
            i = int(name[4]) - 1                            # the first key at which the two best differ
            assert len(keys) >= 2 and keys[0][0][:i] == keys[1][0][:i] and keys[0][0][i] < keys[1][0][i], (name, keys)
        else:
            assert keys and proper.sum() == 2, name
    assert (want[0, [0, 3], 0] != NONE).all() and (want[1, [2, 1], 0] != NONE).all()      # orientations 0 and 1
    assert want[2, 3, 0] == 320 and want[2, 3, 1] & RESCUED                               # the rescued side won
    assert want[8, 0, 0] == 100 and want[8, 1, 0] == NONE and want[8, 3, 1] == 1          # (E, strand); bits 20+ cleared
    assert want[0, 0, 1] & MULTI and want[1, 1, 1] & MULTI                                # the source's MULTI bit on either side
    assert (want[:, :, 1] >> 20 == 0).all()
    return hits, resc, names, want.reshape(-1, 2)


# ---- simulated pairs -------------------------------------------------------------------------------------------------

PAIR_M, PAIR_MIN, PAIR_MAX, PAIR_BAND, PAIR_EDITS = 100, 200, 400, 3, 12


def pair_reads(t: np.ndarray, seed: int):
    """(reads [2P, 100] interleaved, kinds, truth [P, 2] = where reads 2p and 2p + 1
    begin on the forward text, -1 for the discordant pairs): fragments of 200, 300 and 400 bases in
    both orientations with clean mates, a mate with one deleted / inserted base,
    a mate with a 10-base indel (the band of 3 cannot place it: the rescue
    must), and discordant pairs: too far apart, the wrong order, the same strand."""
    n, m = t.size, PAIR_M
    rng = np.random.default_rng(seed)
    reads, kinds, truth = [], [], []
    for frag in (PAIR_MIN, 300, PAIR_MAX):
        for orient in (0, 1):
            for kind in ("clean", "del1", "ins1", "del10", "ins10", "del10-first"):
                o = int(rng.integers(30, n - frag - 60))
                first, second = t[o:o + m], t[o + frag - m:o + frag]
                if kind in ("del1", "del10"):
                    second = deleted(t, o + frag - m, m, m // 2, int(kind[3:]))
                elif kind in ("ins1", "ins10"):
                    second = inserted(t, o + frag - m, m, m // 2, int(kind[3:]), rng)
                elif kind == "del10-first":
                    first = deleted(t, o, m, m // 2, 10)
                mates = [first, revcomp_def(second[None, :])[0]]
                reads += mates[::-1] if orient else mates
                kinds.append("%s/%d/%d" % (kind, frag, orient))
                truth.append((o + frag - m, o) if orient else (o, o + frag - m))
    for kind in ("far", "order", "same"):
        for _ in range(2):
            o = int(rng.integers(30, n - 700))
            if kind == "far":
                a, b = t[o:o + m], revcomp_def(t[o + 500:o + 600][None, :])[0]
            elif kind == "order":
                a, b = t[o + 200:o + 300], revcomp_def(t[o:o + m][None, :])[0]   # the forward mate right of the reverse one
            else:
                a, b = t[o:o + m], t[o + 200:o + 300]
            reads += [a, b]
            kinds.append(kind)
            truth.append((-1, -1))
    return np.ascontiguousarray(np.stack(reads)), kinds, np.asarray(truth, np.int64)
