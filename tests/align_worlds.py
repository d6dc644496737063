"""Align seeds on low-complexity texts: texts, reads and handles shared by
test_align_worlds_host.py and test_align_worlds_gpu.py.  No model lives here:
align_ref.Rows / Aligned / records stay the reference, verify_ref.candidates
lists the candidates.

Texts (n % 16 covers 0, 1 and 15):
  allA    319 bases, all A;
  cg      400 bases, CG repeated: its own reverse complement, both strands place;
  p3      321 bases, ACT repeated;
  two     511 random bases over A and T;
  runs    about 1,000 bases in runs of 5-9 equal bases with random letters, 45
          runs of them written twice (two distant placements);
  tandem  1,089 random bases with three tandem-repeat stretches (units A, CA
          and GATTC, 50, 48 and 55 bases) and one copied segment of 300 bases.

Lengths 17, 100, 129, 256.  Per (text, length) two kinds of handles, at most
160 tasks together:

  direct  at most 128 forward tasks whose slots are filled here: a slot is the
          single row [ISA[o + start], ISA[o + start] + 1) with span (start, len),
          so the test chooses each candidate's origin o.
          * Per band w = 1 .. 15: the exact window at o + w and the one at
            o - w scored at o (every third w with o at a text end, so that band
            cells fall off the text).
          * Per k = 1 .. 16 with 3 k <= m: k bases deleted near m // 2 and k
            foreign bases inserted near m // 2 (indel_site picks the place).
          * Per w with 3 (w + 1) <= m: w + 1 bases deleted at m // 3 and w + 1
            inserted at 2 m // 3 (the path leaves the band of w), and the
            mirror image, inserted first and deleted after, which leaves on the
            side of the bits above 2w.
          * Per w with w + 8 <= m: w foreign bases in front of the window, a
            path along the band's lower edge.
          * Three tasks use all eight slots: neighbouring origins at the text's
            start, at its end, and around a window whose first base is changed,
            where two begin positions tie; that read once more with its own
            origin alone.  One eight-slot task holds a read of foreign letters
            at origins all over the text: every cell of every candidate ties.
          * Every eighth task has no slot at all, and the eight-slot tasks are
            spread so that every wave of 64 tasks holds some of each kind.
  real    16 reads (32 tasks under BOTH) drawn from the text -- exact, one base
          changed, deleted or inserted, half of them reverse complements -- with
          seed_ref.reference's records at S = 8 on the brute-force suffix
          array: intervals hundreds of rows wide that max_occ = 1, 8, 256 cuts.

ends_world(): the 16 first and 16 last origins x the 8 pinned read positions x
{one base deleted, one inserted} at m = 100 on `two`, 512 single-slot tasks.
batch_world(): 513 tasks of `cg` at m = 100, by turns a slot 300 rows wide (256
candidates at max_occ 256), no slot, one row.

Non-vacuity (assert_not_vacuous, on the model alone, for every band w >= 1):
  (a) a record with more than one cell of a single candidate attaining E;
  (b) a scored candidate whose only minimum is at d = +w, and one at d = -w;
  (c) a record with E = w that at band w - 1 is NONE or has E > w;
  (d) a record with MULTI, and one with B_max > B_min without MULTI;
  (e) a candidate with invalid cells at the text's start and one at the text's
      end, with E <= 1.
What cannot hold, and why.  On a text of period P (allA: 1, cg: 2, p3: 3) a
path shifted by P sees the same text, so the cell d - P of a candidate costs no
more than the cell d wherever it is valid and the shifted path stays in the
band, and a net shift of s bases costs what the shift s modulo P does.  Hence:
  * (b) as stated can hold on cg for no w and on p3 for w = 1 only.  These
    texts are asked for "the edge cell attains the candidate's minimum, and
    every cell that does lies a multiple of P from it": B_max (B_min) of such a
    record comes from the edge cell alone.
  * (c) can hold on them only while w <= max(1, P // 2): a wider band places no
    read more cheaply there.  It is asked for those w.
  * allA is excused from (b) and (c) by name: every cell of every row sees the
    same text.
  * An indel of w bases is the cheapest path only while the bases on both sides
    outweigh it; (c) is asked for 3 w <= m, which at m = 17 is w <= 5.

The whole module's model (six texts, four lengths, sixteen bands, K = 2 and for
two texts K = 1, the ends and the batch) takes about 15 s on eight CPU threads."""
import os
from bisect import bisect_left, bisect_right
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import align_ref as ar
import seed_ref as sr
import verify_ref as vr
from skip_texts import ACGT
from strand_reads import revcomp_def

LENGTHS = (17, 100, 129, 256)
BANDS = tuple(range(16))
OCCS = (1, 8, 256)
PERIOD = {"allA": 1, "cg": 2, "p3": 3}
K1_TEXTS = ("cg", "tandem")              # the texts whose real seeds exist at K = 1 as well
A, C, G, T = (int(b) for b in ACGT)


COPY = {"tandem": (60, 300)}             # (where a segment that occurs twice begins, its length); runs: set by texts()


def _runs_text(rng) -> np.ndarray:
    """Runs of 5-9 equal bases, neighbours differ; runs 10 .. 54 are written a second time after run 59."""
    def run(no):
        return (int(rng.choice([b for b in (A, C, G, T) if b not in no])), int(rng.integers(5, 10)))
    first = []
    for i in range(60):
        no = {first[-1][0]} if first else set()
        if i == 59:
            no.add(first[10][0])
        first.append(run(no))
    out = first + first[10:55]
    while sum(ln for _, ln in out) < 1_000:
        out.append(run({out[-1][0]}))
    COPY["runs"] = (sum(ln for _, ln in first[:10]), sum(ln for _, ln in first[10:55]))
    assert COPY["runs"][1] >= 256 + 24
    return np.concatenate([np.full(ln, b, np.uint8) for b, ln in out])


def texts() -> dict:
    rng = np.random.default_rng(21_000)
    t = ACGT[rng.integers(0, 4, size=1_089)].copy()
    t[400:450] = A
    t[460:508] = np.tile(np.asarray([C, A], np.uint8), 24)
    t[520:575] = np.tile(np.frombuffer(b"GATTC", np.uint8), 11)
    t[700:1_000] = t[60:360]
    out = {
        "allA": np.full(319, A, np.uint8),
        "cg": np.tile(np.asarray([C, G], np.uint8), 200),
        "p3": np.tile(np.asarray([A, C, T], np.uint8), 107),
        "two": np.asarray([A, T], np.uint8)[rng.integers(0, 2, size=511)],
        "runs": _runs_text(rng),
        "tandem": t,
    }
    assert {v.size % 16 for v in out.values()} >= {0, 1, 15} and all(300 <= v.size <= 1_100 for v in out.values())
    assert np.array_equal(revcomp_def(out["cg"][None, :])[0], out["cg"])
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def brute_search(w: vr.World):
    """The `search` of seed_ref.reference on the brute-force suffix array: the
    rows whose suffix begins with the pattern.  (The CPU oracle restates the
    reference's walk, which is undefined where a step reads past the index;
    these texts have such steps.)"""
    tb, sa = w.text.tobytes() + b"$", [int(x) for x in w.sa]

    def search(q):
        out = np.zeros((q.shape[0], 2), np.uint32)
        for i, row in enumerate(q):
            p = row.tobytes()
            key = lambda s: tb[s:s + len(p)]   # noqa: E731
            out[i] = (bisect_left(sa, p, key=key), bisect_right(sa, p, key=key))
        return out.reshape(-1)
    return search


def foreign(t: np.ndarray, at: int, k: int, rng) -> np.ndarray:
    """k bases to insert before t[at]: a letter the text does not hold where there
    is one, else bases that differ from both neighbours and from each other in turn."""
    absent = [b for b in (G, C, T, A) if b not in t]
    if absent:
        return np.full(k, absent[0], np.uint8)
    new = [ar.other_base(t, at, rng)]
    while len(new) < k:
        new.append(int(rng.choice([b for b in (A, C, G, T) if b not in (new[-1], int(t[at]))])))
    return np.asarray(new, np.uint8)


def inserted(t, a, m, p, k, rng):
    return np.concatenate([t[a:a + p], foreign(t, a + p, k, rng), t[a + p:a + m - k]])


def anchors(name: str, n: int, m: int) -> list:
    """Origins away from both ends: 16 <= a <= n - m - 42; on `tandem` and `runs` next to the repeats."""
    lo, hi = 16, n - m - 42
    want = {"tandem": (392, 452, 512, 150), "runs": (80, 300)}.get(name, ())
    out = [a for a in want if lo <= a <= hi]
    return out or [lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3]


def plain_anchors(name: str, n: int, m: int) -> list:
    """On `tandem`, origins in the random stretches: a deletion of k bases costs k there, not k modulo a unit."""
    return [a for a in (150, 620) if name == "tandem" and a <= n - m - 42] or anchors(name, n, m)


def indel_site(t: np.ndarray, anc: list, m: int, k: int):
    """(a, p) for an indel of k bases at read position p of the window at a: near
    an anchor and near m // 2, where the bases before and the bases after the
    indel both change letter most often -- a stretch of one letter shifts for
    free, and then a narrower band places the read at the same cost."""
    changes = lambda x: int(np.count_nonzero(x[1:] != x[:-1]))   # noqa: E731
    best = None
    for a0 in anc:
        for a in range(a0, a0 + 10):
            for p in (m // 2, m // 2 - 1, m // 2 + 1, m // 2 - 2, m // 2 + 2):
                v = min(changes(t[a:a + p]), changes(t[a + p:a + m - k]), changes(t[a + p + k:a + m + k]))
                if best is None or v > best[0]:
                    best = (v, a, p)
    return best[1], best[2]


def direct(name: str, w: vr.World, m: int, seed: int):
    """(q, iv, sp) at S = 8, forward tasks: the module's text says which."""
    t, n = w.text, w.n
    rng = np.random.default_rng(seed)
    isa = np.empty(n + 1, np.int64)
    isa[w.sa] = np.arange(n + 1)
    anc, plain = anchors(name, n, m), plain_anchors(name, n, m)
    last = n - m
    tasks = []                                           # (read, [origins])
    for b in range(1, 16):
        at_end = b % 3 == 0
        o = b // 2 if at_end else anc[b % len(anc)]
        tasks.append((t[o + b:o + b + m], [o]))          # the only zero at d = +b
        o = last - b // 2 if at_end else anc[(b + 1) % len(anc)]
        tasks.append((t[o - b:o - b + m], [o]))          # ... at d = -b
    for k in range(1, 17):
        if 3 * k <= m:
            a, p = indel_site(t, plain[k % len(plain):] + plain[:k % len(plain)], m, k)
            tasks.append((ar.deleted(t, a, m, p, k), [a]))
            a, p = indel_site(t, anc[k % len(anc):] + anc[:k % len(anc)], m, k)
            tasks.append((inserted(t, a, m, p, k, rng), [a]))
    for b in range(1, 16):
        k = b + 1
        if 3 * k <= m:
            a, p1, p2 = anc[b % len(anc)], m // 3, 2 * m // 3
            tasks.append((np.concatenate([t[a:a + p1], t[a + p1 + k:a + p2 + k], foreign(t, a + p2 + k, k, rng),
                                          t[a + p2 + k:a + m]]), [a]))
            # the mirror image: inserted first, deleted after -- the path leaves on the side of the bits above 2w
            tasks.append((np.concatenate([t[a:a + p1], foreign(t, a + p1, k, rng), t[a + p1:a + p2 - k], t[a + p2:a + m]]), [a]))
    for b in range(1, 16):
        if b + 8 <= m:                                   # b foreign bases, then the window: the path keeps to d = -b
            a = anc[b % len(anc)]
            front = foreign(t, a, b, rng)
            if len(set(t.tolist())) == 4:                # no absent letter: a place whose neighbourhood lacks one
                for a2 in range(a, min(a + 40, last - 42)):
                    lacks = [x for x in (A, C, G, T) if x not in t[a2 - b:a2 + 1]]
                    if lacks:
                        a, front = a2, np.full(b, lacks[0], np.uint8)
                        break
            tasks.append((np.concatenate([front, t[a:a + m - b]]), [a]))
    tasks.append((t[1:1 + m], [0, 1, 2, 3, 4, 5, 8, 16]))
    tasks.append((t[last - 1:last - 1 + m], [last - d for d in (0, 1, 2, 3, 4, 5, 8, 16)]))
    a = anc[0]
    changed = t[a:a + m].copy()
    changed[0] = foreign(t, a, 1, rng)[0]
    tasks.append((changed, [a + d for d in (0, 1, -1, 2, -2, 5, -7, 16)]))
    tasks.append((changed, [a]))                         # the same read alone: B = a and a + 1 tie, no MULTI
    absent = [b for b in (G, C, T, A) if b not in t]
    noise = np.full(m, absent[0], np.uint8) if absent else ACGT[rng.integers(0, 4, size=m)]
    tasks.append((noise, [int(x) for x in np.linspace(0, last, 8).astype(np.int64)]))
    eight = [x for x in tasks if len(x[1]) == 8]         # two of them in every wave of 64 tasks
    tasks = [x for x in tasks if len(x[1]) != 8]
    for i, x in enumerate(eight):
        tasks.insert(3 + 28 * i, x)
    q, iv, sp = [], [], []
    for read, origins in tasks:
        if len(q) % 8 == 3:                              # a task without a slot in every group of eight
            q.append(t[anc[0]:anc[0] + m])
            iv.append(np.zeros((8, 2), np.uint32))
            sp.append(np.zeros((8, 2), np.uint32))
        assert read.size == m and all(0 <= o <= last for o in origins)
        i, s = np.zeros((8, 2), np.uint32), np.zeros((8, 2), np.uint32)
        for j, o in enumerate(origins):
            start = (7 * len(q) + 3 * j) % m
            i[j] = (isa[o + start], isa[o + start] + 1)
            s[j] = (start, max(1, (m - start) // 2))
        q.append(read)
        iv.append(i)
        sp.append(s)
    assert len(q) <= 128
    return np.ascontiguousarray(np.stack(q)), np.stack(iv), np.stack(sp)


def real_reads(name: str, t: np.ndarray, m: int, seed: int) -> np.ndarray:
    """16 reads: windows of the text (origins 0 and n - m among them, and on
    `runs` and `tandem` the copied segment), by turns exact, one base changed,
    one deleted, one inserted; odd rows reverse complements."""
    n = t.size
    rng = np.random.default_rng(seed)
    o = [int(x) for x in rng.integers(0, n - m + 1, size=16)]
    o[0], o[1] = 0, n - m
    if name in COPY:
        inside = COPY[name][0]
        o[4], o[5], o[8] = inside + 2, inside + 9, inside + 20
    if name == "tandem" and m <= 129:
        o[6], o[7], o[9], o[10] = 395, 440, 500, 530
    out = []
    for i, a in enumerate(o):
        a = min(a, n - m - 1) if i % 4 == 2 else a
        r = t[a:a + m].copy()
        p = int(rng.integers(1, m - 1))
        if i % 4 == 1:
            r[p] = foreign(t, a + p, 1, rng)[0]
        elif i % 4 == 2:
            r = ar.deleted(t, a, m, p)
        elif i % 4 == 3:
            r = inserted(t, a, m, p, 1, rng)
        out.append(r)
    q = np.stack(out)
    q[1::2] = revcomp_def(q[1::2])
    return np.ascontiguousarray(q)


def assert_not_vacuous(name: str, n: int, m: int, als) -> None:
    """als: the Aligned of the direct and of the real tasks of one (text,
    length), every band filled; S = 8, max_occ = 256."""
    P = PERIOD.get(name)
    for w in range(1, 16):
        got = dict.fromkeys(("a", "b+", "b-", "c", "multi", "spread", "start", "end"), False)
        for a in als:
            rec, prev = ar.records(a, 8, 256, w, m), ar.records(a, 8, 256, w - 1, m)
            E, Ep = ar.edits_of(rec), ar.edits_of(prev)
            R, t, o = a.cand_rows(w), a.c.task[a.sc], a.c.origin[a.sc]
            mn = R.min(axis=1)
            at = R == mn[:, None]
            got["a"] |= bool(((R == E[t][:, None]).sum(axis=1) > 1).any())
            if P is None:
                only = at.sum(axis=1) == 1
                got["b+"] |= bool((only & at[:, 2 * w]).any())
                got["b-"] |= bool((only & at[:, 0]).any())
            else:
                k = np.arange(2 * w + 1)
                got["b+"] |= bool((at[:, 2 * w] & (~at | ((2 * w - k) % P == 0)[None, :]).all(axis=1) & (mn < ar.INF)).any())
                got["b-"] |= bool((at[:, 0] & (~at | (k % P == 0)[None, :]).all(axis=1) & (mn < ar.INF)).any())
            scored = rec[:, 1] >> ar.SCORED_SHIFT > 0
            got["c"] |= bool((scored & (E == w) & ((Ep < 0) | (Ep > w))).any())
            _, bmin, bmax, _ = a.best(8, 256, w)
            hit = rec[:, 0] != ar.NONE
            got["multi"] |= bool((hit & ((rec[:, 1] & ar.MULTI) != 0)).any())
            got["spread"] |= bool((hit & (bmax > bmin) & ((rec[:, 1] & ar.MULTI) == 0)).any())
            got["start"] |= bool(((o < w) & (R[:, 0] >= ar.INF) & (mn <= 1)).any())
            got["end"] |= bool(((o + m + w > n) & (mn <= 1)).any())      # cells (i, d) with o + i + d > n, in later rows
        if name == "allA":
            got["b+"] = got["b-"] = got["c"] = True      # excused: every cell of every row sees the same text
        if (P is not None and w > max(1, P // 2)) or 3 * w > m:
            got["c"] = True                              # a shift of P is free; no single indel of w is cheapest
        assert all(got.values()), (name, m, "band", w, "not shown", [k for k, v in got.items() if not v])


_cache = {}


def _fill(jobs) -> None:
    jobs.sort(key=lambda j: -j[0])
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        list(pool.map(lambda j: j[1].fill(j[2]), jobs))


def world(K) -> dict:
    """Per text: the World, the K = 1, 2 indexes and, per length,
    direct = (q, iv, sp, Aligned) of the forward tasks and real = (q, both, {K:
    (iv, sp, Aligned)}) at S = 8, max_occ = 256; every band.  The conditions
    are asserted here, on the model alone.  Built once per session."""
    if _cache:
        return _cache
    out, jobs = {}, []
    for ti, (name, t) in enumerate(texts().items()):
        w = vr.World(t)
        idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2)}
        search = brute_search(w)
        cases = {}
        for m in LENGTHS:
            q, iv, sp = direct(name, w, m, 31_000 + 100 * ti + m)
            dc = vr.candidates(w, q, iv, sp, 256)
            rows = ar.Rows(w, q, [dc], bands=BANDS, fill=False)
            dal = ar.Aligned(w, q, dc, rows=rows)
            jobs += [(m * (2 * b + 1) * rows.keys.size, rows, b) for b in BANDS]
            rq = real_reads(name, t, m, 41_000 + 100 * ti + m)
            both = sr.tasks_of(rq, sr.BOTH)
            seeds = {}
            for k in (1, 2) if name in K1_TEXTS else (2,):
                riv, rsp, _ = sr.reference(search, both, k, 8)
                seeds[k] = (riv, rsp, vr.candidates(w, both, riv, rsp, 256))
            rrows = ar.Rows(w, both, [s[2] for s in seeds.values()], bands=BANDS, fill=False)
            jobs += [(m * (2 * b + 1) * rrows.keys.size, rrows, b) for b in BANDS]
            per_k = {k: (riv, rsp, ar.Aligned(w, both, c, rows=rrows)) for k, (riv, rsp, c) in seeds.items()}
            for x in (q, iv, sp, rq) + tuple(y for s in seeds.values() for y in s[:2]):
                x.setflags(write=False)
            cases[m] = dict(direct=(q, iv, sp, dal), real=(rq, both, per_k))
        out[name] = dict(world=w, text=t, idx=idx, cases=cases, search=search)
    _fill(jobs)
    for name, x in out.items():
        for m, c in x["cases"].items():
            assert_not_vacuous(name, x["world"].n, m, [c["direct"][3], c["real"][2][2][2]])
    _cache.update(out)
    return _cache


_ends = {}


def ends_world(w: vr.World, m: int = 100):
    """(q, iv, sp, Aligned): every one of the 16 first and 16 last origins x
    every pinned read position x {one base deleted, one inserted}, one
    single-row slot each, every band."""
    if not _ends:
        t, n = w.text, w.n
        rng = np.random.default_rng(51_000)
        isa = np.empty(n + 1, np.int64)
        isa[w.sa] = np.arange(n + 1)
        q, iv, sp = [], [], []
        for o in list(range(16)) + list(range(n - m - 15, n - m + 1)):
            for p in ar.pinned(m):
                for r in (ar.deleted(t, o, m, p), inserted(t, o, m, p, 1, rng)):
                    start = (5 * len(q)) % m
                    q.append(r)
                    iv.append([[isa[o + start], isa[o + start] + 1]] + [[0, 0]] * 7)
                    sp.append([[start, 1 + (m - 1 - start) // 3]] + [[0, 0]] * 7)
        q, iv, sp = np.ascontiguousarray(np.stack(q)), np.asarray(iv, np.uint32), np.asarray(sp, np.uint32)
        assert q.shape == (32 * 8 * 2, m)
        a = ar.Aligned(w, q, vr.candidates(w, q, iv, sp, 256), bands=BANDS)
        e1 = ar.edits_of(ar.records(a, 8, 256, 1, m))
        assert ((e1 >= 0) & (e1 <= 1)).all()             # every read is placed with its one indel
        _ends["x"] = (q, iv, sp, a)
    return _ends["x"]


_batch = {}
BATCH_BAND = 7


def batch_world(w: vr.World, q_from: np.ndarray, m: int = 100):
    """(q, iv, sp, Aligned at band 7): 513 tasks, reads taken by turns from
    q_from; task i has a slot of 300 rows (256 candidates at max_occ 256) when
    i % 3 == 0, no slot when i % 3 == 1, else one row."""
    if not _batch:
        rows = w.n + 1
        q = np.ascontiguousarray(q_from[np.arange(513) % q_from.shape[0]])
        iv, sp = np.zeros((513, 8, 2), np.uint32), np.zeros((513, 8, 2), np.uint32)
        for i in range(513):
            if i % 3 == 0:
                L = (37 * i) % (rows - 300)
                iv[i, i % 8], sp[i, i % 8] = (L, L + 300), (i % 5, 3)
            elif i % 3 == 2:
                L = (11 * i) % rows
                iv[i, 0], sp[i, 0] = (L, L + 1), (0, m)
        a = ar.Aligned(w, q, vr.candidates(w, q, iv, sp, 256), bands=(BATCH_BAND,))
        scored = ar.records(a, 8, 256, BATCH_BAND, m)[:, 1] >> ar.SCORED_SHIFT
        assert (scored[0::3] > 100).all() and (scored[1::3] == 0).all()
        assert scored[255] > 100 and scored[256] == 0    # a batch of 257 ends on a lane without candidates
        _batch["x"] = (q, iv, sp, a)
    return _batch["x"]
