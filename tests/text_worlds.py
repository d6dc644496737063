"""Random worlds for the text kernels (verify, align, paths, windows, pairs):
the generator and the chain of models shared by test_text_worlds_host.py and
test_text_worlds_gpu.py.  Nothing here calls the library or needs a device:
the models are verify_ref.candidates / records, align_ref.Aligned / records,
path_ref.Walk / records, window_ref.Begins / place / mate_windows / pair_hits
and seed_ref.reference over align_worlds.brute_search.

world(i), i in range(WORLDS), is deterministic from default_rng(BASE + i):

  n       even worlds take the fixed lengths N_FIXED in turn (all of them, the
          twelve shortest twice); odd worlds take a free draw in 4 .. 2,000 whose
          residue n % 16 goes round with the world, so that every residue occurs
          three times whatever BASE is.
  text    test_random_worlds._text: random, runs, tandem, two letters.
  K, d    K in {1, 2} (K = 1 where n < 2K + 1), d in {32, 64, 128, 192, 448, 960}.
  m       by i % 3: an edge length <= min(n, 256) of verify_ref.LENGTHS; one of
          n - 1, n, n + 1 clipped to 1 .. 256; any of 1 .. 256 (m > n occurs).
  reads   N in {1, 5, 24, 63, 64, 65, 130}.  Where n >= m the kinds go round:
          exact windows, one and three substitutions, a one-base and a k-base
          (k <= 17, 3k <= m) deletion and insertion, a read hanging off the
          text's start and one off its end, foreign reads, a window inside the
          band's reach of either text end.  Where n < m: the text followed or
          preceded by foreign bases.  Odd rows are reverse complements; a few
          rows carry N or lowercase bytes.  On pair worlds (N even, strands
          BOTH) every other odd read is the mate of the read before it -- a
          window one fragment length downstream, exact or with k bases deleted.
  call    S, max_occ, band, strands, max_mism, max_edits, C, path chunk, split
          class and backend are all drawn per world; one caller-filled window
          per task; min_frag, max_frag on pair worlds.

The model chain runs on the tasks of the world's strand mode: seeds at S = 8,
candidates at max_occ 256, the verify and align records at the world's cuts,
walks from the align records' B, from caller-filled B (path_ref.hand_hits: B >
n comes from nowhere else) and from the placed records' B, Begins, place on the
caller's windows and, on pair worlds, mate_windows in modes 0 and 1, place in
those windows, pair_hits and the walk of the paired records.  Every fourth
world carries a host-only variant: a suffix array with rows that have no
suffix and one hand-made slot over the whole array (NO_SUFFIX cannot occur on
a device, whose suffix array is the index's own).

assert_not_vacuous(all worlds) states what the worlds must show, on the model
alone.  The whole module's model -- 96 worlds, up to 260 tasks each -- takes
under 10 s on one CPU thread (measured: 4.4 and 8.7 s on two hosts), and the
conditions 0.1 s more."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import align_ref as ar
import align_worlds as aw
import path_ref as pr
import seed_ref as sr
import verify_ref as vr
import window_ref as wr
from strand_reads import code_of, revcomp_def
from test_random_worlds import _text

WORLDS = 96
BASE = 250_000
N_FIXED = (1, 2, 3, 4, 5, 7, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 100, 127, 128, 129, 255,
           256, 257, 258, 271, 300, 511, 1000, 2047)
DS = (32, 64, 128, 192, 448, 960)
NS = (1, 5, 24, 63, 64, 65, 130)
SEEDS, OCCS, ENTRIES, CHUNKS, CLASSES = (1, 4, 8), (1, 2, 8, 256), (1, 2, 8, 32), (0, 64), (0, 1, 4)
STRANDS = (sr.FWD, sr.REV, sr.BOTH)
WINDOW_LENS = (0, 1, 33, 400, wr.MAX_LEN)
FRAG_SPANS = (0, 200, wr.MAX_LEN - 1)
KINDS = ("exact", "subs1", "subs3", "del1", "delk", "ins1", "insk", "off-start", "off-end", "foreign", "near-start",
         "near-end")
ACGT = wr.ACGT


def brute_search(w: vr.World):
    """align_worlds.brute_search on the bases the reads' bytes stand for.  It compares raw bytes, and these reads
    carry N and lowercase bytes; kstep_fmi.h ("both strands", which the seed search's tasks follow): "The definition
    is on codes: N and every other byte go the way base2index sends them (N -> G, lowercase like uppercase)"."""
    search = aw.brute_search(w)
    return lambda q: search(ACGT[code_of(q)])


def _bound(rng, m: int) -> int:
    return int(rng.choice([0, 1, int(rng.integers(0, m + 1)), m]))


def _read(kind: str, t: np.ndarray, m: int, band: int, rng) -> np.ndarray:
    """One read of m <= n bases of the kind; a kind the sizes leave no room for falls back to the exact window."""
    n = t.size
    o = int(rng.integers(0, n - m + 1))
    k = int(rng.integers(2, 18))
    k = k if 3 * k <= m else 1
    if kind == "subs1":
        return wr.changed(t, o, m, 1, rng)
    if kind == "subs3":
        return wr.changed(t, o, m, min(3, m), rng)
    if kind in ("del1", "delk"):
        k = 1 if kind == "del1" else k
        o = min(o, max(n - m - k, 0))
        return wr.deleted(t, o, m, m // 2, k) if o + m + k <= n else t[o:o + m]
    if kind in ("ins1", "insk"):
        k = 1 if kind == "ins1" else k
        return wr.inserted(t, o, m, m // 2, k, rng) if m - m // 2 >= k else t[o:o + m]
    if kind in ("off-start", "off-end"):
        h = min(int(rng.integers(1, 4)), m - 1)
        if kind == "off-start":
            return np.concatenate([wr.foreign(t, 0, h, rng), t[:m - h]])
        return np.concatenate([t[n - (m - h):], wr.foreign(t, n - 1, h, rng)])
    if kind == "foreign":
        return ACGT[rng.integers(0, 4, size=m)]
    if kind == "near-start":
        o = min(int(rng.integers(0, band + 1)), n - m)
    if kind == "near-end":
        o = max(n - m - int(rng.integers(0, band + 1)), 0)
    return t[o:o + m]


def _reads(rng, t: np.ndarray, m: int, N: int, band: int, pair: bool, min_frag: int, max_frag: int) -> np.ndarray:
    n = t.size
    rows = []
    first = int(rng.integers(0, len(KINDS)))
    for r in range(N):
        if n < m:
            extra = ACGT[rng.integers(0, 4, size=m - n)]
            rows.append(np.concatenate([t, extra] if r % 4 < 2 else [extra, t]))
            continue
        if pair and r % 4 == 1 and n >= min_frag:
            # the mate of read r - 1, where that is a window: drawn again here as one, a fragment length downstream
            frag = int(rng.integers(min_frag, min(max_frag, n) + 1))
            o = int(rng.integers(0, n - frag + 1))
            rows[-1] = t[o:o + m]
            a, k = o + frag - m, int(rng.integers(2, 18))
            rows.append(wr.deleted(t, a, m, m // 2, k) if r % 8 == 5 and 3 * k <= m and a + m + k <= n else t[a:a + m])
            continue
        rows.append(_read(KINDS[(first + r) % len(KINDS)], t, m, band, rng))
    q = np.stack([np.asarray(r, np.uint8) for r in rows])
    assert q.shape == (N, m)
    for r in range(2, N, 7):                                  # other bytes on top of a few rows
        if r % 3 == 0:
            q[r, int(rng.integers(0, m))] = ord("N")
        elif r % 3 == 1:
            q[r] = np.char.lower(q[r:r + 1].view("S1")).view(np.uint8)
        else:
            q[r, int(rng.integers(0, m))] = ord("n")
    q[1::2] = revcomp_def(q[1::2])
    return np.ascontiguousarray(q)


def _windows(rng, n: int, T: int) -> np.ndarray:
    lo = [int(rng.choice([0, n - 1, n, n + 1, int(rng.integers(0, n + 3))])) for _ in range(T)]
    ln = [int(rng.choice(list(WINDOW_LENS) + [int(rng.integers(1, 601))])) for _ in range(T)]
    return np.asarray(list(zip(lo, ln)), np.uint32).reshape(T, 2)


def _cut(c: vr.Cands, s: int, occ: int) -> vr.Cands:
    """The candidates in slots < s and ranks < occ."""
    keep = (c.slot < s) & (c.rank < occ)
    return vr.Cands(c.T, np.stack([c.task, c.slot, c.rank, c.why, c.origin, c.mism], axis=1)[keep])


@lru_cache(maxsize=None)
def world(i: int) -> SimpleNamespace:
    """World i: its sizes, text, reads and call parameters, then the chain of models on them."""
    rng = np.random.default_rng(BASE + i)
    free = int(rng.integers(4, 2_001))
    if i % 2 == 0:
        n = N_FIXED[(i // 2) % len(N_FIXED)]
    else:
        n = free - free % 16 + (i // 2) % 16
        n += 16 if n < 4 else -16 if n > 2_000 else 0
    text = _text(rng, n)
    K = int(rng.choice([1, 2]))
    if n < 2 * K + 1:
        K = 1
    d = int(rng.choice(DS))
    if i % 3 == 0:
        m = int(rng.choice([x for x in vr.LENGTHS if x <= min(n, 256)]))
    elif i % 3 == 1:
        m = min(max(n + int(rng.integers(-1, 2)), 1), 256)
    else:
        m = int(rng.integers(1, 257))
    N = int(rng.choice(NS))
    x = SimpleNamespace(i=i, n=n, text=text, K=K, d=d, m=m, S=int(rng.choice(SEEDS)), occ=int(rng.choice(OCCS)),
                        band=int(rng.integers(0, 16)), strands=int(rng.choice(STRANDS)), max_mism=_bound(rng, m),
                        max_edits=_bound(rng, m), C=int(rng.choice(ENTRIES)), chunk=int(rng.choice(CHUNKS)),
                        split=int(rng.choice(CLASSES)), backend="task" if i % 8 == 7 else "task-mid")
    x.pair = N % 2 == 0 and x.strands == sr.BOTH
    x.min_frag = m + int(rng.integers(0, 301))
    x.max_frag = x.min_frag + int(rng.choice(FRAG_SPANS))
    x.N, x.q = N, _reads(rng, text, m, N, x.band, x.pair, x.min_frag, x.max_frag)
    band = x.band
    x.w = w = vr.World(x.text)
    x.tasks = sr.tasks_of(x.q, x.strands)
    x.T = T = x.tasks.shape[0]
    iv8, sp8, _ = sr.reference(brute_search(w), x.tasks, x.K, 8)
    x.cands = vr.candidates(w, x.tasks, iv8, sp8, 256)
    x.iv, x.sp = np.ascontiguousarray(iv8[:, :x.S]), np.ascontiguousarray(sp8[:, :x.S])
    x.verify = vr.records(x.cands, x.S, x.occ, x.max_mism)
    x.aligned = ar.Aligned(w, x.tasks, _cut(x.cands, x.S, x.occ), bands=(band,))
    x.align = ar.records(x.aligned, x.S, x.occ, band, x.max_edits)
    # the host-only variant: rows without a suffix and a hand-made slot over the whole array in the last task
    x.holes = None
    if i % 4 == 1:
        sa = w.sa.copy()
        sa[1::3] = 0xFFFFFFFF
        hiv, hsp = x.iv.copy(), x.sp.copy()
        hiv[T - 1, 0], hsp[T - 1, 0] = (0, n + 1), (0, max(1, m // 2))
        hc = vr.candidates(w, x.tasks, hiv, hsp, x.occ, sa=sa)
        ha = ar.Aligned(w, x.tasks, hc, bands=(band,))
        x.holes = SimpleNamespace(sa=sa, iv=hiv, sp=hsp, cands=hc, verify=vr.records(hc, x.S, x.occ, x.max_mism),
                                  align=ar.records(ha, x.S, x.occ, band, x.max_edits))
    # paths: from the align records, from caller-filled begin positions, from the placed records
    x.windows = _windows(rng, n, T)
    x.begins = wr.Begins(w, x.tasks)
    x.placed = wr.place(x.begins, x.windows, x.max_edits)
    x.B_align = x.align[:, 0].astype(np.int64)
    x.B_hand = pr.hand_hits(n, m, band, x.B_align)
    x.B_placed = x.placed[:, 0].astype(np.int64)
    x.walks = {k: pr.Walk(w, x.tasks, B, band) for k, B in (("align", x.B_align), ("hand", x.B_hand), ("placed", x.B_placed))}
    x.modes = {}
    if x.pair:
        for mode in (0, 1):
            win = wr.mate_windows(x.align, n, m, x.min_frag, x.max_frag, mode)
            resc = wr.place(x.begins, win, x.max_edits)
            paired = wr.pair_hits(x.align, resc, m, x.min_frag, x.max_frag)
            x.modes[mode] = SimpleNamespace(win=win, resc=resc, paired=paired)
        x.B_paired = x.modes[0].paired[:, 0].astype(np.int64)
        x.walks["paired"] = pr.Walk(w, x.tasks, x.B_paired, band)
    x.paths = {k: pr.records(p, x.max_edits, x.C) for k, p in x.walks.items()}
    for a in (x.q, x.tasks, x.iv, x.sp, x.windows, x.verify, x.align, x.placed):
        a.setflags(write=False)
    return x


def worlds() -> list:
    return [world(i) for i in range(WORLDS)]


def assert_not_vacuous(ws: list) -> None:
    """What the worlds must show together, on the model alone."""
    got = dict.fromkeys(("n = m", "n = m - 1", "n = m + 1", "low > 0", "o < band", "OFF_START", "OFF_END", "NO_SUFFIX",
                         "MULTI verify", "MULTI align", "MULTI place", "bound verify", "bound align", "bound place",
                         "I run", "D run", "OVERFLOW", "no path: NONE", "no path: n < m", "no path: B > n",
                         "no path: B - c > w", "b = n", "past n", "lo > n", "len 0", "PROPER | RESCUED", "no combination",
                         "N byte", "lowercase"), False)
    short, tiny, small, residues, shifts = [], 0, 0, set(), set()
    for x in ws:
        n, m, band, c = x.n, x.m, x.band, x.cands
        tiny += n < 16
        small += 16 <= n < 64
        got["n = m"] |= n == m
        got["n = m - 1"] |= n == m - 1
        got["n = m + 1"] |= n == m + 1
        got["N byte"] |= bool(np.isin(x.q, np.frombuffer(b"Nn", np.uint8)).any())
        got["lowercase"] |= bool((x.q >= ord("a")).any())
        sel = (c.why == vr.SCORED) & (c.slot < x.S) & (c.rank < x.occ)
        o = c.origin[sel]
        if o.size:
            residues.add(n % 16)
            shifts |= {int(v) for v in np.unique((n - o - m + 16 - band) & 15)}
            got["low > 0"] |= bool((band > n - o - m).any())
            got["o < band"] |= bool((o < band).any())
        cut = (c.slot < x.S) & (c.rank < x.occ)
        got["OFF_START"] |= bool((cut & (c.why == vr.OFF_START)).any())
        got["OFF_END"] |= bool((cut & (c.why == vr.OFF_END)).any())
        if x.holes is not None:
            got["NO_SUFFIX"] |= bool((x.holes.cands.why == vr.NO_SUFFIX).any())
        hit_v, hit_a, hit_p = (r[:, 0] != vr.NONE for r in (x.verify, x.align, x.placed))
        got["MULTI verify"] |= bool((hit_v & ((x.verify[:, 1] & vr.MULTI) != 0)).any())
        got["MULTI align"] |= bool((hit_a & ((x.align[:, 1] & ar.MULTI) != 0)).any())
        got["MULTI place"] |= bool((hit_p & ((x.placed[:, 1] & wr.MULTI) != 0)).any())
        got["bound verify"] |= bool((~hit_v & (vr.records(c, x.S, x.occ, m)[:, 0] != vr.NONE)).any())
        got["bound align"] |= bool((~hit_a & (ar.records(x.aligned, x.S, x.occ, band, m)[:, 0] != ar.NONE)).any())
        got["bound place"] |= bool((~hit_p & (wr.place(x.begins, x.windows, m)[:, 0] != wr.NONE)).any())
        for kind, p in x.walks.items():
            paths = x.paths[kind][0]
            has = paths[:, 0] != pr.NONE
            for t in np.flatnonzero(has):
                ops = p.ops_of(t)
                got["I run"] |= pr.OP_I in ops
                got["D run"] |= pr.OP_D in ops
            got["OVERFLOW"] |= bool((has & ((paths[:, 1] & pr.OVERFLOW) != 0)).any())
            some = p.B != pr.NONE
            got["no path: NONE"] |= bool((~some).any())
            got["no path: n < m"] |= bool((some & (n < m)).any())
            got["no path: B > n"] |= bool((some & (n >= m) & (p.B > n)).any())
            got["no path: B - c > w"] |= bool((some & (n >= m) & (p.B <= n) & (p.B - np.minimum(p.B, n - m) > band)).any())
        lo, ln = x.windows[:, 0].astype(np.int64), x.windows[:, 1].astype(np.int64)
        got["b = n"] |= bool(((ln > 0) & (lo <= n) & (lo + ln - 1 >= n)).any())
        got["past n"] |= bool(((ln > 0) & (lo <= n) & (lo + ln - 1 > n)).any())
        got["lo > n"] |= bool(((ln > 0) & (lo > n)).any())
        got["len 0"] |= bool((ln == 0).any())
        for mode in x.modes.values():
            y = mode.paired[:, 1]
            got["PROPER | RESCUED"] |= bool(((mode.paired[:, 0] != wr.NONE) & ((y & wr.PROPER) != 0) & ((y & wr.RESCUED) != 0)).any())
            h4, r4 = x.align.reshape(-1, 4, 2), mode.resc.reshape(-1, 4, 2)
            got["no combination"] |= any(not wr.pair_keys(h4[p], r4[p], m, x.min_frag, x.max_frag) and
                                         (h4[p, :, 0] != wr.NONE).any() for p in range(h4.shape[0]))
        if n < m:
            # the header: verify and align score nothing, no task has a path, windows still place with e(b) >= m - (n - b)
            assert (x.verify == (vr.NONE, 0)).all() and (x.align == (ar.NONE, 0)).all(), (x.i, "a record where n < m")
            assert all((pp[:, 0] == pr.NONE).all() for pp, _ in x.paths.values()), (x.i, "a path where n < m")
            full = wr.place(x.begins, x.windows, m)
            E = (full[:, 1] & wr.EDITS).astype(np.int64)
            if ((full[:, 0] != wr.NONE) & (E >= m - n)).any():
                short.append(x.i)
            assert (E[full[:, 0] != wr.NONE] >= m - n).all(), (x.i, "a placement cheaper than the missing bases")
    assert len(short) >= 6, ("worlds with n < m and a window record", short)
    assert tiny >= 6 and small >= 6, ("worlds with n < 16, with 16 <= n < 64", tiny, small)
    assert residues == set(range(16)), ("n % 16 among worlds with a scored candidate", sorted(residues))
    assert shifts == set(range(16)), ("BandWindow::sh among scored candidates", sorted(shifts))
    assert sum(bool(x.modes) for x in ws) >= 6, "pair worlds"
    assert all(got.values()), ("not shown", [k for k, v in got.items() if not v])
