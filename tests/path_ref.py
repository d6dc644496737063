"""Align paths: the model, the reads, the hits and the non-vacuity conditions
shared by test_path_host.py and test_path_gpu.py.

The model restates the definition of kstep_fmi.h ("align paths") in numpy on
the text's codes; it calls nothing from the library.  table() fills the full
band table A(i, d) of many tasks at once (a Python loop over the read's rows;
the chain of skipped text bases inside a row is a running minimum over the
band, as in align_ref.row0), Walk takes the definition's walk through it, all
tasks in step, and records() forms `paths` and `cigars` for any cut of
max_edits and C.  Walk(reverse=True) is the same walk with the priority
reversed (diagonal, I, D): it only serves the condition that pins the priority.

Worlds (world()): align_ref.world's four texts with their reads, seed records
and aligned rows, and two of align_worlds' texts -- allA and tandem -- with
align_worlds.real_reads and the reads of align_worlds.direct as BOTH tasks.
Every text gets one more batch of 100-base reads ("x"), which the conditions
need: windows with ten spaced substitutions (E > 8 at band 8), with six, with a
deletion and an insertion, with a tandem unit spliced in and, where the text
lacks a letter, with that letter strewn in.

Hits.  seed_hits() are word x of align_ref.records -- what kfmi_align_seeds
leaves on the device, pinned to that model by test_align_gpu.py.  hand_hits()
are caller-filled: the same begin positions moved by -2 .. 2, and at fixed
tasks KFMI_HIT_NONE, n + 1 (B > n), n - m + w + 1 (B - c > w), n - m + 1 and
n - m + min(w, 2) (B + m > n, so c < B), n, 0 and 1 (B < w).

Non-vacuity (assert_not_vacuous, on the model alone, per text over its cases
with m >= 24 at the bands >= 4, which are 8 and 15):
  * tasks whose CIGAR has an I, a D and an X, and one with a D and an I;
  * a task whose runs differ under the reversed priority;
  * a task with a path and B < w; one with B + m > n, from hand_hits;
  * tasks with B - c > w, with B > n and with x = NONE, all without a path;
  * a task with D > 1, which max_edits = 1 cuts;
  * a task of 3 or 4 runs: it overflows at C = 1 and fits at C = 2;
  * a hit of the align step with E > w.
What cannot hold, and why.  On allA every cell of a row sees the same text, so
skipping a text base never lowers a cell's value: A(i, d + 1) + 1 = A(i, d)
would need a path from (i, d + 1) that is cheaper by one, and shifted back by
one base it is a path from (i, d) at the same cost or, where it leaves the band
or the text, no path at all.  No walk on allA takes a D; allA is excused by
name from the D and from the D-and-I condition."""
import numpy as np

import align_ref as ar
import align_worlds as aw
import seed_ref as sr
import verify_ref as vr
from skip_texts import ACGT
from strand_reads import code_of

NONE = 0xFFFFFFFF
EDITS_MASK, RUNS_SHIFT, RUNS_MASK, OVERFLOW = 0xFFFF, 16, 0xFFF, 0x80000000
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
MAX_ENTRIES = 32
BANDS = (0, 1, 3, 8, 15)                  # all of them bands of align_ref.BANDS: the seed hits exist
LENGTHS = ar.LENGTHS
AW_TEXTS = ("allA", "tandem")
AW_LENGTHS = (17, 100, 129, 256)
INF = 1 << 20
A, C, G, T = (int(b) for b in ACGT)


def table(w: vr.World, pc: np.ndarray, c: np.ndarray, band: int) -> np.ndarray:
    """int32 [N, m + 1, 2 * band + 1]: A(i, d) of N tasks at index [i, band - d]
    (pc: their reads' codes [N, m]; c: their bands' centres), INF for invalid
    cells.  The cells of a row are laid out by r = band - d, so that the chain
    of skipped text bases (d + 1 -> d) runs forward."""
    n, (N, m), Bw = w.n, pc.shape, 2 * band + 1
    r = np.arange(Bw, dtype=np.int64)
    out = np.empty((N, m + 1, Bw), np.int32)
    codes = w.codes if n else np.zeros(1, np.uint8)
    for i in range(m, -1, -1):
        j = c.astype(np.int64)[:, None] + i + band - r[None, :]
        valid = (j >= 0) & (j <= n)
        if i == m:
            out[:, i] = np.where(valid, 0, INF)
            continue
        nxt = out[:, i + 1].astype(np.int64)
        tb = codes[np.clip(j, 0, max(n - 1, 0))]
        base = np.where(j < n, nxt + (pc[:, i][:, None] != tb), INF)           # P[i] on T[j], when j < n
        base[:, :-1] = np.minimum(base[:, :-1], nxt[:, 1:] + 1)                # a read base with no text base: from d - 1
        base = np.where(valid, base, INF)
        # text bases skipped: A(i, r) = min over r' <= r of base(r') + r - r' (every cell past a valid r' has j < n)
        base = np.minimum.accumulate(base - r[None, :], axis=1) + r[None, :]
        out[:, i] = np.where(valid, np.minimum(base, INF), INF)
    return out


class Walk:
    """The definition's walk of every task of one (text, tasks, B, band): ok (the
    task has a path before max_edits is asked), D, end and runs (per task the
    u32 words len << 4 | op of its whole path)."""

    def __init__(self, w: vr.World, tasks: np.ndarray, B: np.ndarray, band: int, reverse: bool = False):
        n, (N, m) = w.n, tasks.shape
        self.N, self.m, self.n, self.band = N, m, n, band
        self.B = B = np.asarray(B, np.int64)
        pc = code_of(tasks).astype(np.uint8)
        pos = (B != NONE) & (n >= m) & (B <= n)
        c = np.where(pos, np.minimum(B, n - m), 0)
        self.c = c
        self.ok = ok = pos & (B - c <= band)
        idx = np.flatnonzero(ok)
        self.D = np.zeros(N, np.int64)
        self.end = np.full(N, -1, np.int64)
        self.runs = [np.empty(0, np.uint32) for _ in range(N)]
        self.nruns = np.zeros(N, np.int64)
        if not idx.size:
            return
        tab = table(w, pc[idx], c[idx], band).astype(np.int64)
        pcs, cs = pc[idx], c[idx]
        M = idx.size
        ar_ = np.arange(M)
        i = np.zeros(M, np.int64)
        k = band - (B[idx] - cs)                                   # the cell's index r = band - d
        v = tab[ar_, 0, k]
        assert (v < INF).all()                                     # D is finite (kstep_fmi.h)
        self.D[idx] = v
        ops = np.zeros((M, m + int(v.max()) + 1), np.int8)          # a path has m read bases and at most D gaps
        step = 0
        codes = w.codes if n else np.zeros(1, np.uint8)
        while True:
            act = i < m
            if not act.any():
                break
            ii = np.minimum(i, m - 1)
            j = cs + ii + band - k
            mis = (pcs[ar_, ii] != codes[np.clip(j, 0, max(n - 1, 0))]).astype(np.int64)
            dele = act & (k >= 1) & (j < n) & (tab[ar_, ii, np.maximum(k - 1, 0)] + 1 == v)
            ins = act & (k + 1 <= 2 * band) & (tab[ar_, ii + 1, np.minimum(k + 1, 2 * band)] + 1 == v)
            diag = act & (j < n) & (tab[ar_, ii + 1, k] + mis == v)
            assert (dele | ins | diag)[act].all()
            if reverse:
                ins &= ~diag
                dele &= ~(diag | ins)
            else:
                ins &= ~dele
                diag &= ~(dele | ins)
            ops[:, step] = np.where(dele, OP_D, np.where(ins, OP_I, np.where(diag, np.where(mis == 1, OP_X, OP_EQ), 0)))
            v = v - np.where(dele | ins, 1, np.where(diag, mis, 0))
            i = i + (ins | diag)
            k = k + ins.astype(np.int64) - dele.astype(np.int64)
            step += 1
        assert (v == 0).all()
        self.end[idx] = cs + m + band - k
        for a, t in enumerate(idx):
            o = ops[a][ops[a] != 0].astype(np.uint32)
            cut = np.flatnonzero(np.diff(o)) + 1
            starts = np.concatenate([[0], cut])
            lens = np.diff(np.concatenate([starts, [o.size]])).astype(np.uint32)
            self.runs[t] = (lens << 4 | o[starts]).astype(np.uint32)
        self.nruns = np.asarray([r.size for r in self.runs], np.int64)

    def ops_of(self, t: int) -> set:
        return {int(x) & 15 for x in self.runs[t]}


def records(p: Walk, max_edits: int, C: int, rows=slice(None)):
    """(paths uint32 [N, 2], cigars uint32 [N, 2 * C]) of the definition; rows: a cut of the tasks."""
    has = p.ok & (p.D <= max_edits)
    nruns = np.where(has, p.nruns, 0)
    over = nruns > 2 * C
    paths = np.zeros((p.N, 2), np.uint32)
    paths[:, 0] = np.where(has, p.end, NONE)
    paths[:, 1] = np.where(has, p.D | (nruns << RUNS_SHIFT) | np.where(over, OVERFLOW, 0), 0)
    cig = np.zeros((p.N, 2 * C), np.uint32)
    for t in np.flatnonzero(has & ~over):
        cig[t, :nruns[t]] = p.runs[t]
    return np.ascontiguousarray(paths[rows]), np.ascontiguousarray(cig[rows])


def check_properties(w: vr.World, tasks: np.ndarray, B, band: int, paths: np.ndarray, cig: np.ndarray, what) -> int:
    """The header's sum and replay properties on every record with a path that fits; returns how many it checked."""
    pc, m, done = code_of(tasks), tasks.shape[1], 0
    for t in range(tasks.shape[0]):
        x, y = int(paths[t, 0]), int(paths[t, 1])
        if x == NONE:
            assert y == 0 and not cig[t].any(), (what, t)
            continue
        runs = (y >> RUNS_SHIFT) & RUNS_MASK
        if y & OVERFLOW:
            assert runs > cig.shape[1] and not cig[t].any(), (what, t)
            continue
        words = [int(v) for v in cig[t, :runs]]
        assert all(v >> 4 for v in words) and not cig[t, runs:].any(), (what, t)
        assert all((a & 15) != (b & 15) for a, b in zip(words, words[1:])), (what, t, "two runs of one op")
        total = {o: sum(v >> 4 for v in words if v & 15 == o) for o in (OP_I, OP_D, OP_EQ, OP_X)}
        assert total[OP_EQ] + total[OP_X] + total[OP_I] == m, (what, t)
        assert int(B[t]) + total[OP_EQ] + total[OP_X] + total[OP_D] == x, (what, t)
        assert total[OP_X] + total[OP_I] + total[OP_D] == y & EDITS_MASK, (what, t)
        if band == 0:
            assert total[OP_I] == total[OP_D] == 0, (what, t)
        i, j = 0, int(B[t])
        for v in words:
            ln, o = v >> 4, v & 15
            if o in (OP_EQ, OP_X):
                same = pc[t, i:i + ln] == w.codes[j:j + ln]
                assert same.size == ln and (same.all() if o == OP_EQ else not same.any()), (what, t, "replay")
            i += ln if o != OP_D else 0
            j += ln if o != OP_I else 0
        assert (i, j) == (m, x), (what, t)
        done += 1
    return done


def seed_hits(a: ar.Aligned, band: int, m: int, rows=slice(None)):
    """(B, E): word x of the align step's records at S = 8, max_occ = 8 and no bound, and their edits (-1: none)."""
    rec = ar.records(a, 8, 8, band, m, rows)
    return rec[:, 0].astype(np.int64), ar.edits_of(rec)


def hand_hits(n: int, m: int, band: int, B: np.ndarray) -> np.ndarray:
    """Caller-filled begin positions from the align step's: moved by -2 .. 2,
    and the special ones of the module's text at tasks 0 .. 8 (where there are
    that many)."""
    B = np.asarray(B, np.int64)
    out = np.where(B == NONE, NONE, np.clip(B + (np.arange(B.size) % 5) - 2, 0, n))
    special = (NONE, n + 1, n - m + band + 1, n - m + 1, n - m + min(band, 2), n, 0, 1, max(n - m, 0))
    for t, b in enumerate(special[:B.size]):
        out[t] = b if 0 <= b <= n + 1 or b == NONE else NONE
    return out


def extra_reads(name: str, t: np.ndarray, m: int = 100) -> np.ndarray:
    """The batch "x" of the module's text: forward reads."""
    n = t.size
    rng = np.random.default_rng(61_000 + n)
    a0 = {"tandem": 150, "allA": 100}.get(name, (n // 3))
    absent = [b for b in (G, C, T, A) if b not in t]
    out = []

    def changed(a, at):
        r = t[a:a + m].copy()
        for p in at:
            r[p] = absent[0] if absent else ar.other_base(t, a + p, rng)
        return r

    for a in (a0, a0 + 7, 3, n - m - 2):
        out.append(changed(a, range(5, m, 10)))                    # ten substitutions
        out.append(changed(a, range(8, m, 16)))                    # six or seven
    for a in (a0, 2, n - m - 1):
        out.append(np.concatenate([t[a:a + m // 3], t[a + m // 3 + 1:a + 2 * m // 3 + 1],
                                   aw.foreign(t, a + 2 * m // 3 + 1, 1, rng), t[a + 2 * m // 3 + 1:a + m]]))
        unit = t[a + 4:a + 6]
        out.append(np.concatenate([t[a:a + 6], unit, unit, t[a + 6:a + m - 4]]))
        out.append(aw.inserted(t, a, m, 40, 6, rng))               # six foreign bases: I's, and X's where the band ends
        out.append(ar.deleted(t, a, m, 50, 2))
    for r in out:
        assert r.size == m
    return np.ascontiguousarray(np.stack(out))


def assert_not_vacuous(name: str, w: vr.World, walks) -> None:
    """walks: (m, band, Walk, reversed Walk, E of the align step or None for hand hits) of one text, m >= 24, band >= 4."""
    got = dict.fromkeys(("I", "D", "X", "D and I", "priority", "B < w", "c < B", "B - c > w", "B > n", "NONE", "D > 1",
                         "3 or 4 runs", "E > w"), False)
    for m, band, p, rv, E in walks:
        assert m >= 24 and band >= 4
        n = w.n
        for t in np.flatnonzero(p.ok):
            ops = p.ops_of(t)
            got["I"] |= OP_I in ops
            got["D"] |= OP_D in ops
            got["X"] |= OP_X in ops
            got["D and I"] |= OP_I in ops and OP_D in ops
            got["priority"] |= not np.array_equal(p.runs[t], rv.runs[t])
            got["3 or 4 runs"] |= p.runs[t].size in (3, 4)
        got["B < w"] |= bool((p.ok & (p.B < band)).any())
        got["D > 1"] |= bool((p.ok & (p.D > 1)).any())
        if E is None:
            got["c < B"] |= bool((p.ok & (p.B + m > n)).any())
            got["B - c > w"] |= bool(((p.B != NONE) & (p.B <= n) & ~p.ok).any())
            got["B > n"] |= bool(((p.B != NONE) & (p.B > n)).any())
        else:
            got["E > w"] |= bool(((E > band) & p.ok).any())
        got["NONE"] |= bool((p.B == NONE).any())
    if name == "allA":
        got["D"] = got["D and I"] = True                           # excused: see the module's text
    assert all(got.values()), (name, "not shown", [k for k, v in got.items() if not v])


_cache = {}
_walks = {}


def walk_of(name: str, label, k: int, band: int, kind: str):
    """(B, E or None, Walk) of the BOTH tasks of one case of world(): kind
    "seed" | "hand".  The single strands are cuts of it (verify_ref.strand_rows)."""
    key = (name, label, k, band, kind)
    if key not in _walks:
        x = _cache[name]
        m, q, both, per_k = x["cases"][label]
        B, E = seed_hits(per_k[k][2], band, m)
        if kind == "hand":
            B, E = hand_hits(x["world"].n, m, band, B), None
        _walks[key] = (B, E, Walk(x["world"], both, B, band))
    return _walks[key]


def world(K, oracle_mod) -> dict:
    """Per text: the World, the K = 1, 2 indexes and cases[label] = (m, q, both,
    {K: (iv, sp, Aligned)}) with label m for the texts' own reads and "x" for
    the extra batch; the conditions are asserted here, on the model alone.
    Built once per session."""
    if _cache:
        return _cache
    out = {}
    for name, x in ar.world(K, oracle_mod).items():
        cases = {m: (m, q, both, per_k) for m, (q, both, per_k) in x["cases"].items()}
        out[name] = dict(world=x["world"], text=x["text"], idx=x["idx"], cases=cases, search=x["search"], ks=(1, 2))
    for name, t in aw.texts().items():
        if name not in AW_TEXTS:
            continue
        w = vr.World(t)
        ti = AW_TEXTS.index(name)
        cases = {}
        for m in AW_LENGTHS:
            q = np.ascontiguousarray(np.concatenate([aw.real_reads(name, t, m, 71_000 + 100 * ti + m),
                                                     aw.direct(name, w, m, 72_000 + 100 * ti + m)[0]]))
            cases[m] = (m, q, sr.tasks_of(q, sr.BOTH), None)
        out[name] = dict(world=w, text=t, idx={2: K.Index.build(t.tobytes(), k=2, d=64)}, cases=cases,
                         search=aw.brute_search(w), ks=(2,))
    for name, x in out.items():
        q = extra_reads(name, x["text"])
        x["cases"]["x"] = (100, q, sr.tasks_of(q, sr.BOTH), None)
        for label, (m, q, both, per_k) in list(x["cases"].items()):
            if per_k is not None:
                continue
            per_k = {}
            for k in x["ks"]:
                iv, sp, _ = sr.reference(x["search"], both, k, 8)
                per_k[k] = (iv, sp, ar.Aligned(x["world"], both, vr.candidates(x["world"], both, iv, sp, 8), bands=BANDS))
            q.setflags(write=False)
            x["cases"][label] = (m, q, both, per_k)
    _cache.update(out)
    for name, x in out.items():
        walks = []
        for label in ("x", 100):
            m = x["cases"][label][0]
            for band in (8, 15):
                for kind in ("seed", "hand"):
                    B, E, p = walk_of(name, label, 2, band, kind)
                    walks.append((m, band, p, Walk(x["world"], x["cases"][label][2], B, band, reverse=True), E))
        assert_not_vacuous(name, x["world"], walks)
    return _cache
