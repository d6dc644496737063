"""The model of kfmi_sam_lines (kstep_fmi.h, "SAM lines"): Python string
formatting from decoded records, written from the header's definition and not
from the C, an independent checker of a mapped line (replay), and the world the
SAM tests share.

model_lines() takes what the call takes -- the text, the contig table, the
reads, the hits / paths / cigars / quals records as arrays -- and returns one
line per read.  The path records it is given come from kfmi_align_paths_cpu,
which tests/test_path_host.py pins to its own model; nothing of the SAM code
is used here.

replay() trusts neither: it parses a mapped line, rebuilds the reference
segment from SEQ + CIGAR + MD alone and compares it with the text.

world(K) builds, per read length, a text of 4,100 bases, four contigs and a
batch of reads whose hits are caller-filled, so that each placement sits where
a case needs it; it asserts on the model alone that every case the tests claim
to cover occurs.
"""
import re
from functools import lru_cache

import numpy as np

import util

NONE = 0xFFFFFFFF
EDITS_MASK, RUNS_SHIFT, RUNS_MASK, OVERFLOW = 0xFFFF, 16, 0xFFF, 0x80000000
FWD, REV, BOTH = 1, 2, 3
CIGAR_M = 1
ST_NONE, ST_OVERFLOW, ST_SPAN, ST_OK = 0, 1, 2, 3
OPS = "MIDNSHP=X"
N_TEXT = 4100
LENGTHS = (1, 20, 100, 256)
BANDS = (0, 3, 15)
MAX_BAND = 15


def letters(raw) -> str:
    """ "ACGT"[base2index(byte)] of every byte."""
    return "".join("ACGT"[util.code_of(int(b))] for b in bytes(raw))


def revcomp(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


class Table:
    """The contig table as plain lists."""

    def __init__(self, names, begins, lengths):
        self.names = [n if isinstance(n, str) else n.decode() for n in names]
        self.begins = [int(b) for b in begins]
        self.lengths = [int(x) for x in lengths]

    def header(self) -> bytes:
        out = "@HD\tVN:1.6\tSO:unknown\n"
        for n, ln in zip(self.names, self.lengths):
            out += "@SQ\tSN:%s\tLN:%d\n" % (n, ln)
        return out.encode()

    def holder(self, B: int, end: int):
        """The contig i with begins[i] <= B and end <= begins[i] + lengths[i], or None."""
        for i in range(len(self.begins)):
            if self.begins[i] <= B and end <= self.begins[i] + self.lengths[i]:
                return i
        return None


def runs_of(py: int, words) -> list:
    return [(int(v) >> 4, int(v) & 15) for v in words[:(py >> RUNS_SHIFT) & RUNS_MASK]]


def status(tab: Table, n: int, m: int, band: int, C: int, B: int, px: int, py: int, words):
    """(status, contig) of one task, in the header's order."""
    if px == NONE:
        return ST_NONE, None
    if py & OVERFLOW:
        return ST_OVERFLOW, None
    end = px
    if end <= B or n < m or B > n:
        return ST_SPAN, None
    c = min(B, n - m)
    if B - c > band or end > c + m + band:
        return ST_SPAN, None
    runs = runs_of(py, words)
    if not 1 <= len(runs) <= 2 * C or any(ln < 1 or op not in (1, 2, 7, 8) for ln, op in runs):
        return ST_SPAN, None
    if sum(ln for ln, op in runs if op != 2) != m or sum(ln for ln, op in runs if op != 1) != end - B:
        return ST_SPAN, None
    i = tab.holder(B, end)
    return (ST_SPAN, None) if i is None else (ST_OK, i)


def cigar_string(runs, options: int) -> str:
    if not options & CIGAR_M:
        return "".join("%d%s" % (ln, OPS[op]) for ln, op in runs)
    out, acc = "", 0
    for ln, op in runs:
        if op in (7, 8):
            acc += ln
            continue
        if acc:
            out += "%dM" % acc
            acc = 0
        out += "%d%s" % (ln, OPS[op])
    return out + ("%dM" % acc if acc else "")


def md_string(runs, B: int, text: str) -> str:
    out, c, p = "", 0, B
    for ln, op in runs:
        if op == 7:
            c += ln
            p += ln
        elif op == 8:
            for _ in range(ln):
                out += "%d%s" % (c, text[p])
                c = 0
                p += 1
        elif op == 2:
            out += "%d^%s" % (c, text[p:p + ln])
            c = 0
            p += ln
    return out + "%d" % c


def model_lines(text: bytes, tab: Table, reads: np.ndarray, hits, paths, cigars, quals, strands: int, C: int, band: int,
                options: int, name_base: int, notes=None) -> list:
    """One bytes line per read, each ending in a newline.  notes: a set that
    collects what occurred (see world())."""
    t = letters(text)
    n, (num, m) = len(t), reads.shape
    ns = 2 if strands == BOTH else 1
    hits = np.asarray(hits).reshape(ns * num, 2)
    paths = np.asarray(paths).reshape(ns * num, 2)
    cigars = np.asarray(cigars).reshape(ns * num, 2 * C)
    quals = None if quals is None else np.asarray(quals).reshape(ns * num, 2)
    notes = set() if notes is None else notes
    out = []
    for q in range(num):
        fwd = letters(reads[q])
        tasks = []
        for s in range(ns):
            u = ns * q + s
            B, px, py = int(hits[u, 0]), int(paths[u, 0]), int(paths[u, 1])
            st, i = status(tab, n, m, band, C, B, px, py, cigars[u])
            tasks.append((st, py & EDITS_MASK, u, i, strands == REV or s == 1))
            if st == ST_SPAN:
                note_span(notes, tab, B, px)
        ok = [x for x in tasks if x[0] == ST_OK]
        if ns == 2:
            note_both(notes, tasks)
        if not ok:
            r = max(x[0] for x in tasks)
            notes.add("YU%d" % r)
            out.append(("%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\tYU:i:%d\n" % (name_base + q, fwd, r)).encode())
            continue
        st, D, u, i, rev = min(ok, key=lambda x: (x[1], x[4]))   # fewer edits; FWD on a tie
        B, py = int(hits[u, 0]), int(paths[u, 1])
        runs = runs_of(py, cigars[u])
        mapq = 255 if quals is None else min(int(quals[u, 0]), 254)
        pos = B - tab.begins[i] + 1
        cg, md = cigar_string(runs, options), md_string(runs, B, t)
        note_mapped(notes, tab, i, pos, int(paths[u, 0]), runs, cg, md, mapq, m, options)
        out.append(("%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*\tNM:i:%d\tMD:Z:%s\n" % (
            name_base + q, 16 if rev else 0, tab.names[i], pos, mapq, cg, revcomp(fwd) if rev else fwd, D, md)).encode())
    return out


def offsets_of(lines) -> np.ndarray:
    return np.concatenate(([0], np.cumsum([len(x) for x in lines]))).astype(np.uint64)


# ---- what occurred, for the world's conditions ----

def note_span(notes, tab, B, end):
    if end == B:
        notes.add("insertions only")
    if B < tab.begins[0]:
        notes.add("before the first contig")
    for i, (b, ln) in enumerate(zip(tab.begins, tab.lengths)):
        if B + 1 == b:
            notes.add("crosses a begin by one")
        if b <= B < b + ln and end == b + ln + 1:
            notes.add("crosses an end by one")
        nxt = tab.begins[i + 1] if i + 1 < len(tab.begins) else None
        if nxt is not None and b + ln <= B < nxt:
            notes.add("inside a gap")


def note_both(notes, tasks):
    (sf, df, *_), (sr, dr, *_) = tasks
    if sf == ST_OK and sr == ST_OK:
        notes.add("both OK, tie" if df == dr else "both OK, FWD chosen" if df < dr else "both OK, REV chosen")
    elif sf == ST_OK or sr == ST_OK:
        notes.add("one side OK")
    elif sf != sr:
        notes.add("both fail, different codes")


def note_mapped(notes, tab, i, pos, end, runs, cg, md, mapq, m, options):
    if pos == 1:
        notes.add("first base")
    if end == tab.begins[i] + tab.lengths[i]:
        notes.add("last base")
    if pos in (9, 10, 99, 100, 999, 1000):
        notes.add("POS %d" % pos)
    plain = cigar_string(runs, 0)
    if re.match(r"0[ACGT]", md):
        notes.add("MD leading X")
    if re.search(r"[ACGT]0$", md):
        notes.add("MD trailing X")
    if re.search(r"(?<!\^)[ACGT]0[ACGT]", md) and re.search(r"\d+X", plain) and any(op == 8 and ln > 1 for ln, op in runs):
        notes.add("MD adjacent X")
    if re.search(r"\d+X\d+D", plain):
        notes.add("X then D")
    if re.search(r"\d+D\d+X", plain):
        notes.add("D then X")
    if re.search(r"\d+=\d+I\d+=", plain):
        notes.add("I between matches")
    for c in re.findall(r"\d+", md):
        if c in ("9", "10", "99", "100"):
            notes.add("MD count " + c)
    if plain == "%d=" % m:
        notes.add("all =")
    notes.add("MAPQ %d" % mapq)
    if options & CIGAR_M and re.search(r"\d+=\d+X\d+=", plain) and re.fullmatch(r"\d+M", cg):
        notes.add("=X= merged into one M")


REQUIRED = {
    "first base", "last base", "crosses a begin by one", "crosses an end by one", "inside a gap",
    "before the first contig", "POS 9", "POS 10", "POS 99", "POS 100", "POS 999", "POS 1000", "MD leading X",
    "MD trailing X", "MD adjacent X", "X then D", "D then X", "I between matches", "MD count 9", "MD count 10",
    "MD count 99", "MD count 100", "all =", "YU1", "insertions only", "YU0", "YU2", "both OK, FWD chosen",
    "both OK, REV chosen", "both OK, tie", "one side OK", "both fail, different codes", "MAPQ 0", "MAPQ 60", "MAPQ 255",
    "=X= merged into one M",
}


# ---- the independent checker ----

def replay(line: bytes, tab: Table, text: bytes) -> None:
    """A mapped line holds to the text: the reference segment rebuilt from SEQ,
    CIGAR and MD equals the text at POS, NM is the X + I + D bases, and the =,
    X, M and I bases are SEQ."""
    f = line.decode().rstrip("\n").split("\t")
    assert len(f) == 13 and f[6:9] == ["*", "0", "0"] and f[10] == "*", line
    assert f[1] in ("0", "16") and f[11].startswith("NM:i:") and f[12].startswith("MD:Z:"), line
    i = tab.names.index(f[2])
    pos, seq, nm, md = int(f[3]), f[9], int(f[11][5:]), f[12][5:]
    cig = [(int(a), b) for a, b in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
    assert "".join("%d%s" % x for x in cig) == f[5] and all(ln > 0 for ln, _ in cig), line
    # MD as one item per reference base: None = the read's base, a letter = a mismatch, ("^", letter) = deleted
    items, k = [], 0
    assert re.fullmatch(r"\d+(([ACGT]|\^[ACGT]+)\d+)*", md), line
    for tok in re.findall(r"\d+|\^[ACGT]+|[ACGT]", md):
        if tok[0].isdigit():
            items += [None] * int(tok)
        elif tok[0] == "^":
            items += [("^", c) for c in tok[1:]]
        else:
            items.append(tok)
    ref, r, edits = "", 0, 0
    for ln, op in cig:
        if op == "I":
            r += ln
            edits += ln
            continue
        assert op in "=XMD", line
        for _ in range(ln):
            it = items[k]
            k += 1
            if op == "D":
                assert isinstance(it, tuple), line
                ref += it[1]
                edits += 1
                continue
            assert not isinstance(it, tuple), line
            if it is None:
                assert op in "=M", line
                ref += seq[r]
            else:
                assert op in "XM" and it != seq[r], line
                ref += it
                edits += 1
            r += 1
    assert k == len(items) and r == len(seq), line
    assert nm == edits, line
    begin = tab.begins[i] + pos - 1
    assert pos >= 1 and begin + len(ref) <= tab.begins[i] + tab.lengths[i], line
    assert ref == letters(text[begin:begin + len(ref)]), line


# ---- the world ----

def other(c: int, *avoid) -> int:
    """A base that differs from c and from every base in `avoid`."""
    for x in b"ACGT":
        if x != c and x not in avoid:
            return x
    raise AssertionError("no base left")


def edited(text: bytearray, B: int, m: int, script) -> bytes:
    """A read of m bases that follows the text from B on with the script's
    edits: ("X", at) a substituted base, ("D", at) a text base skipped, ("I", at)
    a base the text does not have, `at` the text offset from B."""
    out, j = bytearray(), B
    for op, at in script:
        out += text[j:B + at]
        j = B + at
        nxt = text[j + 1] if j + 1 < len(text) else 0
        if op == "X":
            out.append(other(text[j], nxt))
            j += 1
        elif op == "D":
            j += 1
        else:
            out.append(other(text[j], text[j - 1] if j else 0))
    out += text[j:j + m - len(out)]
    assert len(out) == m, (B, m, script)
    return bytes(out)


class World:
    """One read length's text, table, reads and caller-filled hits."""

    def __init__(self, m: int):
        rng = np.random.default_rng(27_000 + m)
        t = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=N_TEXT).tobytes())
        b0 = 7
        b1 = b0 + 700                      # the second contig follows the first without a gap, and is exactly m long
        b2 = b1 + m + 50
        b3 = b2 + 1500 + 33
        self.m = m
        self.table = Table(["a", "L" * 254, "chr3", "ctg_4|x"], [b0, b1, b2, b3], [700, m, 1500, N_TEXT - 20 - b3])
        e0, e1, e2 = b1, b1 + m, b2 + 1500
        reads, hf, hr = [], [], []

        def add(read, f=NONE, r=NONE):
            assert len(read) == m
            reads.append(read)
            hf.append(f)
            hr.append(r)

        p3 = b3 + 40
        if m >= 8:   # the strand cases: S at p3, its reverse complement with two substitutions 300 further on
            rc = bytearray(revcomp(bytes(t[p3:p3 + m]).decode()).encode())
            rc[1], rc[m - 2] = other(rc[1]), other(rc[m - 2])
            t[p3 + 300:p3 + 300 + m] = rc
        if m % 2 == 0:   # a reverse-complement palindrome: both strands of it are the same read
            half = bytes(t[p3 + 700:p3 + 700 + m // 2]).decode()
            t[p3 + 700:p3 + 700 + m] = (half + revcomp(half)).encode()
        seg = lambda B: bytes(t[B:B + m])   # noqa: E731
        minus = lambda B: revcomp(seg(B).decode()).encode()   # noqa: E731
        for B in (b0, e0 - m, b1, b2 - 1, e2 - m + 1, b1 - 1, e1 + 10, 0, 3):   # edges, gaps, before the first contig
            add(seg(B), B, NONE)
        for pos in (9, 10, 99, 100, 999, 1000):
            add(seg(b2 + pos - 1), b2 + pos - 1, NONE)
        scripts = [[("X", 0)], [("X", m - 1)], [("X", m // 2), ("X", m // 2 + 1)], [("X", m // 3), ("D", m // 3 + 1)],
                   [("D", m // 3), ("X", m // 3 + 1)], [("I", m // 2)], [("X", 9)], [("X", 10)], [("X", 99)], [("X", 100)],
                   [("D", m // 4), ("D", m // 4 + 1)], [("X", 2), ("I", m // 2), ("D", m - 5)], [("I", 3), ("I", 4)],
                   [("X", m // 5), ("D", m // 5 + 1), ("X", m // 5 + 2)], [("D", 5), ("X", 6), ("X", 7)],
                   [("X", k) for k in range(2, m - 2, max(2, m // 12))]]
        k = 0
        for sc in scripts:
            if all(2 <= at < m - 2 or (op == "X" and 0 <= at < m) for op, at in sc) and len({at for _, at in sc}) == len(sc):
                B = b0 + 50 + 7 * k
                k += 1
                add(edited(t, B, m, sc), B, NONE)
        if m == 1:   # a base that differs from the text at B and after it: under a band the path is one I
            for B in (b0 + 50, b0 + 51, b0 + 52, b0 + 53):
                add(bytes([other(t[B], t[B + 1])]), B, NONE)
        add(seg(b2 + 5))                                    # no hit at all
        add(minus(b2 + 300), NONE, b2 + 300)                # the REV task alone
        add(minus(b2 - 1), NONE, b2 - 1)                    # ... and across an edge
        add(seg(b2 + 20), NONE, e1 + 10)                    # both fail, with different codes
        if m >= 8:
            add(seg(p3), p3, p3 + 300)                      # both OK, FWD has fewer edits
            add(minus(p3 + 300), p3, p3 + 300)              # both OK, REV has fewer
        if m % 2 == 0:
            add(seg(p3 + 700), p3 + 700, p3 + 700)          # both OK, a tie
        self.text = bytes(t)
        self.reads = np.frombuffer(b"".join(reads), dtype=np.uint8).reshape(len(reads), m).copy()
        self.hf, self.hr = np.array(hf, dtype=np.uint32), np.array(hr, dtype=np.uint32)

    def batch(self, num: int):
        """num reads and their hits: the world's, repeated in order."""
        pick = np.arange(num) % self.reads.shape[0]
        return np.ascontiguousarray(self.reads[pick]), self.hf[pick], self.hr[pick]


def task_hits(hf, hr, strands: int) -> np.ndarray:
    """Word x of every task's caller-filled hit."""
    if strands == FWD:
        return hf.copy()
    if strands == REV:
        return hr.copy()
    return np.stack([hf, hr], axis=1).reshape(-1)


def task_quals(tasks: int) -> np.ndarray:
    """Caller-filled quality records: word x cycles through values at and past the cap."""
    x = np.array([0, 60, 37, 254, 255, 300, 3], dtype=np.uint32)[np.arange(tasks) % 7]
    return np.stack([x, np.full(tasks, 0xA5A5A5A5, dtype=np.uint32)], axis=1).reshape(-1)


def swap_first_dx(text: bytes, reads: np.ndarray, strands: int, hits, paths, cigars, C: int) -> bool:
    """kfmi_align_paths puts gaps first, so its records never hold an X run
    followed by a D run: the first task whose runs hold 1D 1X, and whose read
    base also differs from the text base the D skips, gets the equivalent 1X 1D
    written into its words in place -- a caller-made record, which
    kfmi_sam_lines takes like any other.  Returns whether one was found."""
    t = letters(text)
    ns = 2 if strands == BOTH else 1
    hits, paths, cigars = hits.reshape(-1, 2), paths.reshape(-1, 2), cigars.reshape(-1, 2 * C)
    for u in range(hits.shape[0]):
        px, py = int(paths[u, 0]), int(paths[u, 1])
        if px == NONE or py & OVERFLOW:
            continue
        runs = runs_of(py, cigars[u])
        fwd = letters(reads[u // ns])
        p = revcomp(fwd) if strands == REV or (ns == 2 and u & 1) else fwd
        i, j = 0, int(hits[u, 0])
        for r, (ln, op) in enumerate(runs):
            if op == 2 and ln == 1 and r + 1 < len(runs) and runs[r + 1] == (1, 8) and p[i] != t[j]:
                cigars[u, r], cigars[u, r + 1] = 1 << 4 | 8, 1 << 4 | 2
                return True
            i += ln if op != 2 else 0
            j += ln if op != 1 else 0
    return False


class HostChain:
    """The handles of one batch on the host: caller-filled hits, then kfmi_align_paths_cpu."""

    def __init__(self, K, w: World, num: int, strands: int, band: int, C: int, with_quals: bool):
        self.K, self.w, self.strands, self.band, self.C = K, w, strands, band, C
        self.reads, hf, hr = w.batch(num)
        self.ns = 2 if strands == BOTH else 1
        self.T = self.ns * num
        self.Q = K.Queries.from_array(self.reads)
        self.H, self.P, self.G = K.Results.alloc(self.T), K.Results.alloc(self.T), K.Results.alloc(self.T * C)
        self.U = K.Results.alloc(self.T) if with_quals else None
        self.B = task_hits(hf, hr, strands)
        a = self.H.array().reshape(self.T, 2)
        a[:, 0], a[:, 1] = self.B, 0xA5A5A5A5
        if with_quals:
            self.U.array()[:] = task_quals(self.T)
        K.align_paths_cpu(w.text, self.Q, self.H, self.P, self.G, strands, band, w.m, C)
        swap_first_dx(w.text, self.reads, strands, self.H.array(), self.P.array(), self.G.array(), C)

    def records(self):
        return (self.H.array().copy(), self.P.array().copy(), self.G.array().copy(),
                None if self.U is None else self.U.array().copy())

    def model(self, options: int, name_base: int, notes=None):
        h, p, g, u = self.records()
        return model_lines(self.w.text, self.w.table, self.reads, h, p, g, u, self.strands, self.C, self.band, options,
                           name_base, notes)

    def close(self):
        for h in (self.Q, self.H, self.P, self.G, self.U):
            if h is not None:
                h.close()


def configs():
    """(m, strands, band, C, with_quals, options) of the host test: every length, strand mode, option value and
    band, with the small C and the absent quals where they show something."""
    for m in LENGTHS:
        for strands in (FWD, REV, BOTH):
            for band in BANDS:
                for options in (0, CIGAR_M):
                    yield m, strands, band, 8, band != 15, options
            yield m, strands, 3, 1, True, 0


@lru_cache(maxsize=None)
def world(K):
    """{m: World}; asserts on the model alone that every case of REQUIRED occurs somewhere in configs()."""
    w = {m: World(m) for m in LENGTHS}
    notes = set()
    for m, strands, band, C, with_quals, options in configs():
        h = HostChain(K, w[m], w[m].reads.shape[0], strands, band, C, with_quals)
        try:
            h.model(options, 0, notes)
        finally:
            h.close()
    missing = REQUIRED - notes
    assert not missing, sorted(missing)
    return w
