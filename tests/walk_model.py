"""A host model of skip_walk's decisions (csrc/hip/kfmi_kernels.h), read by
read: which rounds are ordinary K-steps, which are skip lookups and whether
they match, and the one text jump -- where, with how many bases left, from a
line or from the flat tables, and how it ends.  It is built from brute force: a
suffix array of the text (util.suffix_array) and the textbook backward search
on it, one base at a time, which gives the true interval of every suffix of a
read, empty ones included.  From the library it takes the three numbers the
caller passes in -- the jump start's step count (ftab_auto_bases // K), the skip
table's step count (16 // K) and jump_min -- and nothing else.

The fields it returns are the ones kstep_fmi.decode_trace names, plus the
interval (L, R) the walk ends with.
"""
import numpy as np

import util

ACGT = np.frombuffer(b"ACGT", np.uint8)
W_LINE = 240                    # the longest window a line of the line table serves
MAX_M_GROUPED = 192             # the longest read launched with the lines' grouped form
SPLIT4, LINES, GROUPED = 4, 0x100, 0x200
TAKEN, REFUSED, DIFFERED, BAD_ISA = 0, 1, 2, 3
FIELDS = ("steps", "skip_hits", "skip_misses", "jump_tried", "jump_pos", "jump_nb", "jump_line", "jump_outcome",
          "start_steps", "jump_split")


class World:
    """A text with its suffix array, inverse, and the counts of the backward search."""

    def __init__(self, text):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        n = self.n = int(self.text.size)
        self.sa = np.asarray(util.suffix_array(self.text.tobytes() + b"$"), dtype=np.int64)
        assert self.sa.size == n + 1 and self.sa[0] == n                   # row 0 is the suffix "$"
        self.isa = np.empty(n + 1, dtype=np.int64)
        self.isa[self.sa] = np.arange(n + 1)
        code = np.searchsorted(ACGT, self.text)
        assert (ACGT[code] == self.text).all()
        bwt = np.where(self.sa > 0, code[self.sa - 1], -1)                 # -1: the '$'
        self.occ = np.zeros((4, n + 2), dtype=np.int64)                    # occ[c, i] = rows < i with BWT == c
        for c in range(4):
            self.occ[c, 1:] = np.cumsum(bwt == c)
        self.first = 1 + np.concatenate([[0], np.cumsum(np.bincount(code, minlength=4))[:3]])

    def intervals(self, reads):
        """(L, R), int64 [n, m + 1]: column j is the interval of the reads' last j bases."""
        reads = np.asarray(reads, dtype=np.uint8)
        n, m = reads.shape
        code = np.searchsorted(ACGT, reads)
        assert (ACGT[code] == reads).all()
        L = np.zeros((n, m + 1), dtype=np.int64)
        R = np.full((n, m + 1), self.n + 1, dtype=np.int64)
        for j in range(1, m + 1):
            c = code[:, m - j]
            L[:, j] = self.first[c] + self.occ[c, L[:, j - 1]]
            R[:, j] = self.first[c] + self.occ[c, R[:, j - 1]]
        return L, R


def jump_split_of(jump, lines, cls, m):
    """IdxArgs::jump_split as the kernel receives it: use_jump's bits under the
    settings, then the launch's rule for reads over 192 bases."""
    if not jump:
        return 1
    v = (SPLIT4 if cls == 4 else 0) | (LINES if lines else 0) | (GROUPED if lines == 1 and cls == 4 else 0)
    if (v & GROUPED) and m > MAX_M_GROUPED:
        v &= ~(LINES | GROUPED)
    return v


def play(world, k, reads, ftab_steps=0, skip=False, jump=False, jump_min=8, lines=1, cls=0, iv=None):
    """The walk of every read under the tables in effect: ftab_steps = the jump
    start's K-steps (0 = off), skip / jump = whether the table is there,
    lines = set_jump_lines' mode, cls = set_split_class' class.  iv: the reads'
    world.intervals, when the caller has them."""
    reads = np.asarray(reads, dtype=np.uint8)
    n, m = reads.shape
    Ls, Rs = iv if iv is not None else world.intervals(reads)
    rem = m % k
    steps = (m - rem) // k
    start = ftab_steps if ftab_steps and not rem and steps >= ftab_steps else 0   # the remainder table replaces it
    J = 16 // k
    split = jump_split_of(jump, lines, cls, m)
    text, sa, isa = world.text, world.sa, world.isa
    # beside the record's fields: the final interval, the bases left when the lane was first on one row (-1:
    # never) and its skip lookups with exactly J steps left -- what the classes below count
    out = {f: np.zeros(n, dtype=np.int64) for f in FIELDS + ("L", "R", "row1_left", "skip_last")}
    for f in ("jump_pos", "jump_nb", "jump_line", "jump_outcome", "row1_left"):
        out[f][:] = -1
    out["start_steps"][:] = start
    out["jump_split"][:] = split
    for i in range(n):
        read, Li, Ri = reads[i], Ls[i], Rs[i]
        pos = start
        L, R = int(Li[rem + k * pos]), int(Ri[rem + k * pos])
        dead = failed = False
        nsteps = hits = misses = 0
        while pos < steps:
            left = (steps - pos) * k                               # the read's first `left` bases remain
            row1 = R == L + 1
            if row1 and out["row1_left"][i] < 0:
                out["row1_left"][i] = left
            if jump and row1 and not failed and left >= jump_min:
                p = int(sa[L])                                     # where the matched suffix starts in the text
                out["jump_tried"][i] = 1
                out["jump_pos"][i] = pos
                out["jump_nb"][i] = left
                out["jump_line"][i] = 0
                if p < left:
                    out["jump_outcome"][i] = REFUSED
                    failed = True
                    continue
                out["jump_line"][i] = 1 if (split & LINES) and left <= W_LINE else 0
                if np.array_equal(text[p - left:p], read[:left]):
                    out["jump_outcome"][i] = TAKEN
                    L = int(isa[p - left])
                    R = L + 1
                    pos = steps
                else:
                    out["jump_outcome"][i] = DIFFERED
                    failed = True
                continue
            if skip and row1 and not dead and pos + J <= steps:
                p = int(sa[L])
                out["skip_last"][i] += pos + J == steps
                if p >= 16 and np.array_equal(text[p - 16:p], read[left - 16:left]):
                    hits += 1
                    pos += J
                    L = int(isa[p - 16])
                    R = L + 1
                    assert (L, R) == (int(Li[rem + k * pos]), int(Ri[rem + k * pos]))   # a hit is J of the walk's steps
                else:
                    misses += 1
                    dead = True
                    assert Ri[rem + k * (pos + J)] <= Li[rem + k * (pos + J)]          # a miss: empty J steps on
                continue
            nsteps += 1
            pos += 1
            L, R = int(Li[rem + k * pos]), int(Ri[rem + k * pos])
        out["steps"][i], out["skip_hits"][i], out["skip_misses"][i] = nsteps, hits, misses
        out["L"][i], out["R"][i] = L, R
    return out


def classes(mod, k, st, m):
    """Boolean masks of the event classes the tests count, from a model's fields
    alone; st: the settings the batch ran under (jump_min, lines, cls), m: its
    read length."""
    jump_min = st["jump_min"]
    rule = st["jump"] and st["lines"] == 1 and st["cls"] == 4     # the lines' grouped form is asked for
    tried = mod["jump_tried"] == 1
    took = tried & (mod["jump_outcome"] == TAKEN)
    lookups = mod["skip_hits"] + mod["skip_misses"]
    return {
        "taken_line": took & (mod["jump_line"] == 1),
        "taken_flat": took & (mod["jump_line"] == 0),
        "refused": tried & (mod["jump_outcome"] == REFUSED),
        "differed": tried & (mod["jump_outcome"] == DIFFERED),
        "skip_hit": mod["skip_hits"] > 0,
        "skip_miss": mod["skip_misses"] > 0,
        "at_jump_min": tried & (mod["jump_nb"] == jump_min),
        "below_jump_min": ~tried & (mod["row1_left"] == jump_min - k) & bool(st["jump"]),
        "skip_last": mod["skip_last"] > 0,
        "rule_kept": (mod["jump_split"] & GROUPED != 0) & (rule and m >= MAX_M_GROUPED - 1),
        "rule_dropped": (mod["jump_split"] == SPLIT4) & (rule and m > MAX_M_GROUPED),
        "window_W": tried & (mod["jump_nb"] == W_LINE),
        "window_W_plus_K": tried & (mod["jump_nb"] == W_LINE + k),
        "no_jump": ~tried,
        "steps_only": ~tried & (lookups == 0),
        "jump_start": mod["start_steps"] > 0,
        "jump_start_exact": (mod["start_steps"] > 0) & (mod["start_steps"] == m // k),   # the table's steps are all the read has
        "no_jump_start": mod["start_steps"] == 0,
    }
