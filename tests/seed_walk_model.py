"""A host model of seed_walk's decisions (csrc/hip/kfmi_kernels.h), task by
task: which rounds are ordinary K-steps, which look up the jump-start table
and whether the entry is empty, which look up the skip table and whether it
matches, which units do not occur on their own and how many records the task
stores.  Like walk_model.py it is built from brute force -- walk_model.World's
suffix array, its inverse and the textbook one-base backward step -- and takes
from the library only the numbers the caller passes in: K, the jump start's
step count (ftab_auto_bases // K, 0 = no table; the remainder table replaces it
when m % K != 0), whether a skip table is there (J = 16 // K steps each) and S.

The fields it returns are the ones kstep_fmi.decode_seed_trace names, plus the
intervals and spans of the records ([T, S, 2], unused slots zero).

expected_form() is the fetch form launch_seeds and launch_task pick per
geometry, table-size class and code registers: the table of
test_fetch_forms.py's docstring as a function, and expected_launch() the rest of
a record's word 3.  expected_forward_launch() is the same for the forward search,
whose records carry no launch identity: the launch plan's rules (DESIGN.md
"launch plan") written out again, for tests/test_launch_plan.py to hold the
library's own plan to.
"""
import numpy as np

FIELDS = ("steps", "skip_hits", "skip_misses", "start_hits", "start_empty", "lone_units", "records")
ACGT = np.frombuffer(b"ACGT", np.uint8)
FWD, REV, BOTH = 1, 2, 3
SEED_KERNEL, SEED_STRANDS_KERNEL, SEED_WORDS_KERNEL, TASK_STRANDS_KERNEL, TASK_WORDS_SKIP_KERNEL = range(5)
TASK_FUSED_KERNEL, TASK_TABLES_KERNEL, TASK_JUMP_KERNEL, TASK_WORDS_KERNEL, COOP_KERNEL = range(5, 10)
PACK_NONE, PACK_FORWARD, PACK_STRANDS_ASCII, PACK_STRANDS_WORDS = range(4)


def play(world, k, tasks, ftab_steps=0, skip=False, s=8):
    """The seed walk of every task (uint8 [T, m], bases ACGT) under the tables
    in effect."""
    tasks = np.asarray(tasks, dtype=np.uint8)
    T, m = tasks.shape
    codes = np.searchsorted(ACGT, tasks)
    assert (ACGT[codes] == tasks).all()
    codes = codes.tolist()
    occ = [row.tolist() for row in world.occ]
    first = [int(x) for x in world.first]
    sa, isa, text = world.sa.tolist(), world.isa.tolist(), np.searchsorted(ACGT, world.text).tolist()
    rows = world.n + 1
    rem = m % k
    mk = m - rem
    steps = mk // k
    F = 0 if rem else int(ftab_steps)          # the remainder table is not combined with the jump start
    J = 16 // k
    out = {f: np.zeros(T, dtype=np.int64) for f in FIELDS}
    iv, sp = np.zeros((T, s, 2), dtype=np.uint32), np.zeros((T, s, 2), dtype=np.uint32)

    def extend(L, R, p, hi, lo):
        """[L, R) of x -> of p[lo:hi] + x, one base at a time from p[hi - 1] down."""
        for j in range(hi - 1, lo - 1, -1):
            c = p[j]
            L, R = first[c] + occ[c][L], first[c] + occ[c][R]
        return L, R

    for t in range(T):
        p = codes[t]
        L, R, e = 0, rows, mk
        n_steps = hits = misses = s_hit = s_empty = lone = 0
        if rem:
            l, r = extend(0, rows, p, m, mk)
            if r > l:
                L, R, e = l, r, m
            else:
                lone = 1                                         # the remainder unit does not occur: no lookup, no step
        pos = cnt = 0
        dead = False
        while pos < steps and cnt < s:
            b = mk - k * pos
            fresh = e == b
            if not dead and fresh and F and pos + F <= steps:
                l, r = extend(0, rows, p, b, b - F * k)          # the table's entry: the true interval
                if r > l:
                    L, R, pos, s_hit = l, r, pos + F, s_hit + 1
                else:
                    dead, s_empty = True, s_empty + 1
                continue
            if skip and not dead and not fresh and R == L + 1 and pos + J <= steps:
                q = sa[L]
                if q >= 16 and text[q - 16:q] == p[b - 16:b]:
                    L = isa[q - 16]
                    R, pos, hits = L + 1, pos + J, hits + 1
                else:
                    dead, misses = True, misses + 1
                continue
            n_steps += 1
            l, r = extend(L, R, p, b, b - k)
            if r <= l:
                if fresh:                                        # the unit alone does not occur: past it, no record
                    pos, e, lone = pos + 1, b - k, lone + 1
                else:
                    iv[t, cnt], sp[t, cnt] = (L, R), (b, e - b)
                    cnt, e = cnt + 1, b
                L, R, dead = 0, rows, False
            else:
                L, R, pos = l, r, pos + 1
        b = mk - k * pos
        if cnt < s and e != b:
            iv[t, cnt], sp[t, cnt] = (L, R), (b, e - b)
            cnt += 1
        for f, v in zip(FIELDS, (n_steps, hits, misses, s_hit, s_empty, lone, cnt)):
            out[f][t] = v
    out["intervals"], out["spans"] = iv, sp
    return out


def classes(mod, m):
    """Boolean masks of the task classes the tests count, from a model's fields alone."""
    sp = mod["spans"].astype(np.int64)
    return {
        "start_hit": mod["start_hits"] > 0,
        "start_empty": mod["start_empty"] > 0,
        "skip_hit": mod["skip_hits"] > 0,
        "skip_miss": mod["skip_misses"] > 0,
        "three_records": mod["records"] >= 3,
        "one_whole": (mod["records"] == 1) & (sp[:, 0, 0] == 0) & (sp[:, 0, 1] == m),
        "lone_unit": mod["lone_units"] > 0,
    }


LOOKUPS = ("start_hit", "start_empty", "skip_hit", "skip_miss")
D_ALL = (32, 64, 128, 192, 256, 448, 960)                       # every d the kernels are built for, K = 1 and 2
GEOMETRIES = [(k, d) for k in (1, 2) for d in D_ALL]


def bitmap_words(k, d):
    return 2 * k * d // 32


ASM = {g for g in GEOMETRIES if bitmap_words(*g) == 8}                        # the asm fetch: forms 8 / 7
SMALL = {g for g in GEOMETRIES if bitmap_words(*g) <= 16} - ASM               # one line per block, the C++ fetch: 1 / 4
STREAM = set(GEOMETRIES) - ASM - SMALL                                        # lf_stream whatever the form: 1
assert ASM == {(2, 64), (1, 128)} and {(1, 64), (1, 32), (2, 128)} <= SMALL and (2, 192) in STREAM


def expected_form(layout, k, d, cls, maxw):
    """The SPLIT template value of the seed or strand kernel launched for this
    geometry at table-size class cls (0 = by size: 1 on a small index) with
    maxw code registers (0: the plain walk of packed words)."""
    assert layout in ("task-mid", "task") and cls in (0, 1, 2, 4) and maxw in (0, 8, 16), (layout, cls, maxw)
    cls = cls or 1
    if (k, d) in ASM:
        return 8 if cls == 1 else 7
    if (k, d) in SMALL:
        return 4 if cls == 4 or (cls == 2 and maxw == 8) else 1
    assert (k, d) in STREAM, (k, d)
    return 1


def registers(k, m):
    """Code registers of a task of m bases: 8 up to 128 bases in K-steps, else 16."""
    return 8 if m - m % k <= 128 else 16


def expected_launch(layout, k, d, cls, m, strands, fused, ftab_steps, skip, seeds=True, folded=False):
    """The fields of a record's word 3 (kstep_fmi.decode_launch_id), or None
    where the strand search runs the plain walk of packed words, which has no
    traced form."""
    maxw = registers(k, m)
    in_kernel = fused and (strands == FWD or m % k == 0)         # the strand staging packs whole K-steps only
    if seeds:
        kernel = (SEED_KERNEL if strands == FWD else SEED_STRANDS_KERNEL) if in_kernel else SEED_WORDS_KERNEL
    else:
        assert strands in (REV, BOTH)
        if not in_kernel and not skip:
            return None
        kernel = TASK_STRANDS_KERNEL if in_kernel else TASK_WORDS_SKIP_KERNEL
    steps = 0 if m % k else ftab_steps
    return {"form": expected_form(layout, k, d, cls, maxw), "maxw": maxw, "kernel": kernel,
            "skip_split": (cls or 1) if skip else 1, "ftab_folded": int(bool(folded and steps)), "ftab_steps": steps}


def expected_forward_launch(layout, k, d, cls, m, fused, ascii, skip, jump, traced=False):
    """The launch plan of kfmi_search (kstep_fmi.launch_plan's fields), or the
    code the traced call is refused with.  The kernel packs the ASCII rows
    itself up to 256 bases in K-steps under the fused knob; everything else
    walks packed words plainly -- the pack launch's, or the host's -- whatever
    the tables in effect, and has no traced form."""
    bases = m - m % k
    maxw = (8 if bases <= 128 else 16 if bases <= 256 else 0) if fused and ascii else 0
    if traced and not maxw:
        return 19                                                # KFMI_E_NOT_IMPLEMENTED
    if not maxw:
        kernel = TASK_WORDS_KERNEL
    elif jump:
        kernel = TASK_JUMP_KERNEL
    else:
        kernel = TASK_TABLES_KERNEL if skip or traced else TASK_FUSED_KERNEL
    return {"form": expected_form(layout, k, d, cls, maxw), "maxw": maxw, "words_maxw": 0,
            "pack": PACK_FORWARD if ascii and not maxw else PACK_NONE, "kernel": kernel}
