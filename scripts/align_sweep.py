#!/usr/bin/env python3
"""What seed alignment costs behind the seed search (dev tool; not the bench
contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads, task-mid, auto tables),
legs alternating in one session after a warm-up, each a kfmi_search_seeds
followed by a kfmi_align_seeds on its handles:

  (a) exact reads, S = 1, max_occ = 1, at bands 0, 3 and 15, beside
      kfmi_verify_seeds on the same handles;
  (b) one substituted base per read, S = 4, max_occ = 8, band 3;
  (c) one 1-base indel per read (by turns deleted and inserted, anywhere from
      base 1 to m - 2), S = 4, max_occ = 8, band 3: the share of reads placed
      with one edit, beside the share kfmi_verify_seeds places with at most
      three mismatches;
  (d) (c) on both strands;
  then reads of 150 and of 256 bases (the 16-word form), exact, S = 1,
  max_occ = 1, band 3.

One JSON line per leg: every repeat's kernel ms, the median and the spread
(max - min), the candidates scored, the tasks placed and their edits.  After
the timed region the first --check records of every leg are recomputed on the
host (kfmi_align_seeds_cpu on the device's own seed records and the suffix
array read back from the device).

  python scripts/align_sweep.py --out profiles/r20/align_r20.jsonl
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "k-step_fm-index_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import kstep_fmi as K  # noqa: E402
from kstep_fmi import synth  # noqa: E402
from seed_sweep import substituted  # noqa: E402


def log(*a):
    print(f"[align {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def with_indel(text, starts: np.ndarray, m: int, seed: int) -> np.ndarray:
    """Reads of m bases at `starts` with one base deleted (even rows; refilled
    from the text) or one foreign base inserted (odd rows) at a random position in [1, m - 2]."""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
    n = starts.size
    pos = rng.integers(1, m - 1, size=n)
    col = np.arange(m)[None, :]
    dele = (np.arange(n) % 2 == 0)[:, None]
    src = np.where(dele, col + (col >= pos[:, None]), col - (col > pos[:, None]))
    q = t[np.minimum(starts[:, None] + src, t.size - 1)].copy()
    odd = np.flatnonzero(~dele[:, 0])
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    q[odd, pos[odd]] = acgt[(np.searchsorted(acgt, np.minimum(q[odd, pos[odd]] & 0xDF, ord("T"))) + rng.integers(1, 4, size=odd.size)) % 4]
    return np.ascontiguousarray(q)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--max-edits", type=int, default=3)
    p.add_argument("--check", type=int, default=100_000, help="records recomputed on the host per leg")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    n_text = int(idx.header()["bwtsize"]) - 1
    reads = {}
    for m in (100, 150, 256):
        starts = synth.read_starts(len(text), a.queries, m, 10 + m)
        reads["exact%d" % m] = synth.gather_reads(text, starts, m)
        if m == 100:
            reads["sub1"] = substituted(reads["exact100"], 1, 11)
            reads["indel"] = with_indel(text, np.minimum(np.asarray(starts), n_text - m - 1), m, 12)
    n = a.queries
    log(f"inputs ready: {n} reads per set")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "backend": a.backend, "text_bases": n_text, "max_edits": a.max_edits},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes(), "jump_bytes": idx.jump_bytes()},
             "steps": a.steps, "warmup": a.warmup, "check_records": min(a.check, n)}]
    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    for q in Q.values():
        K.transfer_to_gpu(idx, q, None)
    # leg -> (reads, S, strands, max_occ, band; None: kfmi_verify_seeds)
    legs = {"a: exact, S=1, occ=1, verify": ("exact100", 1, K.STRAND_FWD, 1, None),
            "a: exact, S=1, occ=1, band 0": ("exact100", 1, K.STRAND_FWD, 1, 0),
            "a: exact, S=1, occ=1, band 3": ("exact100", 1, K.STRAND_FWD, 1, 3),
            "a: exact, S=1, occ=1, band 15": ("exact100", 1, K.STRAND_FWD, 1, 15),
            "b: one substitution, S=4, occ=8, band 3": ("sub1", 4, K.STRAND_FWD, 8, 3),
            "c: one indel, S=4, occ=8, band 3": ("indel", 4, K.STRAND_FWD, 8, 3),
            "c: one indel, S=4, occ=8, verify": ("indel", 4, K.STRAND_FWD, 8, None),
            "d: one indel, S=4, occ=8, band 3, both strands": ("indel", 4, K.STRAND_BOTH, 8, 3),
            "150 bases, exact, S=1, occ=1, band 3": ("exact150", 1, K.STRAND_FWD, 1, 3),
            "256 bases, exact, S=1, occ=1, band 3": ("exact256", 1, K.STRAND_FWD, 1, 3)}
    ms = {leg: [] for leg in legs}
    shared = {}                                   # (reads, S, strands) -> handles: legs on the same seeds share them
    for leg, (name, s, strands, occ, band) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        if (name, s, strands) not in shared:
            shared[(name, s, strands)] = hs = (K.Results.alloc(s * ns * n), K.Results.alloc(s * ns * n), K.Results.alloc(ns * n))
            for h in hs:
                K.transfer_to_gpu(idx, None, h)

    def run(leg):
        name, s, strands, occ, band = legs[leg]
        iv, sp, hits = shared[(name, s, strands)]
        K.search_seeds(idx, Q[name], iv, sp, s, strands)
        if band is None:
            K.verify_seeds(idx, Q[name], iv, sp, hits, s, strands, occ, a.max_edits)
        else:
            K.align_seeds(idx, Q[name], iv, sp, hits, s, strands, occ, band, a.max_edits)
        return K.last_timing()["lf_ms"]

    for it in range(a.warmup + a.steps):
        for leg in legs:
            t = run(leg)
            if it >= a.warmup:
                ms[leg].append(t)
    log("timed region done; counting and checking")
    sa = idx.jump_tables()[0]
    for leg, (name, s, strands, occ, band) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        iv, sp, hits = shared[(name, s, strands)]
        run(leg)
        for h in (iv, sp, hits):
            K.transfer_to_cpu(h)
        origin, edits, multi, scored = K.decode_hits(hits.array())
        placed = origin >= 0
        med = statistics.median(ms[leg])
        row = {"leg": leg, "unit": "ms", "kernel": [round(x, 3) for x in ms[leg]], "kernel_median": round(med, 3),
               "kernel_spread": round(max(ms[leg]) - min(ms[leg]), 3), "tasks": ns * n,
               "candidates_scored": int(scored.sum()), "tasks_placed": int(placed.sum()), "tasks_multi": int(multi.sum()),
               "share_placed": round(float(placed.mean()), 6),
               "share_placed_with_at_most_1": round(float((placed & (edits <= 1)).mean()), 6),
               "mean_edits_of_placed": round(float(edits[placed].mean()), 4) if placed.any() else None}
        # the first c reads' records once more on the host, from the device's own seed records
        c = min(a.check, n)
        qc = K.Queries.from_array(np.ascontiguousarray(reads[name][:c]))
        hc = [K.Results.alloc(s * ns * c), K.Results.alloc(s * ns * c), K.Results.alloc(ns * c)]
        try:
            hc[0].array()[:] = iv.array()[:2 * s * ns * c]
            hc[1].array()[:] = sp.array()[:2 * s * ns * c]
            if band is None:
                K.verify_seeds_cpu(text, sa, qc, hc[0], hc[1], hc[2], s, strands, occ, a.max_edits)
            else:
                K.align_seeds_cpu(text, sa, qc, hc[0], hc[1], hc[2], s, strands, occ, band, a.max_edits)
            row["host_equal_on_sample"] = bool(np.array_equal(hc[2].array(), hits.array()[:2 * ns * c]))
        finally:
            qc.close()
            for h in hc:
                h.close()
        rows.append(row)
        log(json.dumps(row))
    base = next(r for r in rows if r.get("leg") == "a: exact, S=1, occ=1, verify")["kernel_median"]
    zero = next(r for r in rows if r.get("leg") == "a: exact, S=1, occ=1, band 0")["kernel_median"]
    rows.append({"summary": "band 0 against the verify, leg (a)", "ratio": round(zero / base, 3) if base else None})
    text_out = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text_out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
