#!/usr/bin/env python3
"""What the paired-end steps cost behind seeds and align (dev tool; not the
bench contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads = 5M pairs, task-mid,
auto tables), fragments uniform in 300 .. 500, legs alternating in one session
after a warm-up.  A leg is a kfmi_search_seeds and a kfmi_align_seeds (S = 4,
max_occ = 8, band 3, max_edits 3) on both strands, then kfmi_mate_windows,
kfmi_place_windows (max_edits 8) and kfmi_pair_hits on the records that leaves:

  (a) exact pairs, mode 0: nothing should be rescued, so the window kernel's
      time is its floor (staging the reads, one window record per task);
  (b) the second mate of every pair carries six spread substitutions: the
      align step's bound refuses it, and every such mate is rescued;
  (c) the reads of (b) in mode 1;
  (d) exact pairs of 150 bases, modes 0 and 1.

One JSON line per leg: every repeat's ms of the align, mate-window, window and
pair kernels, their medians and ranges, the windows that were not empty, the
window kernel's ns per scanned column and word, the pairs PROPER and RESCUED.
After the timed region the first --check records of every leg are recomputed
by the three host forms on the device's own hits.

  python scripts/pair_sweep.py --out profiles/r23/pairs_r23.jsonl
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

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def log(*a):
    print(f"[pairs {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def pairs(text: bytes, count: int, m: int, lo: int, hi: int, seed: int, subs: int = 0) -> np.ndarray:
    """2 * count interleaved reads: read 2p the fragment's first m bases, read 2p + 1 the reverse complement of its
    last m; `subs` evenly spread bases of every second mate get another base."""
    rng = np.random.default_rng(seed)
    frag = rng.integers(lo, hi + 1, size=count)
    start = rng.integers(0, len(text) - hi - 1, size=count)
    first = synth.gather_reads(text, start, m)
    second = synth.gather_reads(text, start + frag - m, m)
    if subs:
        at = (np.arange(subs) * m) // subs + m // (2 * subs)
        second[:, at] = ACGT[(np.searchsorted(ACGT, second[:, at]) + rng.integers(1, 4, size=(count, subs))) % 4]
    out = np.empty((2 * count, m), np.uint8)
    out[0::2] = first
    out[1::2] = COMP[second[:, ::-1]]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--band", type=int, default=3)
    p.add_argument("--max-edits", type=int, default=3, help="the align step's bound")
    p.add_argument("--window-edits", type=int, default=8, help="kfmi_place_windows' bound")
    p.add_argument("--min-frag", type=int, default=300)
    p.add_argument("--max-frag", type=int, default=500)
    p.add_argument("--check", type=int, default=100_000, help="records recomputed on the host per leg")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    log("text ready; building the index on the device")
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    n_text = int(idx.header()["bwtsize"]) - 1
    n, S, OCC = a.queries, 4, 8
    lo, hi = a.min_frag, a.max_frag
    reads = {"exact100": pairs(text, n // 2, 100, lo, hi, 21), "subs100": pairs(text, n // 2, 100, lo, hi, 22, subs=6),
             "exact150": pairs(text, n // 2, 150, lo, hi, 23)}
    log(f"inputs ready: {n} reads per set")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "pairs": n // 2, "backend": a.backend, "text_bases": n_text, "band": a.band,
                       "max_edits": a.max_edits, "window_edits": a.window_edits, "min_frag": lo, "max_frag": hi,
                       "max_seeds": S, "max_occ": OCC},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes(), "jump_bytes": idx.jump_bytes()},
             "steps": a.steps, "warmup": a.warmup, "check_records": min(a.check, 2 * n)}]
    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    for q in Q.values():
        K.transfer_to_gpu(idx, q, None)
    legs = {"(a) exact pairs, mode 0": ("exact100", 0), "(b) six substitutions in one mate, mode 0": ("subs100", 0),
            "(c) six substitutions in one mate, mode 1": ("subs100", 1), "(d) 150 bases, exact, mode 0": ("exact150", 0),
            "(d) 150 bases, exact, mode 1": ("exact150", 1)}
    iv, sp = K.Results.alloc(S * 2 * n), K.Results.alloc(S * 2 * n)
    hits, win, resc, paired = (K.Results.alloc(2 * n) for _ in range(4))
    for h in (iv, sp, hits, win, resc, paired):
        K.transfer_to_gpu(idx, None, h)
    fields = ("align", "mate_windows", "window", "pair")
    ms = {leg: {f: [] for f in fields} for leg in legs}

    def run(leg, out=None):
        name, mode = legs[leg]
        m = reads[name].shape[1]
        t = {}
        K.search_seeds(idx, Q[name], iv, sp, S, K.STRAND_BOTH)
        K.align_seeds(idx, Q[name], iv, sp, hits, S, K.STRAND_BOTH, OCC, a.band, a.max_edits)
        t["align"] = K.last_timing()["lf_ms"]
        K.mate_windows(idx, hits, win, m, lo, hi, mode)
        t["mate_windows"] = K.last_timing()["lf_ms"]
        K.place_windows(idx, Q[name], win, resc, K.STRAND_BOTH, a.window_edits)
        t["window"] = K.last_timing()["lf_ms"]
        K.pair_hits(idx, hits, resc, paired, m, lo, hi)
        t["pair"] = K.last_timing()["lf_ms"]
        if out is not None:
            for f in fields:
                out[f].append(t[f])

    for it in range(a.warmup + a.steps):
        for leg in legs:
            run(leg, ms[leg] if it >= a.warmup else None)
    log("timed region done; counting and checking")
    for leg, (name, mode) in legs.items():
        m = reads[name].shape[1]
        run(leg)
        for h in (hits, win, resc, paired):
            K.transfer_to_cpu(h)
        w = win.array().reshape(-1, 2)
        some = w[:, 1] > 0
        begin, edits, multi, proper, rescued = K.decode_pairs(paired.array())
        row = {"leg": leg, "unit": "ms", "tasks": 2 * n, "read_len": m}
        for f in fields:
            row[f] = [round(x, 3) for x in ms[leg][f]]
            row[f + "_median"] = round(statistics.median(ms[leg][f]), 3)
            row[f + "_range"] = [round(min(ms[leg][f]), 3), round(max(ms[leg][f]), 3)]
        # columns a task with a window scans: its begin positions, then m + min(max_edits, m) more, less the text's end
        cols = float((w[some, 1].astype(np.int64) + m + min(a.window_edits, m)).sum())
        words = (m + 31) // 32
        row.update({"windows": int(some.sum()), "mean_window": round(float(w[some, 1].mean()), 2) if some.any() else None,
                    "window_ns_per_column_and_word": round(1e6 * row["window_median"] / (cols * words), 6) if cols else None,
                    "align_ns_per_task": round(1e6 * row["align_median"] / (2 * n), 4),
                    "window_ns_per_window": round(1e6 * row["window_median"] / int(some.sum()), 4) if some.any() else None,
                    "reads_proper": int(proper.sum()), "reads_rescued": int(rescued.sum()),
                    "reads_placed": int((begin >= 0).sum())})
        c = min(a.check, 2 * n) // 4 * 4
        qc = K.Queries.from_array(np.ascontiguousarray(reads[name][:c // 2]))
        hc = [K.Results.alloc(c) for _ in range(4)]
        try:
            hc[0].array()[:] = hits.array()[:2 * c]
            K.mate_windows_cpu(n_text, hc[0], hc[1], m, lo, hi, mode)
            K.place_windows_cpu(text, qc, hc[1], hc[2], K.STRAND_BOTH, a.window_edits)
            K.pair_hits_cpu(hc[0], hc[2], hc[3], m, lo, hi)
            row["host_equal_on_sample"] = bool(np.array_equal(hc[1].array(), win.array()[:2 * c]) and
                                               np.array_equal(hc[2].array(), resc.array()[:2 * c]) and
                                               np.array_equal(hc[3].array(), paired.array()[:2 * c]))
        finally:
            qc.close()
            for h in hc:
                h.close()
        rows.append(row)
        log(json.dumps(row))
    text_out = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text_out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
