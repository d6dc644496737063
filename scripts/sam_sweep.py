#!/usr/bin/env python3
"""What the SAM lines cost behind seeds, align and paths (dev tool; not the
bench contract).

At the bench's shape (3 Gbase text, 10M x 100 bp reads, task-mid, auto tables),
legs alternating in one session after a warm-up.  A leg is a kfmi_search_seeds,
a kfmi_align_seeds and a kfmi_align_paths at band 3, and on the handles they
leave a kfmi_sam_lines in each form of its write pass -- the wave's LDS tile
and the plain lane-per-line write (kfmi_set_sam_form) -- by turns:

  exact reads (S = 1, max_occ = 1); one substituted base per read; one 1-base
  indel per read; the indel reads on both strands (S = 4, max_occ = 8); exact
  reads of 150 and of 256 bases (S = 1, max_occ = 1).

The text is cut into 24 contigs of equal length, without gaps.  One JSON line
per leg: every repeat's ms of the length pass, the scan and the write pass in
both forms, the medians, the bytes and the write pass's bytes per second, the
paths kernel's time on the same handles, and kfmi_sam_lines_cpu at --threads
threads on the same records, once.  After the timed region the first --check
lines of every leg are compared with the host form's.

  python scripts/sam_sweep.py --out profiles/r27/sam_r27.jsonl
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
from align_sweep import with_indel  # noqa: E402
from seed_sweep import substituted  # noqa: E402

FORMS = ("tile", "lane")


def log(*a):
    print(f"[sam {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--band", type=int, default=3)
    p.add_argument("--max-edits", type=int, default=3)
    p.add_argument("--entries", type=int, default=4, help="cigar_entries: 2 * entries runs per task")
    p.add_argument("--check", type=int, default=100_000, help="lines compared with the host form per leg")
    p.add_argument("--threads", type=int, default=16, help="threads of the host form beside each leg (0: skip it)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    log("text ready; building the index on the device")
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    n_text = int(idx.header()["bwtsize"]) - 1
    per = n_text // 24
    ct = K.Contigs.create(["chr%d" % (i + 1) for i in range(24)], [i * per for i in range(24)],
                          [per if i < 23 else n_text - 23 * per for i in range(24)])
    reads = {}
    for m in (100, 150, 256):
        starts = synth.read_starts(len(text), a.queries, m, 10 + m)
        reads["exact%d" % m] = synth.gather_reads(text, starts, m)
        if m == 100:
            reads["sub1"] = substituted(reads["exact100"], 1, 11)
            reads["indel"] = with_indel(text, np.minimum(np.asarray(starts), n_text - m - 1), m, 12)
    n, C = a.queries, a.entries
    log(f"inputs ready: {n} reads per set")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "backend": a.backend, "text_bases": n_text, "band": a.band, "max_edits": a.max_edits,
                       "cigar_entries": C, "contigs": 24},
             "steps": a.steps, "warmup": a.warmup, "check_lines": min(a.check, n), "host_threads": a.threads}]
    Q = {name: K.Queries.from_array(r) for name, r in reads.items()}
    for q in Q.values():
        K.transfer_to_gpu(idx, q, None)
    legs = {"exact, S=1, occ=1": ("exact100", 1, K.STRAND_FWD, 1),
            "one substitution, S=4, occ=8": ("sub1", 4, K.STRAND_FWD, 8),
            "one indel, S=4, occ=8": ("indel", 4, K.STRAND_FWD, 8),
            "one indel, S=4, occ=8, both strands": ("indel", 4, K.STRAND_BOTH, 8),
            "150 bases, exact, S=1, occ=1": ("exact150", 1, K.STRAND_FWD, 1),
            "256 bases, exact, S=1, occ=1": ("exact256", 1, K.STRAND_FWD, 1)}
    shared = {}
    for leg, (name, s, strands, occ) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        if (s, ns) not in shared:
            shared[(s, ns)] = hs = tuple(K.Results.alloc(x) for x in (s * ns * n, s * ns * n, ns * n, ns * n, C * ns * n))
            for h in hs:
                K.transfer_to_gpu(idx, None, h)
    keys = ["paths"] + [f"{f}_{part}" for f in FORMS for part in ("length", "scan", "write", "call_wall")]
    ms = {leg: {k: [] for k in keys} for leg in legs}
    size = {}

    def run(leg, out=None):
        name, s, strands, occ = legs[leg]
        ns = 2 if strands == K.STRAND_BOTH else 1
        iv, sp, hits, paths, cig = shared[(s, ns)]
        K.search_seeds(idx, Q[name], iv, sp, s, strands)
        K.align_seeds(idx, Q[name], iv, sp, hits, s, strands, occ, a.band, a.max_edits)
        K.align_paths(idx, Q[name], hits, paths, cig, strands, a.band, a.max_edits, C)
        pa = K.last_timing()["lf_ms"]
        if out is not None:
            out["paths"].append(pa)
        for form, f in enumerate(FORMS):
            K.set_sam_form(form)
            t0 = time.perf_counter()
            sam = K.sam_lines(idx, Q[name], ct, hits, paths, cig, None, strands, C, a.band)
            wall = 1e3 * (time.perf_counter() - t0)
            parts = K.sam_last_passes()
            size[leg] = sam.nbytes
            sam.close()
            if out is not None:
                for part, v in zip(("length", "scan", "write"), parts):
                    out[f"{f}_{part}"].append(v)
                out[f"{f}_call_wall"].append(wall)
        K.set_sam_form(0)

    for it in range(a.warmup + a.steps):
        for leg in legs:
            run(leg, ms[leg] if it >= a.warmup else None)
    log("timed region done; checking")
    for leg, (name, s, strands, occ) in legs.items():
        ns = 2 if strands == K.STRAND_BOTH else 1
        iv, sp, hits, paths, cig = shared[(s, ns)]
        run(leg)
        for h in (hits, paths, cig):
            K.transfer_to_cpu(h)
        med = {k: statistics.median(v) for k, v in ms[leg].items()}
        row = {"leg": leg, "unit": "ms", "reads": n, "tasks": ns * n, "bytes": size[leg]}
        for k, v in ms[leg].items():
            row[k] = [round(x, 3) for x in v]
            row[k + "_median"] = round(med[k], 3)
        for f in FORMS:
            row[f + "_write_GBps"] = round(size[leg] / med[f + "_write"] / 1e6, 1) if med[f + "_write"] else None
            row[f + "_total_median"] = round(med[f + "_length"] + med[f + "_scan"] + med[f + "_write"], 3)
        row["tile_over_lane_write"] = round(med["tile_write"] / med["lane_write"], 3) if med["lane_write"] else None
        row["sam_over_paths"] = round(row["tile_total_median"] / med["paths"], 3) if med["paths"] else None
        if a.threads:
            t0 = time.perf_counter()
            ref = K.sam_lines_cpu(text, Q[name], ct, hits, paths, cig, None, strands, C, a.band, nthreads=a.threads)
            row["host_form_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            row["host_bytes_equal"] = ref.nbytes == size[leg]
            ref.close()
        # the first lines again as a batch of their own, on both sides
        c = min(a.check, n)
        qc = K.Queries.from_array(np.ascontiguousarray(reads[name][:c]))
        hc = [K.Results.alloc(ns * c), K.Results.alloc(ns * c), K.Results.alloc(C * ns * c)]
        try:
            K.transfer_to_gpu(idx, qc, hc[0])
            for h in hc[1:]:
                K.transfer_to_gpu(idx, None, h)
            for h, big, k in zip(hc, (hits, paths, cig), (1, 1, C)):
                h.array()[:] = big.array()[:2 * k * ns * c]
                K.results_to_gpu(h)
            same = True
            for form in range(len(FORMS)):
                K.set_sam_form(form)
                got = K.sam_lines(idx, qc, ct, hc[0], hc[1], hc[2], None, strands, C, a.band)
                ref = K.sam_lines_cpu(text, qc, ct, hc[0], hc[1], hc[2], None, strands, C, a.band)
                same = same and got.text() == ref.text() and np.array_equal(got.offsets(), ref.offsets())
                mapped = sum(1 for ln in ref.lines()[:1000] if ln.split(b"\t")[1] != b"4")
                got.close()
                ref.close()
            K.set_sam_form(0)
            row["host_equal_on_sample"] = bool(same)
            row["mapped_of_first_1000"] = mapped
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
