#!/usr/bin/env python3
"""Both strands on the device against the host's way of getting them (dev
tool; not the bench contract).

The counterpart is what a caller had to do before kfmi_search_strands: write
the reverse complement of every read on the host and search the 2N reads
q ++ revcomp(q) forward.  Measured at the bench's shape (3 Gbase text, 10M x
100 bp reads, task-mid, auto tables), the two ways alternating in one session
after a warm-up:

  (a) resident  BOTH on N reads  vs  forward on the 2N reads: LF kernel ms and
      total device ms (kfmi_last_timing);
  (b) streamed  BOTH on N reads  vs  forward on the 2N reads: wall ms, from
      pinned and from pageable host memory.

One JSON line per leg: every repeat's figure, the median, the spread (max -
min) of either side, the ratio of the medians, and the md5 of the outputs
(the 2N forward outputs reordered to the BOTH layout must equal them).

  python scripts/strand_sweep.py --out profiles/r09/strand_r9.jsonl
"""
from __future__ import annotations

import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "k-step_fm-index_amd"))
import kstep_fmi as K  # noqa: E402
from kstep_fmi import synth  # noqa: E402


def log(*a):
    print(f"[strands {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def md5(a: np.ndarray) -> str:
    return hashlib.md5(np.ascontiguousarray(a).view(np.uint8)).hexdigest()


def interleave(two_n: np.ndarray) -> np.ndarray:
    """Outputs of the forward search on q ++ revcomp(q) in the BOTH layout."""
    r = two_n.reshape(2, -1, 2)
    return np.ascontiguousarray(r.transpose(1, 0, 2)).ravel()


def summary(leg: str, unit: str, host: list, dev: list, extra: dict) -> dict:
    mh, md = statistics.median(host), statistics.median(dev)
    return {"leg": leg, "unit": unit,
            "host_2n": [round(x, 3) for x in host], "device_both": [round(x, 3) for x in dev],
            "host_2n_median": round(mh, 3), "device_both_median": round(md, 3),
            "host_2n_spread": round(max(host) - min(host), 3), "device_both_spread": round(max(dev) - min(dev), 3),
            "both_over_host": round(md / mh, 4) if mh > 0 else None, **extra}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=10_000_000)
    p.add_argument("--bases", type=int, default=0, help="text length (0: the bench's 3 Gbase text)")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--backend", default="task-mid")
    p.add_argument("--legs", default="resident,pinned,pageable")
    p.add_argument("--out", default="")
    a = p.parse_args()
    K.load()
    K.set_device(0)
    text = synth.text_3g(a.bases or 3_000_000_000)
    idx = K.Index.build(text, k=2, d=64, gpu=True, host_image=False)
    q = synth.gather_reads(text, synth.read_starts(len(text), a.queries, 100, 10), 100)
    n = q.shape[0]
    # every other read from the reverse strand, so that both strands have matches
    q[1::2] = K.revcomp(np.ascontiguousarray(q[1::2]))
    del text
    t = time.perf_counter()
    q2 = np.concatenate([q, K.revcomp(q)])                  # the host's way: revcomp, double the batch
    host_prep_ms = (time.perf_counter() - t) * 1e3
    log(f"inputs ready; host revcomp + concatenate of {n} reads: {host_prep_ms:.1f} ms")
    K.set_backend(a.backend)
    K.transfer_to_gpu(idx, None, None)
    rows = [{"shape": {"reads": n, "m": 100, "backend": a.backend, "text_bases": int(idx.header()["bwtsize"]) - 1},
             "tables": {"ftab_bytes": idx.ftab_bytes(), "skip_bytes": idx.skip_bytes()},
             "host_revcomp_concat_ms": round(host_prep_ms, 1), "steps": a.steps, "warmup": a.warmup}]
    legs = a.legs.split(",")

    if "resident" in legs:
        Q2, R2 = K.Queries.from_array(q2), K.Results.alloc(2 * n)
        Q1, R1 = K.Queries.from_array(q), K.Results.alloc(2 * n)
        K.transfer_to_gpu(idx, Q2, R2)
        K.transfer_to_gpu(idx, Q1, R1)
        lf, tot = ([], []), ([], [])
        for it in range(a.warmup + a.steps):
            for side, call in enumerate((lambda: K.search(idx, Q2, R2),
                                         lambda: K.search_strands(idx, Q1, R1, K.STRAND_BOTH))):
                call()
                if it >= a.warmup:
                    lt = K.last_timing()
                    lf[side].append(lt["lf_ms"])
                    tot[side].append(lt["total_ms"])
        K.transfer_to_cpu(R2)
        K.transfer_to_cpu(R1)
        want, got = interleave(R2.array()), R1.array()
        eq = {"equal": bool(np.array_equal(want, got)), "md5_host_2n_reordered": md5(want), "md5_device_both": md5(got),
              "nonempty_fwd": int(np.count_nonzero(got[1::4] > got[0::4])),
              "nonempty_rev": int(np.count_nonzero(got[3::4] > got[2::4]))}
        rows.append(summary("resident, LF kernel", "ms", lf[0], lf[1], eq))
        rows.append(summary("resident, total (pack + LF)", "ms", tot[0], tot[1], eq))
        for h in (Q2, R2, Q1, R1):
            h.close()

    for mem in ("pinned", "pageable"):
        if mem not in legs:
            continue
        if mem == "pinned":
            in2, in1 = K.pinned_empty(q2.shape, np.uint8), K.pinned_empty(q.shape, np.uint8)
            in2[:], in1[:] = q2, q
            out2, out1 = K.pinned_empty((4 * n,), np.uint32), K.pinned_empty((4 * n,), np.uint32)
        else:
            in2, in1 = q2, q
            out2, out1 = np.empty(4 * n, np.uint32), np.empty(4 * n, np.uint32)
        wall = ([], [])
        for it in range(a.warmup + a.steps):
            for side, call in enumerate((lambda: K.search_stream(idx, in2, out=out2),
                                         lambda: K.search_stream(idx, in1, out=out1, strands=K.STRAND_BOTH))):
                t = time.perf_counter()
                call()
                if it >= a.warmup:
                    wall[side].append((time.perf_counter() - t) * 1e3)
        want = interleave(out2)
        eq = {"equal": bool(np.array_equal(want, out1)), "md5_host_2n_reordered": md5(want),
              "md5_device_both": md5(out1), "host_2n_excludes_host_revcomp_ms": round(host_prep_ms, 1)}
        rows.append(summary(f"streamed, {mem}, wall", "ms", wall[0], wall[1], eq))
        K.load().kfmi_stream_release()
        del in2, in1, out2, out1

    text_out = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text_out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text_out)


if __name__ == "__main__":
    main()
