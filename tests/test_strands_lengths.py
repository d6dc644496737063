"""Strand searches on the device, densely: every read length from 1 to 272
(every m % 16 and m % K on both sides of the 8- and 16-register forms, reads
shorter than the jump-start table and than one skip-table lookup) and the long
lengths of test_length_sweep.py (the strand pack's halved tiles above 512 bases
and its in-place form above 1,024), through every device path that makes a
reverse strand's code words -- the fused strand kernel, the whole-row and the
general strand pack, the packed-word kernel (host-packed uploads and stream
chunks) -- and the batch edges the BOTH staging depends on (32 reads per wave,
two lanes per LDS row, 16 or 32 rows per staging round).

Reference: the CPU oracle (fmIndexCPUBaseline.c:157-292 restated, pinned by the
golden files) on the K = 1 index of the same text, of the read for the forward
interval and of revcomp_def(read) -- the numpy definition in strand_reads.py,
not the library's reverse complement -- for the reverse one.  The AltCounters
backend is held to the AltCounters restatement on its own image.  Every
comparison is bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from skip_texts import ACGT
from strand_reads import revcomp_def, strand_reads

pytestmark = pytest.mark.gpu

SHORT = tuple(range(1, 273))
LONG = tuple(sorted({300, 511, 512, 513, 1020, 1023, 1024, 1025, 1026, 1040, 1056, 2047, 2048, 2064, 4095, 4096, 4128}
                    | {int(x) for x in np.random.default_rng(4243).integers(273, 5000, size=4)}))
LENGTHS = SHORT + LONG
N_SHORT, N_LONG = 192, 80
EDGE_LENGTHS = (100, 101, 129, 250)          # stage_rows 32, 32, 16, 16; even and odd
EDGE_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513)
EDGE_READS = 513


def sweep_text() -> np.ndarray:
    """20,011 random bases ((n + 1) % 64 != 0) with two copied segments, so some
    intervals stay wide deep into a read, and 400 bases that are the reverse
    complement of 400 others, so some reads match on both strands at once."""
    rng = np.random.default_rng(2027)
    t = ACGT[rng.integers(0, 4, size=20_011)].copy()
    t[9_000:10_500] = t[2_000:3_500]
    t[15_000:15_800] = t[6_000:6_800]
    t[12_000:12_400] = revcomp_def(t[None, 4_000:4_400])[0]
    return t


def sweep_reads(t: np.ndarray, m: int) -> np.ndarray:
    """strand_reads, then the read that ends the text, the one that starts it
    and the reverse complement of each."""
    q = strand_reads(t, m, seed=1_000 + m, n_reads=N_SHORT if m <= SHORT[-1] else N_LONG)
    ends = np.stack([t[t.size - m:], t[:m]])
    return np.ascontiguousarray(np.concatenate([q, ends, revcomp_def(ends)]))


def interleave(fwd: np.ndarray, rev: np.ndarray) -> np.ndarray:
    both = np.empty((fwd.size // 2 * 2, 2), np.uint32)
    both[0::2], both[1::2] = fwd.reshape(-1, 2), rev.reshape(-1, 2)
    return both.ravel()


def nonempty(res: np.ndarray) -> np.ndarray:
    return res[1::2] > res[0::2]


def reference(search, t: np.ndarray, lengths) -> dict:
    """m -> (reads, forward, reverse, both) with search(reads) the reference's
    intervals.  Not vacuous: at every length a quarter of the reads at least has
    a non-empty interval on each strand (the clean text windows of either half
    of strand_reads alone are more than that), and some reads of 32 bases and
    more have one on both strands at once.  The arrays are read-only."""
    cases, twice = {}, 0
    for m in lengths:
        q = sweep_reads(t, m)
        fwd, rev = search(q), search(revcomp_def(q))
        for what, w in (("forward", fwd), ("reverse", rev)):
            assert w.shape == (2 * q.shape[0],)
            assert 4 * np.count_nonzero(nonempty(w)) >= q.shape[0], (m, what, int(np.count_nonzero(nonempty(w))))
        if m >= 32:
            twice += int(np.count_nonzero(nonempty(fwd) & nonempty(rev)))
        cases[m] = (q, fwd, rev, interleave(fwd, rev))
        for a in cases[m]:
            a.setflags(write=False)
    assert twice > 0 or max(lengths) < 32
    return cases


def defaults(K):
    K.set_devices([])
    K.set_split_class(0)
    K.set_fused(True)
    K.set_ftab_budget(None)
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.fixture(scope="module")
def sweep(kfmi_mod, oracle_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    K.set_device(0)
    K.set_devices([])
    t = sweep_text()
    idx = {k: K.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2, 3, 4)}
    img1 = idx[1].image()
    cases = reference(lambda q: oracle_mod.search(img1, q)[0], t, LENGTHS)
    yield K, t, idx, cases
    defaults(K)
    for i in idx.values():
        i.close()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, "first differing interval", int(np.flatnonzero(got != want)[0]) // 2)


def fresh_upload(K, idx, backend):
    """The index on the device again under the settings in effect: its tables are built here."""
    K.set_backend(backend)
    idx.free_gpu()
    K.transfer_to_gpu(idx, None, None)


def check_lengths(K, idx, backend, cases, what):
    for m, (q, _, rev, both) in cases.items():
        same(K.search_array(idx, q, backend, strands=K.STRAND_REV), rev, (what, m, "REV"))
        same(K.search_array(idx, q, backend, strands=K.STRAND_BOTH), both, (what, m, "BOTH"))


@pytest.mark.parametrize("tables", ["auto", "walk"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "packed-first"])
@pytest.mark.parametrize("k", [1, 2])
def test_task_mid_every_length(sweep, k, fused, tables):
    """task-mid at K = 1, 2.  Fused: task_strands_kernel<8 | 16> for m <= 256
    with m % K == 0, the strand pack otherwise.  Not fused: the whole-row pack
    for m <= 256 with m % K == 0, the general pack otherwise, then the walk on
    packed words (with the skip table: task_words_skip_kernel)."""
    K, _, idx, cases = sweep
    try:
        defaults(K)
        fresh_upload(K, idx[k], "task-mid")
        K.set_fused(fused)
        if tables == "walk":
            K.set_ftab(0)
            K.set_skip(0)
        check_lengths(K, idx[k], "task-mid", cases, ("task-mid", k, fused, tables))
        if tables == "auto":
            assert idx[k].skip_bytes() != 0              # the auto tables are on the device
            assert idx[k].ftab_bytes() != 0
    finally:
        defaults(K)


def test_coop_mid_every_length(sweep):
    K, _, idx, cases = sweep
    try:
        defaults(K)
        fresh_upload(K, idx[2], "coop-mid")
        check_lengths(K, idx[2], "coop-mid", cases, "coop-mid")
    finally:
        defaults(K)


def test_alt_counters_every_length(sweep, oracle_mod):
    """task-ac-mid at K = 2 against the AltCounters restatement on the index's
    own AltCounters image; m % K != 0 is refused with code 33, never answered."""
    K, _, idx, cases = sweep
    acs = idx[2].alt_counters()
    img = acs[0].image().copy()
    for a in acs:
        a.close()
    try:
        defaults(K)
        fresh_upload(K, idx[2], "task-ac-mid")
        for m, (q, _, _, _) in cases.items():
            if m % 2:
                for strands in (K.STRAND_REV, K.STRAND_BOTH):
                    with pytest.raises(K.KfmiError) as e:
                        K.search_array(idx[2], q, "task-ac-mid", strands=strands)
                    assert e.value.code == 33, (m, strands)
                continue
            fwd, rev = oracle_mod.search(img, q)[0], oracle_mod.search(img, revcomp_def(q))[0]
            assert 4 * min(np.count_nonzero(nonempty(fwd)), np.count_nonzero(nonempty(rev))) >= q.shape[0], m
            same(K.search_array(idx[2], q, "task-ac-mid", strands=K.STRAND_REV), rev, (m, "REV"))
            same(K.search_array(idx[2], q, "task-ac-mid", strands=K.STRAND_BOTH), interleave(fwd, rev), (m, "BOTH"))
    finally:
        defaults(K)


@pytest.mark.parametrize("backend,k", [("coop-grp", 3), ("task-grp", 4)])
def test_grouped_every_length(sweep, backend, k):
    """pack_strands_kernel<3>, <4>: every remainder m % K, whole tiles staged,
    halved tiles above 512 bases, rows read in place above 1,024."""
    K, _, idx, cases = sweep
    try:
        defaults(K)
        fresh_upload(K, idx[k], backend)
        check_lengths(K, idx[k], backend, cases, (backend, k))
    finally:
        defaults(K)


@pytest.mark.parametrize("hostpack", ["0", "1"])
@pytest.mark.parametrize("k,backend", [(1, "task-mid"), (2, "task-mid"), (2, "coop"), (3, "coop-grp"),
                                       (4, "task-grp")])
def test_streamed_every_length(sweep, k, backend, hostpack, monkeypatch):
    """kfmi_search_stream_strands in chunks of 32 reads: every chunk as ASCII
    (packed on the device) or as host-packed words (strand_words_kernel; K = 3
    has no host-packed form and goes as ASCII either way)."""
    monkeypatch.setenv("KFMI_STREAM_HOSTPACK", hostpack)
    monkeypatch.delenv("KFMI_STREAM_CHUNK", raising=False)
    K, _, idx, cases = sweep
    try:
        defaults(K)
        fresh_upload(K, idx[k], backend)
        for m, (q, _, rev, both) in cases.items():
            same(K.search_stream(idx[k], q, chunk=32, strands=K.STRAND_REV), rev, (backend, k, hostpack, m, "REV"))
            same(K.search_stream(idx[k], q, chunk=32, strands=K.STRAND_BOTH), both, (backend, k, hostpack, m, "BOTH"))
            if hostpack == "1" and k != 3:
                assert K.load().kfmi_stream_hostpacked_fraction() == 1.0, m
    finally:
        defaults(K)


CHILD = r"""
import json, sys
sys.path[:0] = %(paths)r
import numpy as np
import kstep_fmi as K
K.load(); K.set_device(0); K.set_backend(%(backend)r)
d = dict(np.load(%(data)r))
idx = K.Index.build(d["text"].tobytes(), k=%(k)d, d=64)
forms, bad, at, done = set(), [], 0, 0
for m, n in zip(d["lens"].tolist(), d["nums"].tolist()):
    q = d["reads"][at:at + n * m].reshape(n, m)
    want = {K.STRAND_REV: d["rev"][2 * done:2 * (done + n)], K.STRAND_BOTH: d["both"][4 * done:4 * (done + n)]}
    at += n * m
    done += n
    for strands, w in want.items():
        Q, R = K.Queries.from_array(q), K.Results.alloc(w.size // 2)
        K.transfer_to_gpu(idx, Q, R)
        forms.add(K.upload_form(Q))
        K.search_strands(idx, Q, R, strands)
        K.transfer_to_cpu(R)
        if not np.array_equal(R.array(), w):
            bad.append([m, strands])
        Q.close(); R.close()
print(json.dumps({"forms": sorted(forms), "bad": bad, "lengths": len(d["lens"]), "reads": done}))
"""


@pytest.fixture(scope="module")
def sweep_file(sweep, tmp_path_factory):
    """The sweep's reads and reference intervals, for the child processes."""
    _, t, _, cases = sweep
    fn = tmp_path_factory.mktemp("strands") / "sweep.npz"
    np.savez(fn, text=t, lens=np.array(list(cases), np.int64),
             nums=np.array([c[0].shape[0] for c in cases.values()], np.int64),
             reads=np.concatenate([c[0].ravel() for c in cases.values()]),
             rev=np.concatenate([c[2] for c in cases.values()]),
             both=np.concatenate([c[3] for c in cases.values()]))
    return fn


@pytest.mark.parametrize("k,backend", [(1, "task-mid"), (2, "task-mid"), (3, "coop-grp"), (4, "task-grp")])
def test_host_packed_upload_every_length(sweep, sweep_file, k, backend):
    """KFMI_UPLOAD=packed in a process of its own: no ASCII on the device, every
    task column comes from the forward code words (strand_words_kernel), small
    upload chunks.  The packed form exists for K in {1, 2, 4} (kstep_fmi.h); a
    K = 3 handle goes up as ASCII under the same setting and is answered from
    there -- the library's code-33 refusal of 15-base words is the host
    accessor's (test_strands_host.py), no upload reaches it."""
    _, _, _, cases = sweep
    env = dict(os.environ)
    for v in ("KFMI_UPLOAD", "KFMI_UPLOAD_CHUNK", "KFMI_STREAM_HOSTPACK", "KFMI_STREAM_CHUNK", "KFMI_DEVICES",
              "KFMI_BACKEND", "KFMI_FTAB", "KFMI_SKIP", "KFMI_FUSED"):
        env.pop(v, None)
    env.update({"KFMI_UPLOAD": "packed", "KFMI_UPLOAD_CHUNK": "50"})
    code = CHILD % {"paths": [str(util.REPO), str(util.PKG), str(util.REPO / "tests")], "backend": backend, "k": k,
                    "data": str(sweep_file)}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["lengths"] == len(cases) and out["reads"] == sum(c[0].shape[0] for c in cases.values()), out
    assert out["forms"] == (["ascii"] if k == 3 else ["packed"]), out
    assert out["bad"] == [], out


@pytest.fixture(scope="module")
def edges(sweep, oracle_mod):
    """One batch of 513 reads per edge length; every smaller batch is a prefix
    of it.  strand_reads puts its changed reads first, so the batch is shuffled:
    every prefix of 15 reads and more has matches on either strand, a quarter
    of the reads from 63 up."""
    _, t, idx, _ = sweep
    img1 = idx[1].image()
    out = {}
    for m in EDGE_LENGTHS:
        q = strand_reads(t, m, seed=7_000 + m, n_reads=EDGE_READS + 1)
        q = np.ascontiguousarray(q[np.random.default_rng(m).permutation(q.shape[0])[:EDGE_READS]])
        fwd, rev = oracle_mod.search(img1, q)[0], oracle_mod.search(img1, revcomp_def(q))[0]
        for w in (fwd, rev):
            for num in (s for s in EDGE_SIZES if s >= 15):
                hits = np.count_nonzero(nonempty(w[:2 * num]))
                assert hits >= 2 and (num < 63 or 4 * hits >= num), (m, num, hits)
        out[m] = (q, rev, interleave(fwd, rev))
        for a in out[m]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("m", EDGE_LENGTHS)
@pytest.mark.parametrize("k,fused", [(1, True), (2, True), (2, False)], ids=["k1-fused", "k2-fused", "k2-packed-first"])
def test_batch_edges(sweep, edges, k, fused, m):
    """Batches that end inside a wave, a staging round or a block, on a results
    handle of exactly ns * num intervals; after each, the whole 513-read batch
    again, which a block that wrote past its own batch would have damaged."""
    K, _, idx, _ = sweep
    q, rev, both = edges[m]
    try:
        defaults(K)
        K.set_fused(fused)
        K.set_backend("task-mid")
        for num in EDGE_SIZES:
            for strands, want, per in ((K.STRAND_REV, rev, 2), (K.STRAND_BOTH, both, 4)):
                got = K.search_array(idx[k], np.ascontiguousarray(q[:num]), "task-mid", strands=strands)
                same(got, want[:per * num], (m, num, strands))
                same(K.search_array(idx[k], q, "task-mid", strands=strands), want, (m, num, strands, "whole batch after"))
    finally:
        defaults(K)
