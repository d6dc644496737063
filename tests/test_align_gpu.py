"""Align seeds on the device (kfmi_align_seeds) against the model of
align_ref.py, bit for bit on both words of every record, and against the host
form as a cross-check (not as the reference).

The seed records the device aligns are the ones kfmi_search_seeds leaves on the
device -- test_seeds_gpu.py pins them to seed_ref.reference, which is what the
model's candidates come from -- or hand-made ones transferred from the host.
The model is computed once per (text, length) for both strands at S = 8,
max_occ = 8 and every band; smaller S and max_occ and the strand modes are cuts
of it (align_ref.records).  The non-vacuity conditions are asserted on the
model alone in align_ref.world, before any device call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as ar
import seed_ref as sr
import util
import verify_ref as vr
from test_align_host import host_hits
from test_verify_gpu import Device as VerifyDevice
from test_verify_gpu import defaults, fresh_upload, same
from test_verify_host import handmade

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
EDGE_SIZES = (1, 63, 64, 65, 257, 513)
GPU_BANDS = (0, 1, 3, 15)


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    w = ar.world(K, oracle_mod)       # the model and its conditions first
    K.set_device(0)
    defaults(K)
    yield K, w
    defaults(K)
    for x in w.values():
        for i in x["idx"].values():
            i.free_gpu()


class Device(VerifyDevice):
    """test_verify_gpu.Device with the align call."""

    def align(self, occ, band, me, Q=None):
        self.K.align_seeds(self.idx, Q or self.Q, self.iv, self.sp, self.hits, self.s, self.strands, occ, band, me)
        self.K.transfer_to_cpu(self.hits)
        return self.hits.array().copy().reshape(self.T, 2)


def check_lengths(K, w, k, what, lengths=None, seeds=(1, 8), strands=ar.STRANDS, occs=(1, 8), bands=GPU_BANDS, host=False):
    """Device against model: per length and strand mode one upload of the reads
    per S, then every (max_occ, band, max_edits)."""
    idx = w["idx"][k]
    for m, (q, both, per_k) in w["cases"].items():
        if lengths is not None and m not in lengths:
            continue
        iv, sp, a = per_k[k]
        for st in strands:
            rows = vr.strand_rows(st)
            for s in seeds if st == sr.BOTH else seeds[-1:]:
                d = Device(K, idx, q, s, st)
                try:
                    d.seeds()
                    for occ in occs:
                        for band in bands:
                            for me in ar.edit_bounds(m):
                                got = d.align(occ, band, me)
                                same(got, ar.records(a, s, occ, band, me, rows), (what, m, st, s, occ, band, me))
                                if host and me == 1:
                                    same(got, host_hits(K, w["world"], q, np.ascontiguousarray(iv[rows, :s]),
                                                        np.ascontiguousarray(sp[rows, :s]), s, st, occ, band, me),
                                         (what, "host form", m, st, s, occ, band, me))
                finally:
                    d.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("text", list(vr.texts()))
def test_task_mid_every_length(world, text, k):
    """task-mid at K = 1, 2: both stagings at every length (the dword edges,
    the 8 | 16 word switch, odd m at K = 2), bands 0, 1, 3 and 15, every window
    shift at both ends of the word stream, band cells off either end of the
    text, indels at the pinned positions, repeats."""
    K, w = world
    try:
        defaults(K)
        fresh_upload(K, w[text]["idx"][k], "task-mid")
        check_lengths(K, w[text], k, (text, k), host=(text == "n1009"))
        assert w[text]["idx"][k].jump_bytes() != 0
    finally:
        defaults(K)


def test_band_zero_is_the_verify(world):
    """Band 0 on the device equals kfmi_verify_seeds on the same device handles."""
    K, w = world
    K.set_backend("task-mid")
    for text in ("main", "n1009"):
        x = w[text]
        for m in (1, 17, 100, 129, 256):
            q = x["cases"][m][0]
            for st in ar.STRANDS:
                d = Device(K, x["idx"][2], q, 8, st)
                try:
                    d.seeds()
                    for occ in (1, 8):
                        for mm in (0, 3, m):
                            want = d.verify(occ, mm)
                            same(d.align(occ, 0, mm), want, (text, m, st, occ, mm))
                finally:
                    d.close()


def test_task_backend(world):
    """The reference's own layout (tag 101): the "task" backend at K = 2."""
    K, w = world
    try:
        defaults(K)
        fresh_upload(K, w["main"]["idx"][2], "task")
        check_lengths(K, w["main"], 2, "task", seeds=(4,), occs=(8,), bands=(1, 15))
    finally:
        defaults(K)
        fresh_upload(K, w["main"]["idx"][2], "task-mid")


def hand_made(K, x, ks, occs, what):
    q, iv, sp = handmade(x["world"])
    for k in ks:
        d = Device(K, x["idx"][k], q, 8, sr.FWD)
        try:
            d.iv.array()[:] = iv.reshape(-1)
            d.sp.array()[:] = sp.reshape(-1)
            K.results_to_gpu(d.iv)
            K.results_to_gpu(d.sp)
            for occ in occs:
                a = ar.Aligned(x["world"], q, vr.candidates(x["world"], q, iv, sp, occ), bands=(0, 2, 15))
                for band in (0, 2, 15):
                    for me in (0, 40, 0xFFFFFFFF):
                        got = d.align(occ, band, me)
                        same(got, ar.records(a, 8, occ, band, me), (what, k, occ, band, me))
                        same(got, host_hits(K, x["world"], q, iv, sp, 8, sr.FWD, occ, band, me), (what, "host form", k, occ, band, me))
            assert (d.align(256, 15, 40)[:, 1] >> ar.SCORED_SHIFT).max() > 200
        finally:
            d.close()


def test_hand_made_handles(world):
    """Slots filled on the host and transferred: the whole array cut by
    max_occ, every ignored-slot form, R > rows, garbage."""
    K, w = world
    K.set_backend("task-mid")
    hand_made(K, w["n1005"], (1, 2), (1, 7, 256), "hand-made")


def test_split_classes(world):
    """The loads under the 16-lane group mask (class 4), then the plain form
    (class 1) on the same upload: lengths 100, 101, 129, 256 at bands 1 and 15,
    and the hand-made handles at max_occ 256."""
    K, w = world
    x = w["n1005"]
    try:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")
        for cls in (4, 1):
            K.set_split_class(cls)
            check_lengths(K, x, 2, ("class", cls), lengths=(100, 101, 129, 256), seeds=(4,), occs=(8,), bands=(1, 15))
            hand_made(K, x, (2,), (256,), ("hand-made, class", cls))
    finally:
        defaults(K)
        fresh_upload(K, x["idx"][2], "task-mid")


@pytest.fixture(scope="module")
def edges(world):
    """513 shuffled reads of 100 and of 101 bases of the main text with their model at band 3."""
    _, w = world
    x = w["main"]
    out = {}
    for m in (100, 101):
        q = ar.reads_for(x["text"], m, 21_000 + m)
        q = np.ascontiguousarray(np.concatenate([q, q[::-1]])[np.random.default_rng(m).permutation(2 * q.shape[0])[:513]])
        assert q.shape[0] == 513
        both = sr.tasks_of(q, sr.BOTH)
        iv, sp, _ = sr.reference(x["search"], both, 2, 4)
        out[m] = (q, ar.Aligned(x["world"], both, vr.candidates(x["world"], both, iv, sp, 8), bands=(3,)))
    return out


@pytest.mark.parametrize("m", [100, 101])
def test_batch_edges(world, edges, m):
    """Batches that end inside a wave, a staging round or a block, in all three
    strand modes, on a hits handle pre-filled with 0xA5A5A5A5; a stale align of
    other reads runs first on the same device arrays; after each small batch
    the whole batch again."""
    K, w = world
    q, a = edges[m]
    idx = w["main"]["idx"][2]
    K.set_backend("task-mid")
    for num in EDGE_SIZES:
        part = np.ascontiguousarray(q[:num])
        stale = np.ascontiguousarray(np.roll(part, 1, axis=0)[:, ::-1])
        for st in ar.STRANDS:
            rows = vr.strand_rows(st)
            T = (2 if st == sr.BOTH else 1) * num
            d = Device(K, idx, part, 4, st)
            P = K.Queries.from_array(stale)
            try:
                K.transfer_to_gpu(idx, P, None)
                d.seeds(P)
                d.align(8, 3, m, P)                   # other reads' records in every entry
                d.seeds()
                same(d.align(8, 3, 3), ar.records(a, 4, 8, 3, 3, rows)[:T], (m, num, st))
            finally:
                P.close()
                d.close()
            d = Device(K, idx, q, 4, st)
            try:
                d.seeds()
                same(d.align(8, 3, 3), ar.records(a, 4, 8, 3, 3, rows), (m, num, st, "whole batch after"))
            finally:
                d.close()


def test_tables_built_on_demand(world, oracle_mod):
    """An upload under set_jump(0) has no tables; the align builds them,
    answers as the model does, and a forward search afterwards still equals
    the oracle."""
    K, w = world
    x = w["n1008"]
    idx = x["idx"][2]
    q, both, per_k = x["cases"][100]
    iv, sp, a = per_k[2]
    try:
        defaults(K)
        K.set_jump(0)
        fresh_upload(K, idx, "task-mid")
        assert idx.jump_bytes() == 0
        d = Device(K, idx, q, 4, sr.BOTH)
        try:
            d.seeds()
            assert idx.jump_bytes() == 0
            got = d.align(8, 3, 100)
            assert idx.jump_bytes() != 0
            same(got, ar.records(a, 4, 8, 3, 100), "tables built by the call")
        finally:
            d.close()
        K.set_jump("auto")
        want = oracle_mod.search(x["idx"][1].image(), q)[0]
        assert np.array_equal(K.search_array(idx, q, "task-mid"), np.asarray(want).reshape(-1))
    finally:
        defaults(K)
        fresh_upload(K, idx, "task-mid")


def refused(K, idx, q, s, strands, occ=8, band=3, call=None):
    """(error code, whether the hits on the device hold anything but what they held before the call);
    call = (S, strands, max_occ, band) of the align when they differ from the handles'."""
    d = Device(K, idx, q, s, strands)
    try:
        code = 0
        try:
            if call:
                K.align_seeds(idx, d.Q, d.iv, d.sp, d.hits, call[0], call[1], call[2], call[3], 3)
            else:
                K.align_seeds(idx, d.Q, d.iv, d.sp, d.hits, s, strands, occ, band, 3)
        except K.KfmiError as e:
            code = e.code
        K.transfer_to_cpu(d.hits)
        return code, bool((d.hits.array() != d.filled).any())
    finally:
        d.close()


def test_refusals_write_nothing(world):
    K, w = world
    t = w["main"]["text"]
    q = w["main"]["cases"][100][0][:64]
    idx2 = w["main"]["idx"][2]
    idx4 = K.Index.build(t.tobytes(), k=4, d=64)
    try:
        defaults(K)
        K.set_backend("task-mid")
        assert refused(K, idx2, q, 3, K.STRAND_BOTH) == (0, True)
        for call in ((0, 1, 8, 3), (9, 1, 8, 3), (3, 0, 8, 3), (3, 4, 8, 3), (3, 1, 0, 3), (3, 1, 257, 3), (2, 1, 8, 3),
                     (3, 3, 8, 3), (3, 1, 8, 16), (3, 1, 8, 0xFFFFFFFF)):
            assert refused(K, idx2, q, 3, K.STRAND_FWD, call=call) == (33, False), call
        for backend, idx in (("coop-mid", idx2), ("task-ac-mid", idx2), ("task-grp", idx4)):
            K.set_backend(backend)
            assert refused(K, idx, q, 3, K.STRAND_FWD) == (19, False), backend
            assert refused(K, idx, q, 2, K.STRAND_BOTH) == (19, False), backend
        K.set_backend("task-mid")
        K.set_devices([0, 0])
        assert refused(K, idx2, q, 3, K.STRAND_FWD) == (19, False)
        K.set_devices([])
        long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
        assert refused(K, idx2, long, 3, K.STRAND_FWD) == (33, False)
        assert refused(K, idx2, long, 1, K.STRAND_REV) == (33, False)
        # handles of another size
        d = Device(K, idx2, q, 3, K.STRAND_FWD)
        other = K.Results.alloc(d.T + 1)
        try:
            K.transfer_to_gpu(idx2, None, other)
            for args in ((d.iv, d.sp, other, 3), (d.iv, other, d.hits, 3), (other, d.sp, d.hits, 3), (d.iv, d.sp, d.hits, 2)):
                with pytest.raises(K.KfmiError) as e:
                    K.align_seeds(idx2, d.Q, args[0], args[1], args[2], args[3], K.STRAND_FWD, 8, 3, 0)
                assert e.value.code == 33
            K.transfer_to_cpu(d.hits)
            assert (d.hits.array() == FILL).all()
        finally:
            other.close()
            d.close()
    finally:
        defaults(K)
        idx2.free_gpu()
        idx4.close()


CHILD = r"""
import json, sys
sys.path[:0] = %(paths)r
import numpy as np
import kstep_fmi as K
K.load(); K.set_device(0); K.set_backend("task-mid")
d = dict(np.load(%(data)r))
idx = K.Index.build(d["text"].tobytes(), k=2, d=64)
q = d["q"]
Q, iv, sp, hits = K.Queries.from_array(q), K.Results.alloc(3 * q.shape[0]), K.Results.alloc(3 * q.shape[0]), K.Results.alloc(q.shape[0])
hits.array()[:] = 0xA5A5A5A5
K.transfer_to_gpu(idx, Q, iv); K.transfer_to_gpu(idx, None, sp); K.transfer_to_gpu(idx, None, hits)
K.results_to_gpu(hits)
K.search_seeds(idx, Q, iv, sp, 3, 1)
code = 0
try:
    K.align_seeds(idx, Q, iv, sp, hits, 3, 1, 8, 3, 3)
except K.KfmiError as e:
    code = e.code
K.transfer_to_cpu(hits)
print(json.dumps({"form": K.upload_form(Q), "code": code, "untouched": bool((hits.array() == 0xA5A5A5A5).all())}))
"""


def test_host_packed_upload_is_refused(world, tmp_path):
    """KFMI_UPLOAD=packed in a process of its own: no ASCII rows on the device, 19, nothing written."""
    _, w = world
    fn = tmp_path / "align.npz"
    np.savez(fn, text=w["n1005"]["text"], q=w["n1005"]["cases"][100][0])
    env = dict(os.environ)
    for v in ("KFMI_UPLOAD", "KFMI_UPLOAD_CHUNK", "KFMI_DEVICES", "KFMI_BACKEND", "KFMI_FTAB", "KFMI_SKIP", "KFMI_JUMP",
              "KFMI_FUSED"):
        env.pop(v, None)
    env.update({"KFMI_UPLOAD": "packed"})
    code = CHILD % {"paths": [str(util.REPO), str(util.PKG), str(util.REPO / "tests")], "data": str(fn)}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out == {"form": "packed", "code": 19, "untouched": True}, out


def test_last_timing_reports_the_align_kernel(world):
    K, w = world
    x = w["main"]
    K.set_backend("task-mid")
    d = Device(K, x["idx"][2], x["cases"][100][0], 4, sr.BOTH)
    try:
        d.seeds()
        d.align(8, 3, 3)
        t = K.last_timing()
        assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
    finally:
        d.close()


def test_map_reads_device_equals_host(world):
    """End to end: upload, seed search and align in one call, against the same call on the host."""
    K, w = world
    x = w["main"]
    q = x["cases"][101][0]
    try:
        defaults(K)
        got = K.map_reads_array(x["idx"][2], q, "task-mid", max_seeds=4, max_occ=8, band=3, max_edits=3)
        want = K.map_reads_array(x["idx"][2], q, max_seeds=4, max_occ=8, cpu=True, text=x["text"], band=3, max_edits=3)
        for g, h, name in zip(got, want, ("origin", "edits", "multi", "scored")):
            assert np.array_equal(g, h), name
        assert (got[0] >= 0).any() and (got[0] < 0).any() and got[2].any()
        plain = K.map_reads_array(x["idx"][2], q, "task-mid", max_seeds=4, max_occ=8, max_mism=3)
        assert (got[0] >= 0).sum() > (plain[0] >= 0).sum()     # reads with an indel are placed now
    finally:
        defaults(K)
