"""Second placement / mapping quality on the device (kfmi_align_second,
kfmi_map_quality) against the model of second_ref.py, bit for bit on both
words of every record.

The hits the second pass reads are the ones kfmi_align_seeds left on the
device (checked against align_ref's model first), the seed records the ones
kfmi_search_seeds left there or piece seeds sent up by the binding.  The model
is computed once per length for both strands; smaller S and max_occ and the
strand modes are cuts of it.  The non-vacuity conditions are asserted on the
model alone in second_ref.world, before any device call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as ar
import second_ref as s2
import seed_ref as sr
import util
import verify_ref as vr
from test_align_gpu import Device as AlignDevice
from test_verify_gpu import defaults, fresh_upload, same
from test_verify_host import handmade

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
EDGE_SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def world(kfmi_mod, oracle_mod):
    K = kfmi_mod
    if K.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    w = s2.world(K, oracle_mod)       # the model and its conditions first
    K.set_device(0)
    defaults(K)
    yield K, w
    defaults(K)
    for i in w["idx"].values():
        i.free_gpu()


class Device(AlignDevice):
    """test_align_gpu.Device with the `second` and `quals` handles and the two calls."""

    def __init__(self, K, idx, q, s, strands):
        super().__init__(K, idx, q, s, strands)
        self.sec, self.ql = K.Results.alloc(self.T), K.Results.alloc(self.T)
        for h in (self.sec, self.ql):
            h.array()[:] = FILL
            K.transfer_to_gpu(idx, None, h)
            K.results_to_gpu(h)

    def pieces(self, q):
        return self.K.piece_seeds(self.idx, q, self.s, self.strands, self.iv, self.sp)

    def put_hits(self, hits):
        self.hits.array()[:] = np.asarray(hits, np.uint32).reshape(-1)
        self.K.results_to_gpu(self.hits)

    def second(self, occ, band, ms):
        self.K.align_second(self.idx, self.Q, self.iv, self.sp, self.hits, self.sec, self.s, self.strands, occ, band, ms)
        self.K.transfer_to_cpu(self.sec)
        return self.sec.array().copy().reshape(self.T, 2)

    def quality(self, ms):
        self.K.map_quality(self.idx, self.hits, self.sec, self.ql, self.strands, ms)
        self.K.transfer_to_cpu(self.ql)
        return self.ql.array().copy().reshape(self.T, 2)

    def close(self):
        super().close()
        for h in (self.sec, self.ql):
            h.close()


def check(K, idx, q, x, what, seeds, strands=ar.STRANDS, occs=(1, 8), bands=s2.BANDS, pieces=False):
    """Device against model for one Seeded x of the reads q: per strand mode and S one upload, then every
    (max_occ, band, max_second) on the hits the device's own align left."""
    m = q.shape[1]
    for st in strands:
        rows = vr.strand_rows(st)
        for s in seeds if st == sr.BOTH else seeds[-1:]:
            if pieces and s != x.S:
                continue                                           # a piece set is searched at its own S
            d = Device(K, idx, q, s, st)
            try:
                if pieces:
                    iv, _ = d.pieces(q)
                    found = x.iv[rows][:, :, 1] > x.iv[rows][:, :, 0]
                    assert np.array_equal(iv[found], x.iv[rows][found]), (what, "piece rows", st)
                else:
                    d.seeds()
                for occ in occs:
                    trunc = x.trunc(s, occ)
                    for band in bands:
                        hits = ar.records(x.a, s, occ, band, m)
                        same(d.align(occ, band, m), hits[rows], (what, "align", m, st, s, occ, band))
                        for ms in s2.second_bounds(m):
                            want = s2.second_records(x.a, hits[:, 0], s, occ, band, ms, trunc)[rows]
                            same(d.second(occ, band, ms), want, (what, m, st, s, occ, band, ms))
                            same(d.quality(ms), s2.quality(hits[rows], want, st, ms), (what, "quality", m, st, s, occ, band, ms))
            finally:
                d.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("backend", ["task-mid", "task"])
def test_device_equals_the_model(world, backend, k):
    """The seed handles kfmi_search_seeds left on the device, every length (both
    code-word counts, odd m at K = 2), bands 0, 1, 3 and 15."""
    K, w = world
    idx = w["idx"][k]
    try:
        defaults(K)
        fresh_upload(K, idx, backend)
        for m, (q, both, greedy, piece) in w["cases"].items():
            if backend == "task":
                check(K, idx, q, greedy[k], (backend, k), (8,), occs=(8,), bands=(1, 3))
            else:
                check(K, idx, q, greedy[k], (backend, k), (1, 8))
        assert idx.jump_bytes() != 0
    finally:
        defaults(K)
        fresh_upload(K, idx, "task-mid")


@pytest.mark.parametrize("k", [1, 2])
def test_piece_seeds_sent_up(world, k):
    """Piece seeds searched on the device, written into the handles' host arrays and sent up."""
    K, w = world
    idx = w["idx"][k]
    try:
        defaults(K)
        fresh_upload(K, idx, "task-mid")
        for m, (q, both, greedy, piece) in w["cases"].items():
            check(K, idx, q, piece, ("pieces", k), (s2.PIECES,), pieces=True)
    finally:
        defaults(K)


def test_hits_with_none_and_hand_made_handles(world):
    """Caller-filled hits (KFMI_HIT_NONE from max_edits = 0, X past the text, 0) and test_verify_host.handmade's slots."""
    K, w = world
    K.set_backend("task-mid")
    idx = w["idx"][2]
    q, both, greedy, piece = w["cases"][128]
    x = greedy[2]
    d = Device(K, idx, q, 8, sr.BOTH)
    try:
        d.seeds()
        hits = ar.records(x.a, 8, 8, 3, 0)
        assert (hits[:, 0] == s2.NONE).any() and (hits[:, 0] != s2.NONE).any()
        d.put_hits(hits)
        want = s2.second_records(x.a, hits[:, 0], 8, 8, 3, 128, x.trunc(8, 8))
        same(d.second(8, 3, 128), want, "hits with NONE")
        same(d.quality(128), s2.quality(hits, want, sr.BOTH, 128), "quality of hits with NONE")
    finally:
        d.close()
    wd = w["world"]
    q, iv, sp = handmade(wd)
    d = Device(K, idx, q, 8, sr.FWD)
    try:
        d.iv.array()[:] = iv.reshape(-1)
        d.sp.array()[:] = sp.reshape(-1)
        K.results_to_gpu(d.iv)
        K.results_to_gpu(d.sp)
        for occ in (1, 7, 256):
            a = ar.Aligned(wd, q, vr.candidates(wd, q, iv, sp, occ), bands=(0, 2, 15))
            trunc = s2.truncated(wd, q.shape[1], iv, sp, 8, occ)
            for band in (0, 2, 15):
                own = ar.records(a, 8, occ, band, 0xFFFFFFFF)
                for X in (own[:, 0], np.asarray([s2.NONE, wd.n + 50, 0, 7], np.uint32)):
                    hits = np.stack([X, np.full(4, FILL, np.uint32)], axis=1)
                    d.put_hits(hits)
                    for ms in (0, 40, 0xFFFFFFFF):
                        got = d.second(occ, band, ms)
                        same(got, s2.second_records(a, X, 8, occ, band, ms, trunc), ("hand-made", occ, band, ms))
                        same(d.quality(ms), s2.quality(hits, got, sr.FWD, ms), ("hand-made quality", occ, band, ms))
    finally:
        d.close()


@pytest.fixture(scope="module")
def edges(world):
    """257 reads of 100 and of 129 bases with their model at band 3 (greedy seeds at S = 4, K = 2)."""
    _, w = world
    out = {}
    for m in (100, 129):
        q0 = w["cases"][m][0]
        q = np.ascontiguousarray(np.concatenate([q0, q0[:8]])[np.random.default_rng(m).permutation(q0.shape[0] + 8)[:257]])
        assert q.shape[0] == 257
        both = sr.tasks_of(q, sr.BOTH)
        iv, sp, _ = sr.reference(w["search"], both, 2, 4)
        out[m] = (q, s2.Seeded(w["world"], m, both, iv, sp, bands=(3,)))
    return out


@pytest.mark.parametrize("m", [100, 129])
def test_batch_edges(world, edges, m):
    """Batches that end inside a wave, a staging round or a block, in all three
    strand modes, on handles pre-filled with 0xA5A5A5A5: every entry is written."""
    K, w = world
    q, x = edges[m]
    idx = w["idx"][2]
    K.set_backend("task-mid")
    hits = ar.records(x.a, 4, 8, 3, m)
    want = s2.second_records(x.a, hits[:, 0], 4, 8, 3, 3, x.trunc(4, 8))
    for num in EDGE_SIZES:
        part = np.ascontiguousarray(q[:num])
        for st in ar.STRANDS:
            rows = vr.strand_rows(st)
            T = (2 if st == sr.BOTH else 1) * num
            d = Device(K, idx, part, 4, st)
            try:
                d.seeds()
                same(d.align(8, 3, m), hits[rows][:T], (m, num, st, "align"))
                got = d.second(8, 3, 3)
                same(got, want[rows][:T], (m, num, st))
                same(d.quality(3), s2.quality(hits[rows][:T], got, st, 3), (m, num, st, "quality"))
            finally:
                d.close()


def test_split_classes(world):
    """The loads under the 16-lane group mask (class 4, the grouped-load form),
    then the plain form (class 1) on the same upload."""
    K, w = world
    idx = w["idx"][2]
    try:
        defaults(K)
        fresh_upload(K, idx, "task-mid")
        for cls in (4, 1):
            K.set_split_class(cls)
            for m in (17, 100, 129, 256):
                q, both, greedy, piece = w["cases"][m]
                check(K, idx, q, greedy[2], ("class", cls), (8,), strands=(sr.BOTH,), occs=(8,), bands=(1, 15))
                check(K, idx, q, piece, ("class", cls, "pieces"), (s2.PIECES,), strands=(sr.BOTH,), occs=(8,), bands=(3,),
                      pieces=True)
    finally:
        defaults(K)
        fresh_upload(K, idx, "task-mid")


def test_quality_modes_by_hand(world):
    """kfmi_map_quality on records written out by hand, in FWD, REV and BOTH."""
    K, w = world
    K.set_backend("task-mid")
    idx, N = w["idx"][2], s2.NONE
    K.transfer_to_gpu(idx, None, None)
    hits = np.asarray([[10, 1], [N, 0], [10, 2], [500, 2], [10, 0], [20, 0], [10, 0], [N, 0]], np.uint32)
    sec = np.asarray([[90, 3], [N, 0], [N, 0], [N, 0], [N, s2.TRUNC], [N, 0], [N, 0], [N, 0]], np.uint32)
    hs = [K.Results.alloc(8) for _ in range(3)]
    try:
        for h, a in zip(hs, (hits, sec, np.full((8, 2), FILL, np.uint32))):
            h.array()[:] = a.reshape(-1)
            K.transfer_to_gpu(idx, None, h)
            K.results_to_gpu(h)
        for strands in ar.STRANDS:
            for ms in (0, 6, 0xFFFFFFFF):
                K.map_quality(idx, hs[0], hs[1], hs[2], strands, ms)
                K.transfer_to_cpu(hs[2])
                same(hs[2].array().copy().reshape(8, 2), s2.quality(hits, sec, strands, ms), (strands, ms))
        t = K.last_timing()
        assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
    finally:
        for h in hs:
            h.close()


def test_last_timing_reports_the_second_kernel(world):
    K, w = world
    K.set_backend("task-mid")
    d = Device(K, w["idx"][2], w["cases"][100][0], 4, sr.BOTH)
    try:
        d.seeds()
        d.align(8, 3, 100)
        d.second(8, 3, 3)
        t = K.last_timing()
        assert t["pack_ms"] == 0 and t["lf_ms"] > 0 and t["total_ms"] == t["lf_ms"]
    finally:
        d.close()


def test_map_reads_end_to_end(world):
    """map_reads_array(mapq=True) on the device against the same call on the
    host, with greedy and with piece seeds; without the new keyword arguments
    the call returns the four arrays it returned."""
    K, w = world
    q = w["cases"][129][0]
    idx = w["idx"][2]
    try:
        defaults(K)
        for pieces in (None, s2.PIECES):
            got = K.map_reads_array(idx, q, "task-mid", max_seeds=8, max_occ=8, band=3, max_edits=129, mapq=True, max_second=6,
                                    pieces=pieces)
            want = K.map_reads_array(idx, q, max_seeds=8, max_occ=8, cpu=True, text=w["text"], band=3, max_edits=129, mapq=True,
                                     max_second=6, pieces=pieces)
            assert len(got) == len(want) == 6
            for g, h, name in zip(got, want, ("origin", "edits", "multi", "scored", "quality", "gap")):
                assert np.array_equal(g, h), (pieces, name)
            # greedy seeds of the strand a read does not lie on are short and wide: every such task is truncated,
            # which in BOTH mode caps its read's other task at 3
            assert 3 in got[4] and 0 in got[4]
        for v in (60, 10, 20):                                        # piece seeds: no second, E2 = E + 1, E2 = E + 2
            assert v in got[4], v
        plain = K.map_reads_array(idx, q, "task-mid", max_seeds=8, max_occ=8, band=3, max_edits=3)
        assert len(plain) == 4
        x = w["cases"][129][2][2]
        rec = ar.records(x.a, 8, 8, 3, 3)
        assert np.array_equal(plain[0], np.where(rec[:, 0] == s2.NONE, -1, rec[:, 0].astype(np.int64)))
        assert np.array_equal(plain[1], np.where(rec[:, 0] == s2.NONE, 0, rec[:, 1] & s2.EDIT_MASK))
        assert np.array_equal(plain[3], rec[:, 1] >> s2.SCORED_SHIFT)
    finally:
        defaults(K)


def refused(K, idx, q, s, strands, occ=8, band=3, call=None):
    """(error code, whether `second` on the device holds anything but the fill, the same of `quals`)."""
    d = Device(K, idx, q, s, strands)
    try:
        codes = []
        for f in (lambda: K.align_second(idx, d.Q, d.iv, d.sp, d.hits, d.sec, *(call or (s, strands, occ, band)), 3),
                  lambda: K.map_quality(idx, d.hits, d.sec, d.ql, (call or (s, strands))[1], 3)):
            try:
                f()
                codes.append(0)
            except K.KfmiError as e:
                codes.append(e.code)
        K.transfer_to_cpu(d.sec)
        K.transfer_to_cpu(d.ql)
        return codes[0], bool((d.sec.array() != FILL).any()), codes[1], bool((d.ql.array() != FILL).any())
    finally:
        d.close()


def test_refusals_write_nothing(world):
    K, w = world
    t = w["text"]
    q = w["cases"][100][0][:64]
    idx2 = w["idx"][2]
    idx3, idx4 = K.Index.build(t.tobytes(), k=3, d=64), K.Index.build(t.tobytes(), k=4, d=64)
    try:
        defaults(K)
        K.set_backend("task-mid")
        assert refused(K, idx2, q, 3, K.STRAND_BOTH) == (0, True, 0, True)
        for call in ((0, 1, 8, 3), (9, 1, 8, 3), (3, 0, 8, 3), (3, 4, 8, 3), (3, 1, 0, 3), (3, 1, 257, 3), (2, 1, 8, 3),
                     (3, 3, 8, 3), (3, 1, 8, 16), (3, 1, 8, 0xFFFFFFFF)):
            assert refused(K, idx2, q, 3, K.STRAND_FWD, call=call)[:2] == (33, False), call
        for strands in (0, 4):
            assert refused(K, idx2, q, 3, K.STRAND_FWD, call=(3, strands, 8, 3)) == (33, False, 33, False), strands
        for backend, idx in (("coop-mid", idx2), ("task-ac-mid", idx2), ("task-grp", idx3), ("task-grp", idx4)):
            K.set_backend(backend)
            assert refused(K, idx, q, 3, K.STRAND_FWD) == (19, False, 19, False), backend
            assert refused(K, idx, q, 2, K.STRAND_BOTH) == (19, False, 19, False), backend
        K.set_backend("task-mid")
        long = np.ascontiguousarray(np.tile(q, (1, 3))[:, :257])
        assert refused(K, idx2, long, 3, K.STRAND_FWD)[:2] == (33, False)
        # handles of another size, one handle twice
        d = Device(K, idx2, q, 3, K.STRAND_FWD)
        other = K.Results.alloc(d.T + 1)
        try:
            K.transfer_to_gpu(idx2, None, other)
            for args in ((d.iv, d.sp, d.hits, other), (d.iv, d.sp, other, d.sec), (d.iv, other, d.hits, d.sec),
                         (d.iv, d.sp, d.sec, d.sec), (d.iv, d.sp, d.hits, d.iv)):
                with pytest.raises(K.KfmiError) as e:
                    K.align_second(idx2, d.Q, args[0], args[1], args[2], args[3], 3, K.STRAND_FWD, 8, 3, 0)
                assert e.value.code == 33
            for args in ((d.hits, d.sec, other), (d.hits, other, d.ql), (d.hits, d.sec, d.sec), (d.hits, d.hits, d.ql)):
                with pytest.raises(K.KfmiError) as e:
                    K.map_quality(idx2, args[0], args[1], args[2], K.STRAND_FWD, 3)
                assert e.value.code == 33
            for h in (d.sec, d.ql):
                K.transfer_to_cpu(h)
                assert (h.array() == FILL).all()
        finally:
            other.close()
            d.close()
    finally:
        defaults(K)
        idx2.free_gpu()
        idx3.close()
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
n = q.shape[0]
Q, iv, sp, hits, sec = (K.Queries.from_array(q), K.Results.alloc(3 * n), K.Results.alloc(3 * n), K.Results.alloc(n),
                        K.Results.alloc(n))
sec.array()[:] = 0xA5A5A5A5
K.transfer_to_gpu(idx, Q, iv)
for h in (sp, hits, sec):
    K.transfer_to_gpu(idx, None, h)
K.results_to_gpu(sec)
K.search_seeds(idx, Q, iv, sp, 3, 1)
code = 0
try:
    K.align_second(idx, Q, iv, sp, hits, sec, 3, 1, 8, 3, 3)
except K.KfmiError as e:
    code = e.code
K.transfer_to_cpu(sec)
print(json.dumps({"form": K.upload_form(Q), "code": code, "untouched": bool((sec.array() == 0xA5A5A5A5).all())}))
"""


def test_host_packed_upload_is_refused(world, tmp_path):
    """KFMI_UPLOAD=packed in a process of its own: no ASCII rows on the device, 19, nothing written."""
    _, w = world
    fn = tmp_path / "second.npz"
    np.savez(fn, text=w["text"], q=w["cases"][100][0][:64])
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
