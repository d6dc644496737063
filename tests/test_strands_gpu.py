"""Strand searches on the device (kstep_fmi.h "both strands"):
a reverse-strand interval is, bit for bit, what the forward search of the same
backend returns for the reverse complement, and BOTH interleaves the two --
every backend, K = 1-4, read lengths across the pack paths and m % K != 0,
odd batch sizes, tables on and off, host-packed uploads, the streamed call
(every chunk mode, device groups) and locate on a BOTH handle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from skip_texts import texts
from strand_reads import N_READS, strand_reads

TASK = ("task", "task-mid", "task-ac", "task-ac-mid")
ALT = ("task-ac", "task-ac-mid")
LENGTHS = (15, 16, 17, 31, 33, 100, 101, 128, 129, 256, 257, 300)
SIZES = (N_READS, 1_003, 33, 1)


@pytest.fixture(scope="module")
def gpu(kfmi_mod):
    if kfmi_mod.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    kfmi_mod.set_device(0)
    kfmi_mod.set_devices([])
    yield kfmi_mod
    _defaults(kfmi_mod)


def _defaults(K):
    K.set_devices([])
    K.set_split_class(0)
    K.set_fused(True)
    K.set_ftab_budget(None)
    K.set_skip("auto")
    K.set_ftab("auto")


@pytest.fixture(scope="module")
def world(gpu):
    """Indexes built on first use and kept for the module."""
    cache = {}

    def index(name, k, d, sa_rate=0):
        key = (name, k, d, sa_rate)
        if key not in cache:
            cache[key] = gpu.Index.build(texts()[name].tobytes(), k=k, d=d, sa_rate=sa_rate)
        return cache[key]

    yield index
    for i in cache.values():
        i.close()


def _oracle(oracle_mod, index, name, idx, backend, k, q):
    """The CPU oracle on the index's own image (the AltCounters one for those
    backends); for m % K != 0 the true interval, which is the K = 1 oracle's."""
    if q.shape[1] % k:
        img = index(name, 1, 64).image()
    elif backend in ALT:
        ac = idx.alt_counters()
        img = ac[0].image().copy()
        for i in ac:
            i.close()
    else:
        img = idx.image()
    return oracle_mod.search(img, q)[0]


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int(np.flatnonzero(got != want)[0]) // 2)


def _interleave(fwd, rev):
    both = np.empty((fwd.size // 2 * 2, 2), np.uint32)
    both[0::2], both[1::2] = fwd.reshape(-1, 2), rev.reshape(-1, 2)
    return both.ravel()


def _want(gpu, oracle_mod, world, name, idx, backend, k, q):
    """The forward search on q and on revcomp(q) under the pure walk, each equal
    to the oracle, with at least a quarter of either strand's intervals non-empty."""
    gpu.set_ftab(0)
    gpu.set_skip(0)
    rq = gpu.revcomp(q)
    fwd, rev = gpu.search_array(idx, q, backend), gpu.search_array(idx, rq, backend)
    for got, reads in ((fwd, q), (rev, rq)):
        want = _oracle(oracle_mod, world, name, idx, backend, k, reads)
        _same(got, want, "forward search != oracle")
        assert np.count_nonzero(want[1::2] > want[0::2]) >= q.shape[0] // 4
    return fwd, rev


CASES = ([(b, k, 64) for b in ("task", "task-mid", "coop", "coop-mid", "task-ac", "task-ac-mid") for k in (1, 2)] +
         [("task-mid", k, 192) for k in (1, 2)] +
         [(b, k, 64) for b in ("task-grp", "coop-grp") for k in (3, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain", "dup"])
@pytest.mark.parametrize("backend,k,d", CASES, ids=[f"{b}-k{k}d{d}" for b, k, d in CASES])
def test_strands_equal_forward_search_of_the_reverse_complement(gpu, oracle_mod, world, backend, k, d, name):
    K = gpu
    t = texts()[name]
    idx = world(name, k, d)
    try:
        _defaults(K)
        K.set_backend(backend)
        idx.free_gpu()                                       # a fresh upload under the auto settings:
        K.transfer_to_gpu(idx, None, None)                   # its tables are built here
        for m in LENGTHS:
            q = strand_reads(t, m, seed=m * 13 + k)
            if backend in ALT and m % k:                     # AltCounters semantics take no remainder
                for strands in (K.STRAND_REV, K.STRAND_BOTH):
                    with pytest.raises(K.KfmiError) as e:
                        K.search_array(idx, q, backend, strands=strands)
                    assert e.value.code == 33, m
                continue
            fwd, rev = _want(K, oracle_mod, world, name, idx, backend, k, q)
            both = _interleave(fwd, rev)
            for what, ftab, skip, fused in (("walk", 0, 0, True), ("auto", "auto", "auto", True),
                                            ("auto, not fused", "auto", "auto", False)):
                K.set_ftab(ftab)
                K.set_skip(skip)
                K.set_fused(fused)
                for num in SIZES:
                    got = K.search_array(idx, q[:num], backend, strands=K.STRAND_REV)
                    _same(got, rev[:2 * num], (m, what, num, "REV"))
                    got = K.search_array(idx, q[:num], backend, strands=K.STRAND_BOTH)
                    _same(got, both[:4 * num], (m, what, num, "BOTH"))
                if what == "auto" and backend in TASK and k <= 2:
                    assert idx.skip_bytes() != 0, m          # the auto tables are on the device
                    assert idx.ftab_bytes() != 0, m
                K.set_fused(True)
    finally:
        _defaults(K)


@pytest.mark.gpu
def test_fwd_through_the_new_call_is_kfmi_search(gpu, world):
    K = gpu
    idx = world("plain", 2, 64)
    q = strand_reads(texts()["plain"], 100, seed=11)
    try:
        _defaults(K)
        want = K.search_array(idx, q, "task-mid")
        Q, R = K.Queries.from_array(q), K.Results.alloc(q.shape[0])
        K.transfer_to_gpu(idx, Q, R)
        K.search_strands(idx, Q, R, K.STRAND_FWD)
        K.transfer_to_cpu(R)
        _same(R.array().copy(), want, "FWD")
        Q.close()
        R.close()
    finally:
        _defaults(K)


CHILD = r"""
import json, sys
sys.path[:0] = %(paths)r
import numpy as np
import kstep_fmi as K
from skip_texts import texts
from strand_reads import strand_reads
K.load(); K.set_device(0); K.set_backend("task-mid")
t = texts()["dup"]
idx = K.Index.build(t.tobytes(), k=2, d=64)
out = {}
for m in (100, 101):
    q = strand_reads(t, m, seed=m)
    rq = K.revcomp(q)
    fwd, rev = K.search_array(idx, q), K.search_array(idx, rq)
    both = np.empty((2 * q.shape[0], 2), np.uint32)
    both[0::2], both[1::2] = fwd.reshape(-1, 2), rev.reshape(-1, 2)
    both = both.ravel()
    if %(mode)r == "upload":
        Q, R = K.Queries.from_array(q), K.Results.alloc(2 * q.shape[0])
        K.transfer_to_gpu(idx, Q, R)
        out["form_%%d" %% m] = K.upload_form(Q)
        K.search_strands(idx, Q, R, K.STRAND_BOTH)
        K.transfer_to_cpu(R)
        out["both_%%d" %% m] = bool(np.array_equal(R.array(), both))
        Q.close(); R.close()
        out["rev_%%d" %% m] = bool(np.array_equal(K.search_array(idx, q, strands=K.STRAND_REV), rev))
    else:
        K.transfer_to_gpu(idx, None, None)
        for chunk in (300, 0):
            got = K.search_stream(idx, q, chunk=chunk, strands=K.STRAND_BOTH)
            out["both_%%d_%%d" %% (m, chunk)] = bool(np.array_equal(got, both))
            got = K.search_stream(idx, q, chunk=chunk, strands=K.STRAND_REV)
            out["rev_%%d_%%d" %% (m, chunk)] = bool(np.array_equal(got, rev))
        out["fwd_%%d" %% m] = bool(np.array_equal(K.search_stream(idx, q, chunk=300), fwd))
        out["packed_%%d" %% m] = K.load().kfmi_stream_hostpacked_fraction()
    out["nonempty_%%d" %% m] = [int(np.count_nonzero(x[1::2] > x[0::2])) for x in (fwd, rev)]
print(json.dumps(out))
"""


def _child(mode, env_extra):
    env = dict(os.environ)
    for v in ("KFMI_UPLOAD", "KFMI_UPLOAD_CHUNK", "KFMI_STREAM_HOSTPACK", "KFMI_STREAM_CHUNK", "KFMI_DEVICES",
              "KFMI_BACKEND", "KFMI_FTAB", "KFMI_SKIP", "KFMI_FUSED"):
        env.pop(v, None)
    env.update(env_extra)
    code = CHILD % {"paths": [str(util.REPO), str(util.PKG), str(util.REPO / "tests")], "mode": mode}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_host_packed_upload(gpu):
    """KFMI_UPLOAD=packed: no ASCII on the device, the task columns come from
    the forward code words alone."""
    out = _child("upload", {"KFMI_UPLOAD": "packed", "KFMI_UPLOAD_CHUNK": "400"})
    for m in (100, 101):
        assert out[f"form_{m}"] == "packed"
        assert out[f"both_{m}"] and out[f"rev_{m}"], out
        assert min(out[f"nonempty_{m}"]) >= N_READS // 4, out


@pytest.mark.gpu
@pytest.mark.parametrize("hostpack", ["0", "1", "3"])
def test_search_stream(gpu, hostpack):
    out = _child("stream", {"KFMI_STREAM_HOSTPACK": hostpack})
    for m in (100, 101):
        for chunk in (300, 0):
            assert out[f"both_{m}_{chunk}"] and out[f"rev_{m}_{chunk}"], out
        assert out[f"fwd_{m}"], out
        assert min(out[f"nonempty_{m}"]) >= N_READS // 4, out
        # the last call (FWD, chunk 300): 0 = no chunk host-packed, 1 = all, 3 = alternate
        frac = out[f"packed_{m}"]
        assert {"0": frac == 0.0, "1": frac == 1.0, "3": 0.0 < frac < 1.0}[hostpack], out


@pytest.mark.gpu
def test_device_group_two_replicas(gpu, world):
    """The streamed call on a group: member slices of reads are slices of
    results; the resident call is a follow-up there (19)."""
    K = gpu
    idx = world("dup", 2, 64)
    try:
        _defaults(K)
        for m in (100, 101):
            q = strand_reads(texts()["dup"], m, seed=m + 5)
            fwd, rev = K.search_array(idx, q, "task-mid"), K.search_array(idx, K.revcomp(q), "task-mid")
            K.set_devices([0, 0])
            K.transfer_to_gpu(idx, None, None)
            for chunk in (300, 0):
                _same(K.search_stream(idx, q, chunk=chunk, strands=K.STRAND_BOTH), _interleave(fwd, rev), (m, chunk))
                _same(K.search_stream(idx, q, chunk=chunk, strands=K.STRAND_REV), rev, (m, chunk))
            Q, R = K.Queries.from_array(q), K.Results.alloc(2 * q.shape[0])
            with pytest.raises(K.KfmiError) as e:            # the index is on the group
                K.search_strands(idx, Q, R, K.STRAND_BOTH)
            assert e.value.code == 19
            Q.close()
            R.close()
            K.set_devices([])
    finally:
        _defaults(K)
        idx.free_gpu()


@pytest.mark.gpu
@pytest.mark.parametrize("sa_rate", [1, 32])
def test_locate_on_a_both_handle(gpu, world, sa_rate):
    """kfmi_locate sees 2 * num intervals: positions of P at 2q, of P' at 2q + 1."""
    K = gpu
    name, m = "dup", 32
    t = texts()[name]
    idx = world(name, 2, 64, sa_rate)
    q = strand_reads(t, m, seed=77)
    q = np.ascontiguousarray(np.concatenate([q[:64], q[-192:]]))   # changed bases and N; windows of either strand
    rq = K.revcomp(q)
    try:
        _defaults(K)
        K.set_backend("task-mid")
        Q, R = K.Queries.from_array(q), K.Results.alloc(2 * q.shape[0])
        K.transfer_to_gpu(idx, Q, R)
        K.search_strands(idx, Q, R, K.STRAND_BOTH)
        loc = K.locate(idx, R)
        off, pos = loc.offsets().copy(), loc.positions().copy()
        loc.close()
        Q.close()
        R.close()
        assert off.size == 2 * q.shape[0] + 1
        tb = t.tobytes()
        found = [0, 0]
        for i in range(q.shape[0]):
            for s, reads in enumerate((q, rq)):
                p = bytes(b"ACGT"[util.code_of(c)] for c in reads[i].tobytes())
                want, at = [], tb.find(p)
                while at >= 0:
                    want.append(at)
                    at = tb.find(p, at + 1)
                got = sorted(int(x) for x in pos[off[2 * i + s]:off[2 * i + s + 1]])
                assert got == want, (i, s)
                found[s] += bool(want)
        assert min(found) >= q.shape[0] // 4
    finally:
        _defaults(K)
