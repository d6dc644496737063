"""The reverse strand on the host (kstep_fmi.h, "both strands"), no GPU needed:

* kfmi_revcomp_queries equals a numpy restatement of the definition
  P'[j] = "ACGT"[3 - base2index(P[m-1-j])], N, lowercase and other bytes
  included, and is an involution on ACGT reads;
* kfmi_search_cpu_strands(BOTH) returns at 2q the forward interval of read q
  and at 2q + 1 the forward interval of its reverse complement, both equal to
  the oracle; REV returns the latter alone; FWD is kfmi_search_cpu;
* the code-word identity S' = ~pairreverse_m(S), in both forms the device
  runs (word by word from packed words; the whole stream in 8 or 16
  registers), gives the host packer's words of the reverse complement;
* argument errors: strands outside 1..3 and a results handle too small."""
import numpy as np
import pytest

from skip_texts import ACGT, texts
from strand_reads import revcomp_def, strand_reads


@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 33, 100, 257])
def test_revcomp_equals_the_definition(kfmi_mod, m):
    rng = np.random.default_rng(m)
    q = ACGT[rng.integers(0, 4, size=(300, m))]
    q[:40] = np.frombuffer(b"ACGTNacgtnRx-", np.uint8)[rng.integers(0, 13, size=(40, m))]
    q[40:60] = rng.integers(0, 256, size=(20, m), dtype=np.uint8)
    got = kfmi_mod.revcomp(q)
    assert got.shape == q.shape and got.dtype == np.uint8
    assert np.array_equal(got, revcomp_def(q))
    acgt = np.ascontiguousarray(q[60:])
    assert np.array_equal(kfmi_mod.revcomp(kfmi_mod.revcomp(acgt)), acgt)


def test_revcomp_large_batch_over_the_host_workers(kfmi_mod):
    rng = np.random.default_rng(9)
    q = ACGT[rng.integers(0, 4, size=(50_003, 101))]          # above the single-thread threshold
    assert np.array_equal(kfmi_mod.revcomp(q), revcomp_def(q))


@pytest.mark.parametrize("k", [1, 2, 4])
def test_code_word_identity_equals_the_host_packer_on_the_reverse_complement(kfmi_mod, k):
    """S' = ~pairreverse_m(S) (kfmi_strands.h, the code strand_words_kernel
    runs, here on the host): from the forward words alone, a reverse task's
    words are the host packer's words of revcomp(read) -- every m in 1 .. 300
    (every remainder m % K, windows at and off word boundaries), REV and BOTH."""
    K = kfmi_mod
    rng = np.random.default_rng(k)
    for m in range(1, 301):
        q = np.frombuffer(b"ACGTNacgtnRx", np.uint8)[rng.integers(0, 12, size=(37, m))]
        fwd, rev = K.pack_queries_k(q, k), K.pack_queries_k(K.revcomp(q), k)
        assert np.array_equal(K.strand_words_host(fwd, m, k, K.STRAND_REV), rev), m
        both = K.strand_words_host(fwd, m, k, K.STRAND_BOTH)
        assert np.array_equal(both[:, 0::2], fwd) and np.array_equal(both[:, 1::2], rev), m


def test_code_word_identity_argument_errors(kfmi_mod):
    K = kfmi_mod
    w = np.zeros((7, 4), np.uint32)
    for k, strands in ((3, K.STRAND_REV), (2, K.STRAND_FWD), (2, 0)):
        with pytest.raises(K.KfmiError) as e:
            K.strand_words_host(w, 100, k, strands)
        assert e.value.code == 33


@pytest.mark.parametrize("maxw", [8, 16])
def test_register_form_equals_the_host_packer_on_the_reverse_complement(kfmi_mod, maxw):
    """reverse_stream<MAXW> (kfmi_strands.h), the register form that the fused
    strand kernel and the whole-row strand pack run, here on the host: from a
    read's forward words in MAXW registers (zero above base m-1) it gives the
    host packer's words of revcomp(read), zero words above them -- every m the
    form takes, 1 .. 16 * MAXW (every shift m % 16, every count of whole words
    shifted out)."""
    K = kfmi_mod
    rng = np.random.default_rng(maxw)

    def padded(words):
        out = np.zeros((maxw, words.shape[1]), np.uint32)
        out[:words.shape[0]] = words
        return out

    for m in range(1, 16 * maxw + 1):
        q = np.frombuffer(b"ACGTNacgtnRx", np.uint8)[rng.integers(0, 12, size=(37, m))]
        fwd, rev = padded(K.pack_queries_k(q, 1)), padded(K.pack_queries_k(K.revcomp(q), 1))
        got = K.reverse_stream_host(fwd, m, maxw)
        assert got.shape == rev.shape and np.array_equal(got, rev), m


def test_register_form_argument_errors(kfmi_mod):
    K = kfmi_mod
    for maxw, m in ((4, 16), (12, 16), (32, 16), (8, 129), (16, 257), (8, 0)):
        with pytest.raises(K.KfmiError) as e:
            K.reverse_stream_host(np.zeros((maxw, 3), np.uint32), m, maxw)
        assert e.value.code == 33, (maxw, m)
    with pytest.raises(K.KfmiError) as e:                    # fewer rows than registers
        K.reverse_stream_host(np.zeros((8, 3), np.uint32), 100, 16)
    assert e.value.code == 33


@pytest.fixture(scope="module")
def indexes(kfmi_mod):
    t = texts()["dup"]
    idx = {k: kfmi_mod.Index.build(t.tobytes(), k=k, d=64) for k in (1, 2, 3, 4)}
    yield idx
    for i in idx.values():
        i.close()


@pytest.mark.parametrize("m", [16, 17, 100, 101])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_cpu_search_both_strands(kfmi_mod, oracle_mod, indexes, k, m):
    K = kfmi_mod
    t = texts()["dup"]
    q = strand_reads(t, m, seed=m * 7 + k)
    rq = K.revcomp(q)
    idx = indexes[k]
    # m % K != 0: the true interval, which is the K = 1 oracle's
    img = (indexes[1] if m % k else idx).image()
    want_f, want_r = oracle_mod.search(img, q)[0], oracle_mod.search(img, rq)[0]
    # both strands have matches: all-empty reverse results cannot pass
    for w in (want_f, want_r):
        assert np.count_nonzero(w[1::2] > w[0::2]) >= q.shape[0] // 4
    fwd, rev = K.search_cpu_array(idx, q, nthreads=3), K.search_cpu_array(idx, rq, nthreads=3)
    assert np.array_equal(fwd, want_f) and np.array_equal(rev, want_r)
    both = K.search_cpu_array(idx, q, nthreads=3, strands=K.STRAND_BOTH).reshape(-1, 2)
    assert both.shape[0] == 2 * q.shape[0]
    assert np.array_equal(both[0::2].ravel(), fwd)
    assert np.array_equal(both[1::2].ravel(), rev)
    assert np.array_equal(K.search_cpu_array(idx, q, nthreads=2, strands=K.STRAND_REV), rev)
    assert np.array_equal(K.search_cpu_array(idx, q, nthreads=2, strands=K.STRAND_FWD), fwd)


def test_cpu_search_alt_counters_take_no_remainder(kfmi_mod, indexes):
    K = kfmi_mod
    ac = indexes[2].alt_counters()[0]
    q = strand_reads(texts()["dup"], 101, seed=1)
    with pytest.raises(K.KfmiError) as e:
        K.search_cpu_array(ac, q, strands=K.STRAND_BOTH)
    assert e.value.code == 33
    q = strand_reads(texts()["dup"], 100, seed=1)
    both = K.search_cpu_array(ac, q, strands=K.STRAND_BOTH).reshape(-1, 2)
    assert np.array_equal(both[1::2].ravel(), K.search_cpu_array(ac, K.revcomp(q)))
    ac.close()


def test_argument_errors(kfmi_mod, indexes):
    K = kfmi_mod
    L = K.load()
    q = strand_reads(texts()["dup"], 100, seed=2)[:64]
    Q = K.Queries.from_array(q)
    R1, R2 = K.Results.alloc(64), K.Results.alloc(128)
    try:
        for strands in (0, 4):
            assert L.kfmi_search_cpu_strands(indexes[2].ptr, Q.ptr, R2.ptr, strands, 1) == 33
            assert L.kfmi_search_strands(indexes[2].ptr, Q.ptr, R2.ptr, strands) == 33
            out = np.zeros(4 * 64, np.uint32)
            assert L.kfmi_search_stream_strands(indexes[2].ptr, q.ctypes.data, 64, 100, out.ctypes.data, 0,
                                                strands) == 33
        assert L.kfmi_search_cpu_strands(indexes[2].ptr, Q.ptr, R1.ptr, K.STRAND_BOTH, 1) == 33
        assert L.kfmi_search_strands(indexes[2].ptr, Q.ptr, R1.ptr, K.STRAND_BOTH) == 33
        assert L.kfmi_search_strands(indexes[2].ptr, Q.ptr, R2.ptr, K.STRAND_REV) == 33
        assert L.kfmi_search_cpu_strands(indexes[2].ptr, Q.ptr, R1.ptr, K.STRAND_REV, 1) == 0
        assert L.kfmi_search_cpu_strands(indexes[2].ptr, Q.ptr, R2.ptr, K.STRAND_BOTH, 1) == 0
    finally:
        for h in (Q, R1, R2):
            h.close()
