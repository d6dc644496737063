"""Reads and restatements shared by the strand tests (test_strands_host.py,
test_strands_gpu.py, test_strands_lengths.py, test_random_worlds.py)."""
import numpy as np

from skip_texts import ACGT

N_READS = 1_024


def code_of(x: np.ndarray) -> np.ndarray:
    """base2index (genFMindex.c:71-84) on a uint8 array."""
    x = x.astype(np.uint32)
    b1, f2 = x & 4, x & 2
    return (b1 | np.where(b1 != 0, f2 ^ 2, f2)) >> 1


def revcomp_def(q: np.ndarray) -> np.ndarray:
    """The definition: P'[j] = "ACGT"[3 - base2index(P[m-1-j])], on uint8 [N, m]."""
    return np.ascontiguousarray(ACGT[3 - code_of(q[:, ::-1])])


def strand_reads(t: np.ndarray, m: int, seed: int, n_reads: int = N_READS) -> np.ndarray:
    """n_reads reads of m bases: half windows of the text, half reverse
    complements of windows (so both strands have non-empty intervals); of each
    half of N_READS, 32 reads carry one changed base at each of the positions 0,
    m-17 and m-1 that the length has, and 48 carry N, lowercase or other bytes.
    Another n_reads (even, 64 at least) scales those groups by n_reads / N_READS,
    rounded down: 6 and 9 of each 96 at 192 reads, 2 and 3 of each 40 at 80."""
    assert n_reads % 2 == 0 and n_reads >= 64, n_reads
    g, o = 32 * n_reads // N_READS, 16 * n_reads // N_READS
    rng = np.random.default_rng(seed)
    win = np.arange(m)[None, :]
    halves = []
    for h in range(2):
        st = rng.integers(0, t.size - m + 1, size=n_reads // 2)
        q = t[st[:, None] + win].copy()
        at = 0
        for pos in sorted({0, m - 17, m - 1}):
            if not 0 <= pos < m:
                continue
            rows = slice(at, at + g)
            q[rows, pos] = ACGT[(np.searchsorted(ACGT, q[rows, pos]) + rng.integers(1, 4, size=g)) % 4]
            at += g
        q[at:at + o, rng.integers(0, m)] = ord("N")
        q[at + o:at + 2 * o] = np.char.lower(q[at + o:at + 2 * o].view("S1")).view(np.uint8)
        q[at + 2 * o:at + 3 * o, rng.integers(0, m, size=3)] = np.frombuffer(b"nRx", np.uint8)
        halves.append(revcomp_def(q) if h else q)
    q = np.empty((n_reads, m), np.uint8)                    # the two halves interleaved: any slice has both
    q[0::2], q[1::2] = halves
    return q
