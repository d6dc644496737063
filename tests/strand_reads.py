"""Reads and restatements shared by the strand tests (test_strands_host.py,
test_strands_gpu.py)."""
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


def strand_reads(t: np.ndarray, m: int, seed: int) -> np.ndarray:
    """N_READS reads of m bases: half windows of the text, half reverse
    complements of windows (so both strands have non-empty intervals); of each
    half, 32 reads carry one changed base at each of the positions 0, m-17 and
    m-1 that the length has, and 48 carry N, lowercase or other bytes."""
    rng = np.random.default_rng(seed)
    win = np.arange(m)[None, :]
    halves = []
    for h in range(2):
        st = rng.integers(0, t.size - m + 1, size=N_READS // 2)
        q = t[st[:, None] + win].copy()
        at = 0
        for pos in sorted({0, m - 17, m - 1}):
            if not 0 <= pos < m:
                continue
            rows = slice(at, at + 32)
            q[rows, pos] = ACGT[(np.searchsorted(ACGT, q[rows, pos]) + rng.integers(1, 4, size=32)) % 4]
            at += 32
        q[at:at + 16, rng.integers(0, m)] = ord("N")
        q[at + 16:at + 32] = np.char.lower(q[at + 16:at + 32].view("S1")).view(np.uint8)
        q[at + 32:at + 48, rng.integers(0, m, size=3)] = np.frombuffer(b"nRx", np.uint8)
        halves.append(revcomp_def(q) if h else q)
    q = np.empty((N_READS, m), np.uint8)                    # the two halves interleaved: any slice has both
    q[0::2], q[1::2] = halves
    return q
