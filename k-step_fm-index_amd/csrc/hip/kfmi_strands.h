/*
 * kfmi_strands.h -- the reverse strand on code words.
 *
 * A read P of m bases is searched as the reversed 2-bit stream S that the
 * packers write: base m-1-r at bits 2r.  Its reverse strand P' (kstep_fmi.h:
 * P'[j] = 3 - P[m-1-j] on codes) has the stream S' with P'[m-1-r] = 3 - P[r]
 * at bits 2r, and P[r] sits in S at pair m-1-r, so
 *   S' = ~pairreverse_m(S):
 * pair r of S' is the complement of pair m-1-r of S -- word order reversed,
 * the 2-bit pairs of every word reversed, shifted down by 32*W - 2m bits,
 * inverted, zero from pair m on.
 *   With rem = m % K != 0 the packers keep S in two parts: the remainder code
 * (pairs 0 .. rem-1, the remainder table's index) and the K-step stream
 * (pairs rem .. m-1, shifted down).  The identity holds for the whole m-base
 * stream, so S is put together first and S' is split the same way afterwards.
 *
 * Plain integer code for host and device: the device kernels (kfmi_strands.hip,
 * kfmi_kernels.h) and kfmi_strand_words_host, which tests/test_strands_host.py
 * checks against the host packer on the reverse complement, share it.
 */
#ifndef KFMI_STRANDS_H_
#define KFMI_STRANDS_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KFMI_HD __host__ __device__ __forceinline__
#else
#define KFMI_HD static inline
#endif

namespace kfmi {

/* the sixteen 2-bit pairs of a word in reverse order */
KFMI_HD uint32_t pair_reverse(uint32_t x)
{
  const uint32_t y = __builtin_bitreverse32(x);   /* v_bfrev_b32; every pair comes out bit-swapped */
  return ((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1);
}

/* S' of a whole stream held in MAXW words (m <= 16 * MAXW pairs, zero above
 * pair m-1), every index fixed at compile time so the words stay in registers:
 * the words reversed and pair-reversed, then the stream shifted down by the
 * 32 * MAXW - 2m bits that the zero words above base m-1 turned into all-ones
 * pairs (they leave at the bottom, zeros come in at the top).  m is uniform
 * over a wave on the device. */
template <int MAXW>
KFMI_HD void reverse_stream(const uint32_t (&s)[MAXW], uint32_t m, uint32_t (&rv)[MAXW])
{
  uint32_t t[MAXW + 1];
#pragma unroll
  for (int i = 0; i < MAXW; ++i) t[i] = ~pair_reverse(s[MAXW - 1 - i]);
  t[MAXW] = 0u;
  const uint32_t down = 32u * MAXW - 2u * m, sh = down & 31u;
#pragma unroll
  for (int i = 0; i < MAXW; ++i) rv[i] = (uint32_t) ((((uint64_t) t[i + 1] << 32) | t[i]) >> sh);
#pragma unroll 1
  for (uint32_t w = 0; w < (down >> 5); ++w) {
#pragma unroll
    for (int i = 0; i + 1 < MAXW; ++i) rv[i] = rv[i + 1];
    rv[MAXW - 1] = 0u;
  }
}

/* Word k of the m-base stream S of a read whose forward code words are
 * ks(0 .. nwords-1) (the K-step stream, zero above its last pair; ks(k) = 0
 * from nwords on) and rc (the remainder code of its last rem bases). */
template <class F>
KFMI_HD uint32_t stream_word(F ks, uint32_t k, uint32_t rem, uint32_t rc)
{
  if (!rem) return ks(k);
  const uint32_t lo = k ? ks(k - 1) >> (32u - 2u * rem) : rc;
  return (ks(k) << (2u * rem)) | lo;
}

/* Word j of S' = ~pairreverse_m(S): its pairs 16j .. 16j+15 are the pairs
 * m-1-16j down to m-16-16j of S, a 32-bit window of S that starts at bit
 * 2 * (m - 16j - 16) (below bit 0 for the last word of a read whose length is
 * no multiple of 16: those pairs lie past base m-1 and read as zero). */
template <class F>
KFMI_HD uint32_t rev_stream_word(F ks, uint32_t j, uint32_t m, uint32_t rem, uint32_t rc)
{
  if (16u * j >= m) return 0u;
  const uint32_t left = m - 16u * j;   /* pairs of S' from this word on */
  uint32_t win;
  if (left >= 16u) {
    const uint32_t off = 2u * (left - 16u), k = off >> 5, sh = off & 31u;
    const uint32_t lo = stream_word(ks, k, rem, rc);
    win = sh ? (lo >> sh) | (stream_word(ks, k + 1u, rem, rc) << (32u - sh)) : lo;
  } else {
    win = stream_word(ks, 0u, rem, rc) << (2u * (16u - left));
  }
  const uint32_t v = ~pair_reverse(win);
  return left >= 16u ? v : v & ((1u << (2u * left)) - 1u);
}

/* Task t of the ns * n tasks of `strands` (2 = the reverse strand of every read,
 * 3 = both, task 2q + strand): its column of `out` ((nwords + 1 if rem) rows of
 * ns * n words) from the forward code words `in` (same rows of n words, 16 bases
 * per word, row nwords the remainder codes).  A forward task copies its read's
 * column; a reverse one writes S' word by word and splits it into remainder
 * code and K-step stream again.  The body of strand_words_kernel, and of the
 * host restatement kfmi_strand_words_host that the CPU tests call. */
KFMI_HD void strand_words_task(const uint32_t* in, uint64_t n, uint32_t m, uint32_t nwords, uint32_t rem,
                               uint32_t* out, uint32_t strands, uint64_t t)
{
  const uint32_t ns = strands == 3u ? 2u : 1u;
  const uint64_t ncol = (uint64_t) ns * n;
  const uint64_t qi = ns == 2u ? t >> 1 : t;
  const bool rev = ns == 2u ? (t & 1u) != 0u : true;
  if (!rev) {
    for (uint32_t w = 0; w < nwords + (rem ? 1u : 0u); ++w) out[(uint64_t) w * ncol + t] = in[(uint64_t) w * n + qi];
    return;
  }
  auto ks = [&](uint32_t k) { return k < nwords ? in[(uint64_t) k * n + qi] : 0u; };
  const uint32_t rc = rem ? in[(uint64_t) nwords * n + qi] : 0u;
  uint32_t cur = rev_stream_word(ks, 0u, m, rem, rc);
  if (rem) out[(uint64_t) nwords * ncol + t] = cur & ((1u << (2u * rem)) - 1u);
  for (uint32_t w = 0; w < nwords; ++w) {
    uint32_t word = cur;
    if (rem) {
      const uint32_t next = rev_stream_word(ks, w + 1u, m, rem, rc);
      word = (cur >> (2u * rem)) | (next << (32u - 2u * rem));
      cur = next;
    } else if (w + 1u < nwords) {
      cur = rev_stream_word(ks, w + 1u, m, rem, rc);
    }
    out[(uint64_t) w * ncol + t] = word;
  }
}

}  // namespace kfmi

#endif  // KFMI_STRANDS_H_
