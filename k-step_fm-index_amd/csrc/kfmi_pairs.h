/*
 * kfmi_pairs.h -- the per-task and per-pair arithmetic of kfmi_mate_windows and
 * kfmi_pair_hits (kstep_fmi.h, "place windows / pairs"): the window a mate's
 * hit implies and the choice of one placement per read.  Plain C on u32 record
 * words, so the host forms (csrc/host/windows.c) and the kernels
 * (csrc/hip/kfmi_window.hip) compile the same text; tests/window_ref.py states
 * it again in numpy.
 *
 * Records are (x, y) pairs in BOTH order: task t = 2q + strand, reads 2p and
 * 2p + 1 mates, so a pair owns the four tasks 4p .. 4p + 3 and the mate task of
 * t -- the other read on the other strand -- is t ^ 3.
 */
#ifndef KFMI_PAIRS_H_
#define KFMI_PAIRS_H_

#include <stdint.h>

#include "kfmi_internal.h"   /* KFMI_PAIR_PROPER, KFMI_PAIR_RESCUED */

#if defined(__HIPCC__)
#define KFMI_PAIR_FN __host__ __device__ __forceinline__
#define KFMI_PAIR_ARGS_FN static inline
#else
#define KFMI_PAIR_FN static inline
#define KFMI_PAIR_ARGS_FN static inline
#endif

#define KFMI_PAIR_NONE   0xFFFFFFFFu
#define KFMI_PAIR_EDITS  0x0000FFFFu
#define KFMI_PAIR_MULTI  0x00010000u

/* What the two pair calls require of their arguments; entries is the handles' size, two per read. */
KFMI_PAIR_ARGS_FN int32_t kfmi_pair_args(uint64_t entries, uint32_t read_len, uint32_t min_frag, uint32_t max_frag)
{
  if (entries % 4u) return KFMI_E_BAD_ARGUMENT;   /* an even number of reads, two tasks each */
  if (read_len < 1u || read_len > 256u || min_frag < read_len || max_frag < min_frag) return KFMI_E_BAD_ARGUMENT;
  if (max_frag - min_frag + 1u > KFMI_WINDOW_MAX_LEN) return KFMI_E_BAD_ARGUMENT;
  return KFMI_SUCCESS;
}

/* forward task at bf, reverse task at br: frag = br + m - bf */
KFMI_PAIR_FN int kfmi_concordant(uint32_t bf, uint32_t br, uint32_t m, uint32_t min_frag, uint32_t max_frag)
{
  const uint64_t frag = (uint64_t) br + m - bf;   /* br >= bf is checked first */
  return br >= bf && frag >= min_frag && frag <= max_frag;
}

/* The window (lo, len) of task t: own = hits[t], mate = hits[t ^ 3], two words each. */
KFMI_PAIR_FN void kfmi_mate_window(uint32_t t, const uint32_t* own, const uint32_t* mate, uint64_t n, uint32_t m,
                                   uint32_t min_frag, uint32_t max_frag, uint32_t mode, uint32_t* win)
{
  const int rev = (int) (t & 1u);
  int64_t lo, hi;
  win[0] = 0u;
  win[1] = 0u;
  if (mate[0] == KFMI_PAIR_NONE) return;
  if (mode == 0u && own[0] != KFMI_PAIR_NONE &&
      (rev ? kfmi_concordant(mate[0], own[0], m, min_frag, max_frag) : kfmi_concordant(own[0], mate[0], m, min_frag, max_frag)))
    return;   /* the task's own hit is concordant already: nothing to rescue */
  if (rev) {
    lo = (int64_t) mate[0] + min_frag - m;
    hi = (int64_t) mate[0] + max_frag - m;
  } else {
    lo = (int64_t) mate[0] + m - max_frag;
    hi = (int64_t) mate[0] + m - min_frag;
  }
  if (lo < 0) lo = 0;
  if (hi > (int64_t) n) hi = (int64_t) n;
  if (lo > hi) return;
  win[0] = (uint32_t) lo;
  win[1] = (uint32_t) (hi - lo + 1);
}

/* The four records of pair p, out[0 .. 8): h and r are the pair's four own hits and rescued records (eight words
 * each, tasks 4p .. 4p + 3).
 *   Orientation k = 0 is (f, r) = (task 0, task 3), k = 1 is (task 2, task 1); each side takes its own hit (source 0)
 * or its rescued record (source 1), never two rescued ones.  The admissible combination with the least (E_f + E_r,
 * s_f + s_r, k, B_f, B_r, s_f) wins; s_f is last so that two combinations that agree on everything before it -- the
 * same places reached with the sources swapped -- do not depend on the order they are tried in. */
KFMI_PAIR_FN void kfmi_pair_choice(const uint32_t* h, const uint32_t* r, uint32_t m, uint32_t min_frag,
                                   uint32_t max_frag, uint32_t* out)
{
  uint64_t best_hi = ~0ull, best_lo = ~0ull;
  uint32_t bk = 0, fx = 0, fy = 0, vx = 0, vy = 0, k, c, q;   /* the chosen combination: orientation, both records */
  int found = 0;
  /* every index below is a constant once the loops are unrolled: the eight-word arrays stay in registers */
  for (k = 0; k < 2u; ++k) {
    const uint32_t f = k ? 2u : 0u, v = k ? 1u : 3u;
    for (c = 0; c < 3u; ++c) {   /* (s_f, s_r) = (0, 0), (0, 1), (1, 0) */
      const uint32_t sf = c == 2u, sr = c == 1u;
      const uint32_t ax = (sf ? r : h)[2u * f], ay = (sf ? r : h)[2u * f + 1u];
      const uint32_t bx = (sr ? r : h)[2u * v], by = (sr ? r : h)[2u * v + 1u];
      uint64_t hi, lo;
      if (ax == KFMI_PAIR_NONE || bx == KFMI_PAIR_NONE) continue;
      if (!kfmi_concordant(ax, bx, m, min_frag, max_frag)) continue;
      hi = (uint64_t) ((ay & KFMI_PAIR_EDITS) + (by & KFMI_PAIR_EDITS)) << 34 | (uint64_t) (sf + sr) << 33 |
           (uint64_t) k << 32 | ax;
      lo = (uint64_t) bx << 1 | sf;
      if (!found || hi < best_hi || (hi == best_hi && lo < best_lo)) {
        found = 1;
        best_hi = hi;
        best_lo = lo;
        bk = k;
        fx = ax;
        fy = (ay & (KFMI_PAIR_EDITS | KFMI_PAIR_MULTI)) | KFMI_PAIR_PROPER | (sf ? KFMI_PAIR_RESCUED : 0u);
        vx = bx;
        vy = (by & (KFMI_PAIR_EDITS | KFMI_PAIR_MULTI)) | KFMI_PAIR_PROPER | (sr ? KFMI_PAIR_RESCUED : 0u);
      }
    }
  }
  if (found) {   /* task q is f for q = 2 k, r for q = 3 - 2 k */
    for (q = 0; q < 4u; ++q) {
      const int isf = q == 2u * bk, isv = q == 3u - 2u * bk;
      out[2u * q] = isf ? fx : (isv ? vx : KFMI_PAIR_NONE);
      out[2u * q + 1u] = isf ? fy : (isv ? vy : 0u);
    }
    return;
  }
  for (q = 0; q < 2u; ++q) {   /* each read alone: the least (E, strand) of its own two hits */
    const uint32_t x0 = h[4u * q], y0 = h[4u * q + 1u], x1 = h[4u * q + 2u], y1 = h[4u * q + 3u];
    const int fw = x0 != KFMI_PAIR_NONE, rv = x1 != KFMI_PAIR_NONE;
    const int s0 = fw && (!rv || (y0 & KFMI_PAIR_EDITS) <= (y1 & KFMI_PAIR_EDITS)), s1 = rv && !s0;
    out[4u * q] = s0 ? x0 : KFMI_PAIR_NONE;
    out[4u * q + 1u] = s0 ? y0 & (KFMI_PAIR_EDITS | KFMI_PAIR_MULTI) : 0u;
    out[4u * q + 2u] = s1 ? x1 : KFMI_PAIR_NONE;
    out[4u * q + 3u] = s1 ? y1 & (KFMI_PAIR_EDITS | KFMI_PAIR_MULTI) : 0u;
  }
}

#endif /* KFMI_PAIRS_H_ */
