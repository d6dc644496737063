/*
 * kfmi_window_dp.h -- the unbanded semi-global edit distance of
 * kfmi_place_windows (kstep_fmi.h, "place windows / pairs"), bit-parallel:
 * Myers 1999 in the multi-word form (Hyyro's blocks), one task, a column of the
 * table in NW words of 32 cells.  Plain integer code, so the same text compiles
 * for the device and -- for checking it against the definition -- for the host.
 *
 * Orientation: the suffix direction of kfmi_align_dp.h.  The pattern is
 * reversed, cell k of a column (bit k % 32 of word k / 32) is the read base
 * P[m - 1 - k], which is where the code words hold it (reversed index k at bits
 * 2 (k % 16) of code word k / 16).  The text is consumed from its scan end
 * downwards, one column per text base.  In the definition's terms cell k of the
 * column of text position j is A(m - 1 - k, j): the edits that align P[m-1-k ..
 * m) to text beginning at j.  The row above cell 0 is A(m, j) = 0 for every j,
 * so the horizontal delta fed into the top of each column is 0: the end is
 * free.  The first column is A(i, T) = m - i, all vertical deltas +1.  The
 * bottom cell, bit (m - 1) % 32 of word (m - 1) / 32, is e(j) = A(0, j) once
 * text position j has been consumed; the step returns its horizontal delta.
 *
 * A column is its vertical deltas: bit k of pv / mv set iff cell k holds one
 * more / one less than cell k - 1.  Bits of the last word above bit m - 1 hold
 * garbage that never reaches the bits below: carries and shifts move up only.
 * Words above the last one are not touched (m is uniform over a launch).
 */
#pragma once
#include <stdint.h>

#include "kfmi_align_dp.h"   /* KFMI_DP_FN, even_bits */

namespace kfmi {

/* The four letters' match words: bit k of peq[c][w] set iff the read base of cell 32 w + k has code c.  cw: the
 * read's code words (16 bases each, reversed index r at bits 2 (r % 16) of word r / 16); cells from m on match
 * nothing. */
template <int NW, int MAXW>
KFMI_DP_FN void window_match_words(const uint32_t (&cw)[MAXW], uint32_t m, uint32_t (&peq)[4][NW])
{
  static_assert(MAXW >= 2 * NW, "two code words per word of cells");
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const uint32_t a = cw[2 * w], b = cw[2 * w + 1];
    const uint32_t b0 = even_bits(a) | (even_bits(b) << 16), b1 = even_bits(a >> 1) | (even_bits(b >> 1) << 16);
    const uint32_t left = m > 32u * (uint32_t) w ? m - 32u * (uint32_t) w : 0u;   /* cells of the read from this word on */
    const uint32_t valid = left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u;
    peq[0][w] = ~b1 & ~b0 & valid;
    peq[1][w] = ~b1 & b0 & valid;
    peq[2][w] = b1 & ~b0 & valid;
    peq[3][w] = b1 & b0 & valid;
  }
}

/* The first column: A(i, T) = m - i. */
template <int NW>
KFMI_DP_FN void window_first_column(uint32_t (&pv)[NW], uint32_t (&mv)[NW])
{
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    pv[w] = 0xFFFFFFFFu;
    mv[w] = 0u;
  }
}

/* One column: the text base of code c consumed.  Returns e(j) - e(j + 1), the bottom cell's horizontal delta. */
template <int NW>
KFMI_DP_FN int32_t window_step(const uint32_t (&peq)[4][NW], uint32_t (&pv)[NW], uint32_t (&mv)[NW], uint32_t m,
                               uint32_t c)
{
  const uint32_t last = (m - 1u) >> 5, lb = (m - 1u) & 31u;
  uint32_t hp = 0u, hn = 0u;   /* the horizontal delta into the word: 0 at the top, the end is free */
  int32_t d = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w)
    if ((uint32_t) w <= last) {
      const uint32_t e01 = (c & 1u) ? peq[1][w] : peq[0][w], e23 = (c & 1u) ? peq[3][w] : peq[2][w];
      const uint32_t eq = (c & 2u) ? e23 : e01;
      const uint32_t p = pv[w], n = mv[w];
      const uint32_t xv = eq | n;
      const uint32_t eqc = eq | hn;
      const uint32_t xh = (((eqc & p) + p) ^ p) | eqc;
      uint32_t ph = n | ~(xh | p), mh = p & xh;
      if ((uint32_t) w == last) d = (int32_t) ((ph >> lb) & 1u) - (int32_t) ((mh >> lb) & 1u);
      const uint32_t po = ph >> 31, no = mh >> 31;
      ph = (ph << 1) | hp;
      mh = (mh << 1) | hn;
      pv[w] = mh | ~(xv | ph);
      mv[w] = ph & xv;
      hp = po;
      hn = no;
    }
  return d;
}

/* The task's running (E, B_min, B_max) updated with e(b) = v.  Begin positions arrive in descending order. */
KFMI_DP_FN void window_fold(uint32_t v, uint32_t b, uint32_t& E, uint32_t& bmin, uint32_t& bmax)
{
  if (v < E) {
    E = v;
    bmin = bmax = b;
  } else if (v == E) {
    bmin = b < bmin ? b : bmin;
    bmax = b > bmax ? b : bmax;
  }
}

/* What a task scans.  The window (lo, len) names the begin positions lo .. lo + len - 1, of which those <= n exist:
 * *hi_b is the largest one.  Returns 0 when none does.
 *   The scan bound.  A placement with e edits that begins at b uses at most m + e text bases -- every text base it
 * uses is under a read base or skipped at cost 1 -- so it ends at or before b + m + e.  With K = min(max_edits, m)
 * the scan treats the text as ending at T = min(n, hi_b + m + K).  Cutting the text can only remove placements, so
 * no e(b) gets smaller.  e(b) <= m always (every read base without a text base), so e(b) <= max_edits means e(b) <=
 * K, its placement ends at or before b + m + K <= T and survives the cut: every e(b) <= max_edits is unchanged, and
 * every other e(b) stays above max_edits.  E, B_min and B_max of a record with E <= max_edits are therefore those of
 * the whole text, and a task with E > max_edits has no record either way. */
KFMI_DP_FN int window_scan(uint32_t n, uint32_t lo, uint32_t len, uint32_t m, uint32_t max_edits, uint32_t* hi_b,
                           uint32_t* T)
{
  if (len == 0u || lo > n) return 0;
  const uint64_t hb = (uint64_t) lo + len - 1u < n ? (uint64_t) lo + len - 1u : n;
  const uint64_t t = hb + m + (max_edits < m ? max_edits : m);
  *hi_b = (uint32_t) hb;
  *T = t < n ? (uint32_t) t : n;
  return 1;
}

/* The record of a task from its fold. */
KFMI_DP_FN void window_record(int any, uint32_t E, uint32_t bmin, uint32_t bmax, uint32_t max_edits, uint32_t* x,
                              uint32_t* y)
{
  const int hit = any && E <= max_edits;
  *x = hit ? bmin : 0xFFFFFFFFu;
  *y = hit ? (E | (bmax > bmin ? 0x00010000u : 0u)) : 0u;
}

}  // namespace kfmi
