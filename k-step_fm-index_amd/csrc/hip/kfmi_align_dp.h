/*
 * kfmi_align_dp.h -- the banded edit distance of kfmi_align_seeds, bit-parallel
 * (Myers 1999 in Hyyro's banded form): one candidate, the whole band of a row
 * in one 32-bit word.  Plain integer code, so the same text compiles for the
 * device and -- for checking it against the definition -- for the host.
 *
 * Orientation.  The kernel runs the definition's rows from i = m down to 0: row
 * t = m - i has consumed the read's last t bases, which are the low bits of the
 * code words (reversed index t - 1 at bits 2 (t - 1)), against the text's word
 * stream, whose low bits are the text's last bases too.  With off = n - o - m,
 * cell (i, d) stands at the stream boundary c = off + t - d: c stream bases lie
 * below it.  Bit k of a row's words is the cell d = w - k, so that the cell a
 * skipped text base leads to (d + 1) is the next lower bit, the cell a dropped
 * read base comes from (row t - 1, d - 1) is bit k + 1 of the previous row and
 * the diagonal keeps its bit.  Shifting the previous row's deltas right by one
 * turns this into Myers' column step with a carry-in of +1 at bit 0; bit 2w of
 * the shifted deltas is set to +1, which stands for the +infinity above the
 * band (a +1 there never beats the diagonal).
 *
 * A row is its deltas: bit k of vp / vn set iff cell k holds one more / one
 * less than cell k - 1; s0 is the value of cell 0 (d = w).  Bits above 2w hold
 * garbage that never reaches the bits below: carries and shifts move up only,
 * and the one shift down is overwritten at bit 2w.
 *
 * Text ends.  Cells with c < 0 (past the text's end) are computed as if the
 * stream went on below bit 0 with bases that match nothing: `low` cells of the
 * first row, one fewer per row, get no match bit.  Every cell with c >= 0 then
 * holds the definition's value -- a path from c < 0 enters through a cell at
 * c = 0 of some row t, whose value t the chain of dropped read bases from
 * (0, c = 0) gives as well -- and the caller leaves the cells with c < 0 out of
 * row m.  Cells with c > n (before the text's start) are fed by nothing valid
 * and feed nothing valid (a cell's three neighbours stand at c or c - 1); the
 * caller leaves them out too.
 *
 * The match bits of a row come from two bit planes of the text window (bit 0
 * and bit 1 of every base, 64 bases each), shifted down one base per row and
 * refilled with one stream word per 16 rows: bit k of a plane's low word is
 * the base below boundary c of cell k.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KFMI_DP_FN __device__ __forceinline__
#else
#define KFMI_DP_FN static inline
#endif

namespace kfmi {

/* the even bits of x, gathered into the low 16 */
KFMI_DP_FN uint32_t even_bits(uint32_t x)
{
  x &= 0x55555555u;
  x = (x | (x >> 1)) & 0x33333333u;
  x = (x | (x >> 2)) & 0x0F0F0F0Fu;
  x = (x | (x >> 4)) & 0x00FF00FFu;
  return (x | (x >> 8)) & 0x0000FFFFu;
}

/* Row m of one candidate, every row handed to `keep(t - 1, vp, hp, eq)`, t = 1
 * .. m in this order (kfmi_path_dp.h says what the three words are).  cw: the
 * read's code words; tx: the stream words from the one that holds base off - w
 * of a stream with 16 bases in front (tx[j] is word (off + 16 - w) / 16 + j - 1
 * of the stream, 0 where that is no word of the text); sh = (off + 16 - w) % 16;
 * low = max(w - off, 0). */
template <int MAXW, class Keep>
KFMI_DP_FN void band_rows_keep(const uint32_t (&cw)[MAXW], const uint32_t (&tx)[MAXW + 3], uint32_t m, uint32_t w,
                               uint32_t sh, uint32_t low, Keep& keep, uint32_t& vp_out, uint32_t& vn_out,
                               uint32_t& s0_out)
{
  const uint32_t top = 1u << (2u * w), nw = (m + 15u) >> 4;
  uint32_t vp = 0u, vn = 0u, s0 = 0u;
  int32_t live = (int32_t) (0xFFFFFFFFu << low);   /* cells with a text base below them; one more per row */
  uint32_t a0 = even_bits(tx[0]) | (even_bits(tx[1]) << 16), b0 = even_bits(tx[2]) | (even_bits(tx[3]) << 16);
  uint32_t a1 = even_bits(tx[0] >> 1) | (even_bits(tx[1] >> 1) << 16);
  uint32_t b1 = even_bits(tx[2] >> 1) | (even_bits(tx[3] >> 1) << 16);
  a0 = (uint32_t) ((((uint64_t) b0 << 32) | a0) >> sh);
  a1 = (uint32_t) ((((uint64_t) b1 << 32) | a1) >> sh);
  b0 >>= sh;
  b1 >>= sh;
#pragma unroll
  for (int j = 0; j < MAXW; ++j)
    if ((uint32_t) j < nw) {
      if (j > 0) {   /* 16 rows took 16 bases: the next word's go in above them */
        b0 |= even_bits(tx[j + 3]) << (16u - sh);
        b1 |= even_bits(tx[j + 3] >> 1) << (16u - sh);
      }
      uint32_t c = cw[j];
      const uint32_t cnt = m - 16u * (uint32_t) j < 16u ? m - 16u * (uint32_t) j : 16u;
#pragma unroll 1
      for (uint32_t r = 0; r < cnt; ++r) {
        const uint32_t p0 = 0u - (c & 1u), p1 = 0u - ((c >> 1) & 1u);
        const uint32_t eq = ~((a0 ^ p0) | (a1 ^ p1)) & (uint32_t) live;
        const uint32_t pv = (vp >> 1) | top, mv = (vn >> 1) & ~top;
        const uint32_t xv = eq | mv;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        const uint32_t hp = mv | ~(xh | pv);
        const uint32_t ph = (hp << 1) | 1u;
        const uint32_t mh = (pv & xh) << 1;
        s0 += 1u - (xv & 1u);
        vp = mh | ~(xv | ph);
        vn = ph & xv;
        keep(16u * (uint32_t) j + r, vp, hp, eq);
        c >>= 2;
        a0 = (a0 >> 1) | (b0 << 31);
        b0 >>= 1;
        a1 = (a1 >> 1) | (b1 << 31);
        b1 >>= 1;
        live >>= 1;
      }
    }
  vp_out = vp;
  vn_out = vn;
  s0_out = s0;
}

/* ... with no row kept: what kfmi_align_seeds scores a candidate with */
template <int MAXW>
KFMI_DP_FN void band_rows(const uint32_t (&cw)[MAXW], const uint32_t (&tx)[MAXW + 3], uint32_t m, uint32_t w,
                          uint32_t sh, uint32_t low, uint32_t& vp_out, uint32_t& vn_out, uint32_t& s0_out)
{
  auto keep = [](uint32_t, uint32_t, uint32_t, uint32_t) {};
  band_rows_keep<MAXW>(cw, tx, m, w, sh, low, keep, vp_out, vn_out, s0_out);
}

/* The task's running (E, B_min, B_max) updated with row m of one candidate:
 * cell k (d = w - k) begins at o + w - k, valid iff that lies in [0, n]. */
KFMI_DP_FN void band_fold(uint32_t vp, uint32_t vn, uint32_t s0, uint32_t w, uint32_t o, uint32_t n, uint32_t& E,
                          uint32_t& bmin, uint32_t& bmax)
{
  uint32_t v = s0;
#pragma unroll 1
  for (uint32_t k = 0; k <= 2u * w; ++k) {
    if (k) v += ((vp >> k) & 1u) - ((vn >> k) & 1u);
    const int64_t b = (int64_t) o + w - k;
    if (b < 0 || b > (int64_t) n) continue;
    if (v < E) {
      E = v;
      bmin = bmax = (uint32_t) b;
    } else if (v == E) {
      bmin = (uint32_t) b < bmin ? (uint32_t) b : bmin;
      bmax = (uint32_t) b > bmax ? (uint32_t) b : bmax;
    }
  }
}

/* ... leaving out the cells that begin within 2w of X, the begin position already reported (kfmi_align_second): the
 * running (E2, B2_min, B2_max) over the far cells alone, |b - X| > 2w in signed 64-bit arithmetic. */
KFMI_DP_FN void band_fold_far(uint32_t vp, uint32_t vn, uint32_t s0, uint32_t w, uint32_t o, uint32_t n, uint32_t X,
                              uint32_t& E, uint32_t& bmin, uint32_t& bmax)
{
  uint32_t v = s0;
#pragma unroll 1
  for (uint32_t k = 0; k <= 2u * w; ++k) {
    if (k) v += ((vp >> k) & 1u) - ((vn >> k) & 1u);
    const int64_t b = (int64_t) o + w - k, dx = b - (int64_t) X;
    if (b < 0 || b > (int64_t) n || (dx <= 2 * (int64_t) w && dx >= -2 * (int64_t) w)) continue;
    if (v < E) {
      E = v;
      bmin = bmax = (uint32_t) b;
    } else if (v == E) {
      bmin = (uint32_t) b < bmin ? (uint32_t) b : bmin;
      bmax = (uint32_t) b > bmax ? (uint32_t) b : bmax;
    }
  }
}

}  // namespace kfmi
