/*
 * kfmi_path_dp.h -- the alignment path of kfmi_align_paths on top of the banded
 * edit distance of kfmi_align_dp.h: the same row step with every row kept, and
 * the walk that reads the kept rows back.  Plain integer code, so the same text
 * compiles for the device and -- for checking it against the definition -- for
 * the host.  Orientation, bit order, text ends and the match planes are those
 * of kfmi_align_dp.h, with the band's centre c in place of the origin o.
 *
 * What a row keeps.  Row t = m - i, bit k (the cell d = w - k) of three words:
 *   vp  cell k holds one more than cell k - 1 of the same row: the cell a
 *       skipped text base leads to, (i, d + 1), attains it with its +1;
 *   hp  cell k holds one more than cell k + 1 of row t - 1 (Myers' horizontal
 *       +1 before its shift): the cell of a read base with no text base,
 *       (i + 1, d - 1), attains it with its +1;
 *   eq  the read base of the row equals the text base below the cell.
 * The diagonal needs no word: a valid cell's value is the minimum over its
 * transitions, so where neither gap attains it the diagonal does, as `=` under
 * a set eq bit and as `X` otherwise.  No cell's value is needed after row 0,
 * and that one is s0 plus the prefix popcounts of the last row's vp and vn
 * (band_value).
 *
 * Which deltas may be trusted.  Cells past the text's end hold as-if values,
 * cells before its start and bits above 2w hold garbage (kfmi_align_dp.h), so
 * the walk asks positions, never values, whether a transition exists: d + 1 <=
 * w is k >= 1, d - 1 >= -w is k < 2w, and j < n is kept as a running text
 * position.  Each of the three words is then read at a bit whose two cells are
 * both valid: (i, d + 1) and (i + 1, d) stand at j + 1 <= n, (i + 1, d - 1) at
 * j itself.  Bit 2w of hp is the +infinity above the band and is never read.
 *
 * Order.  The rows are computed from t = 1 up and walked from t = m down: the
 * path begins at the read's first base, which the last row holds.
 */
#pragma once
#include <stdint.h>

#include "kfmi_align_dp.h"

namespace kfmi {

/* BAM's codes of the four operations a path holds */
enum : uint32_t { PATH_OP_I = 1u, PATH_OP_D = 2u, PATH_OP_EQ = 7u, PATH_OP_X = 8u };

/* band_rows with every row handed to `keep(t - 1, vp, hp, eq)`, t = 1 .. m in
 * this order; cw, tx, sh and low as for band_rows, and the same last row out. */
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

/* the value of cell k of a row from its deltas; every cell below k is one the row step computed */
KFMI_DP_FN uint32_t band_value(uint32_t vp, uint32_t vn, uint32_t s0, uint32_t k)
{
  const uint32_t mask = ((2u << k) - 1u) & ~1u;   /* bits 1 .. k */
  return s0 + (uint32_t) __builtin_popcount(vp & mask) - (uint32_t) __builtin_popcount(vn & mask);
}

/* The path from cell k of row m (the begin position b = c + w - k, a valid
 * cell) through the kept rows: `row(t - 1, vp, hp, eq)` reads row t back,
 * `run(op, len)` takes the runs in read order.  Per cell the first transition
 * that exists and attains: text base skipped, read base with no text base,
 * diagonal.  Returns the end position, one past the last text base used. */
template <class Row, class Run>
KFMI_DP_FN uint32_t band_walk(uint32_t m, uint32_t w, uint32_t b, uint32_t n, uint32_t k, Row& row, Run& run)
{
  uint32_t j = b, op = 0u, len = 0u;
#pragma unroll 1
  for (uint32_t t = m; t >= 1u; --t) {
    uint32_t vp, hp, eq;
    row(t - 1u, vp, hp, eq);
    uint32_t o;
#pragma unroll 1
    for (;;) {
      if (k >= 1u && j < n && ((vp >> k) & 1u)) {
        o = PATH_OP_D;
        --k;
        ++j;
      } else if (k < 2u * w && ((hp >> k) & 1u)) {
        o = PATH_OP_I;
        ++k;
      } else {
        o = ((eq >> k) & 1u) ? PATH_OP_EQ : PATH_OP_X;
        ++j;
      }
      if (o == op) ++len;
      else {
        if (len) run(op, len);
        op = o;
        len = 1u;
      }
      if (o != PATH_OP_D) break;   /* a read base is taken: the next row */
    }
  }
  if (len) run(op, len);
  return j;
}

}  // namespace kfmi
