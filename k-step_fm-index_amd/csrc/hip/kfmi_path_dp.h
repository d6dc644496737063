/*
 * kfmi_path_dp.h -- the alignment path of kfmi_align_paths on top of the banded
 * edit distance of kfmi_align_dp.h: what its row step hands to the keeper of
 * band_rows_keep, the value of a cell of the last row, and the walk that reads
 * the kept rows back.  Plain integer code, so the same text
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
