/*
 * align.c -- seed alignment on the host (kstep_fmi.h section 2, "align seeds";
 * DESIGN.md 5j; not in the reference, which stops at intervals): the best
 * banded edit-distance placement of every task among the text positions its
 * seeds imply.  kfmi_align_seeds_cpu is the definition written out as a plain
 * dynamic programme, on the ASCII text and a full suffix array the caller
 * passes in -- no index and no device.  Tasks, slots, candidates and the scored
 * test are those of verify.c, whose driver (argument checks, reverse
 * complements, the loop over the tasks) runs this file's task function.
 *
 * A(i, d), 0 <= i <= m, -w <= d <= w, stands at text position j = o + i + d
 * and is valid iff 0 <= j <= n: the least edits that align P[i .. m) to text
 * beginning at j.  Rows run from i = m (all zero) down to 0, a row from d = w
 * down to -w, since a skipped text base leads to the cell above in the band.
 */
#include <stdlib.h>

#include "../kfmi_internal.h"

#define AL_INF 0x3FFFFFFFu

/* Row 0 of the candidate with origin o: row[d + w] = A(0, d), AL_INF for invalid cells. */
static void al_row0(const uint8_t *text, uint64_t n, const uint8_t *pc, uint32_t m, uint64_t o, uint32_t w,
                    uint32_t *row)
{
  const int64_t W = (int64_t) w;
  uint32_t nxt[2 * KFMI_ALIGN_MAX_BAND + 1];
  int64_t i, d;
  for (d = -W; d <= W; ++d) {
    const int64_t j = (int64_t) o + m + d;
    row[d + W] = j >= 0 && j <= (int64_t) n ? 0u : AL_INF;
  }
  for (i = (int64_t) m - 1; i >= 0; --i) {
    for (d = -W; d <= W; ++d) nxt[d + W] = row[d + W];
    for (d = W; d >= -W; --d) {
      const int64_t j = (int64_t) o + i + d;
      uint32_t v = AL_INF, c;
      if (j >= 0 && j <= (int64_t) n) {
        if (j < (int64_t) n) {
          c = nxt[d + W] + (pc[i] != base2index(text[j]));
          if (c < v) v = c;
        }
        if (d - 1 >= -W) {                      /* a read base with no text base */
          c = nxt[d - 1 + W] + 1u;
          if (c < v) v = c;
        }
        if (d + 1 <= W && j < (int64_t) n) {    /* a text base skipped */
          c = row[d + 1 + W] + 1u;
          if (c < v) v = c;
        }
        if (v > AL_INF) v = AL_INF;
      }
      row[d + W] = v;
    }
  }
}

/* One task: p its m bases, iv / sp its S slots; writes the record's two words. */
static void al_task(const uint8_t *text, uint64_t n, const uint32_t *sa, uint64_t rows, const uint8_t *p, uint32_t m,
                    const uint32_t *iv, const uint32_t *sp, uint32_t S, uint32_t max_occ, uint32_t band,
                    uint32_t max_edits, uint32_t *hit)
{
  uint32_t best = AL_INF, scored = 0, s, j, k;
  uint64_t bmin = ~0ull, bmax = 0;
  uint32_t row[2 * KFMI_ALIGN_MAX_BAND + 1];
  uint8_t pc[256];
  for (j = 0; j < m; ++j) pc[j] = (uint8_t) base2index(p[j]);
  for (s = 0; s < S; ++s) {
    const uint64_t L = iv[2 * s], R = iv[2 * s + 1], start = sp[2 * s], len = sp[2 * s + 1];
    uint64_t end, r;
    if (R <= L || L >= rows || len == 0 || start + len > m) continue;
    end = R < rows ? R : rows;
    if (L + max_occ < end) end = L + max_occ;
    for (r = L; r < end; ++r) {
      const uint64_t pos = sa[r];
      uint64_t o;
      if (pos >= rows || pos < start || pos - start + m > n) continue;
      o = pos - start;
      al_row0(text, n, pc, m, o, band, row);
      ++scored;
      for (k = 0; k <= 2 * band; ++k) {
        const uint64_t b = o + k - band;   /* valid cells only: 0 <= b <= n */
        if (row[k] >= AL_INF || row[k] > best) continue;
        if (row[k] < best) {
          best = row[k];
          bmin = bmax = b;
        } else {
          if (b < bmin) bmin = b;
          if (b > bmax) bmax = b;
        }
      }
    }
  }
  if (scored && best <= max_edits) {
    hit[0] = (uint32_t) bmin;
    hit[1] = best | (bmax - bmin > 2ull * band ? KFMI_HIT_MULTI : 0u) | (scored << KFMI_HIT_SCORED_SHIFT);
  } else {
    hit[0] = KFMI_HIT_NONE;
    hit[1] = scored << KFMI_HIT_SCORED_SHIFT;
  }
}

int32_t kfmi_align_seeds_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows, void *queries,
                             void *intervals, void *spans, void *hits, uint32_t max_seeds, uint32_t strands,
                             uint32_t max_occ, uint32_t band, uint32_t max_edits, int32_t nthreads)
{
  if (band > KFMI_ALIGN_MAX_BAND) return KFMI_E_BAD_ARGUMENT;
  return kfmi_seed_tasks_cpu(text, n, sa, rows, queries, intervals, spans, hits, max_seeds, strands, max_occ, band,
                             max_edits, nthreads, al_task);
}
