/*
 * paths.c -- alignment paths on the host (kstep_fmi.h section 2, "align
 * paths"; not in the reference, which stops at intervals): the
 * CIGAR and the end position of every task's placement.  kfmi_align_paths_cpu
 * is the definition written out as a plain full-band table and the walk over
 * it, on the ASCII text -- no suffix array, no index and no device.  The
 * reverse complements of REV / BOTH are written to a temporary, as verify.c
 * writes them.
 *
 * A[i][d + w], 0 <= i <= m, -w <= d <= w, stands at text position j = c + i + d
 * with c = min(B, n - m) the band's centre, and is PA_INF where j is outside
 * [0, n].  Rows run from i = m down to 0, a row from d = w down to -w.
 */
#include <omp.h>
#include <stdlib.h>
#include <string.h>

#include "../kfmi_internal.h"

#define PA_INF 0x3FFFFFFFu
#define PA_BANDW (2 * KFMI_ALIGN_MAX_BAND + 1)

/* One task: p its m bases, B word x of its hit; writes the path record and the task's 2C words. */
static void pa_task(const uint8_t *text, uint64_t n, const uint8_t *p, uint32_t m, uint32_t B, uint32_t w,
                    uint32_t max_edits, uint32_t C, uint32_t *path, uint32_t *cig)
{
  uint32_t A[257][PA_BANDW];
  uint8_t pc[256];
  const int64_t W = (int64_t) w;
  int64_t c, i, d, j;
  uint32_t v, runs = 0, op = 0, len = 0, k;
  path[0] = KFMI_HIT_NONE;
  path[1] = 0;
  memset(cig, 0, 8ull * C);
  if (B == KFMI_HIT_NONE || n < m || B > n) return;
  c = (int64_t) B < (int64_t) (n - m) ? (int64_t) B : (int64_t) (n - m);
  if ((int64_t) B - c > W) return;
  for (k = 0; k < m; ++k) pc[k] = (uint8_t) base2index(p[k]);
  for (i = (int64_t) m; i >= 0; --i)
    for (d = W; d >= -W; --d) {
      uint32_t best = PA_INF, x;
      j = c + i + d;
      if (j >= 0 && j <= (int64_t) n) {
        if (i == (int64_t) m) best = 0;
        else {
          if (j < (int64_t) n) {
            x = A[i + 1][d + W] + (pc[i] != base2index(text[j]));
            if (x < best) best = x;
          }
          if (d - 1 >= -W) {                      /* a read base with no text base */
            x = A[i + 1][d - 1 + W] + 1u;
            if (x < best) best = x;
          }
          if (d + 1 <= W && j < (int64_t) n) {    /* a text base skipped */
            x = A[i][d + 1 + W] + 1u;
            if (x < best) best = x;
          }
          if (best > PA_INF) best = PA_INF;
        }
      }
      A[i][d + W] = best;
    }
  d = (int64_t) B - c;
  v = A[0][d + W];
  if (v >= PA_INF || v > max_edits) return;
  path[1] = v;
  i = 0;
  while (i < (int64_t) m) {
    uint32_t o;
    j = c + i + d;
    if (d + 1 <= W && j < (int64_t) n && A[i][d + 1 + W] + 1u == v) {
      o = 2u;                                     /* D */
      d += 1;
      v -= 1u;
    } else if (d - 1 >= -W && A[i + 1][d - 1 + W] + 1u == v) {
      o = 1u;                                     /* I */
      i += 1;
      d -= 1;
      v -= 1u;
    } else {
      const uint32_t x = pc[i] != base2index(text[j]);   /* the cell is valid and finite: j < n here */
      o = x ? 8u : 7u;                            /* X, = */
      i += 1;
      v -= x;
    }
    if (o == op) ++len;
    else {
      if (len && runs++ < 2 * C) cig[runs - 1] = len << 4 | op;
      op = o;
      len = 1;
    }
  }
  if (len && runs++ < 2 * C) cig[runs - 1] = len << 4 | op;
  path[0] = (uint32_t) (c + (int64_t) m + d);
  if (runs > 2 * C) {
    memset(cig, 0, 8ull * C);
    path[1] |= KFMI_PATH_OVERFLOW;
  }
  path[1] |= runs << KFMI_PATH_RUNS_SHIFT;
}

int32_t kfmi_align_paths_cpu(const char *text, uint64_t n, void *queries, void *hits, void *paths, void *cigars,
                             uint32_t strands, uint32_t band, uint32_t max_edits, uint32_t cigar_entries,
                             int32_t nthreads)
{
  const kfmi_qrys_t *q = (const kfmi_qrys_t *) queries;
  const kfmi_res_t *rh = (const kfmi_res_t *) hits;
  kfmi_res_t *rp = (kfmi_res_t *) paths, *rc = (kfmi_res_t *) cigars;
  const int nt = nthreads > 0 ? nthreads : (getenv("OMP_NUM_THREADS") ? omp_get_max_threads() : kfmi_process_cpus());
  const uint32_t C = cigar_entries;
  uint32_t ns;
  char *rev = NULL;
  int64_t ntasks, t;
  if (band > KFMI_ALIGN_MAX_BAND || C < 1 || C > KFMI_PATH_MAX_ENTRIES) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (!text || n + 1 > 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  if (!q || !rh || !rp || !rc || rp == rh || rc == rh || rc == rp) return KFMI_E_BAD_ARGUMENT;
  if (q->size == 0 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (rh->num != (uint64_t) ns * q->num || rp->num != rh->num || rc->num != (uint64_t) C * rh->num)
    return KFMI_E_BAD_ARGUMENT;
  if (q->num && (!q->h_queries || !rh->h_results || !rp->h_results || !rc->h_results)) return KFMI_E_BAD_ARGUMENT;
  if (strands != KFMI_STRAND_FWD && q->num) {   /* the host form is not the hot path: P' written out */
    int32_t err;
    rev = (char *) kfmi_big_alloc(q->num * (uint64_t) q->size + 1);
    if (!rev) return KFMI_E_ALLOCATING_MFASTA;
    err = kfmi_revcomp_queries(q->h_queries, q->num, q->size, rev);
    if (err) {
      kfmi_big_free(rev);
      return err;
    }
  }
  ntasks = (int64_t) (ns * q->num);
#pragma omp parallel for schedule(static) num_threads(nt)
  for (t = 0; t < ntasks; ++t) {
    const uint64_t r = ns == 2u ? (uint64_t) t >> 1 : (uint64_t) t;
    const int back = strands == KFMI_STRAND_REV || (ns == 2u && (t & 1));
    const uint8_t *p = (const uint8_t *) (back ? rev : q->h_queries) + r * q->size;
    pa_task((const uint8_t *) text, n, p, q->size, rh->h_results[2 * (uint64_t) t], band, max_edits, C,
            rp->h_results + 2 * (uint64_t) t, rc->h_results + 2 * (uint64_t) t * C);
  }
  kfmi_big_free(rev);
  rp->origin = KFMI_RES_FROM_CPU;
  rc->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}
