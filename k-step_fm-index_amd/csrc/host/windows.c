/*
 * windows.c -- window placement and pairing on the host (kstep_fmi.h section
 * 2, "place windows / pairs"; not in the reference, which stops
 * at intervals).  kfmi_place_windows_cpu is the definition written out as a
 * plain table per task on the ASCII text -- no suffix array, no index and no
 * device; kfmi_mate_windows_cpu and kfmi_pair_hits_cpu run the arithmetic of
 * kfmi_pairs.h over the handles' host arrays.  The reverse complements of REV
 * / BOTH are written to a temporary, as verify.c writes them.
 *
 * A[i][j], 0 <= i <= m, lo <= j <= T, is the least number of edits that align
 * P[i .. m) to text beginning at j and ending at or before T, the scan end of
 * the header's "scan bound" (the text's end n, or the window's last position
 * plus m plus min(max_edits, m) where that is smaller: on a 3 Gbase text a
 * table out to n is not an option).  Rows run from i = m down to 0 and only two
 * of them are kept: the record needs row 0 alone.
 */
#include <omp.h>
#include <stdlib.h>
#include <string.h>

#include "../kfmi_internal.h"
#include "../kfmi_pairs.h"

/* One task: p its m bases, (lo, len) its window; cur / nxt hold len + 2 m + 1 cells each. */
static void pw_task(const uint8_t *text, uint64_t n, const uint8_t *p, uint32_t m, uint32_t lo, uint32_t len,
                    uint32_t max_edits, uint32_t *cur, uint32_t *nxt, uint32_t *hit)
{
  const uint32_t K = max_edits < m ? max_edits : m;
  uint64_t hi_b, T, j, cols;
  uint32_t E = 0xFFFFFFFFu, bmin = 0, bmax = 0;
  int64_t i;
  hit[0] = KFMI_HIT_NONE;
  hit[1] = 0;
  if (len == 0 || lo > n) return;
  hi_b = (uint64_t) lo + len - 1 < n ? (uint64_t) lo + len - 1 : n;
  T = hi_b + m + K < n ? hi_b + m + K : n;
  cols = T - lo + 1;                                  /* column c is text position lo + c */
  for (j = 0; j < cols; ++j) nxt[j] = 0;              /* row m: the end is free */
  for (i = (int64_t) m - 1; i >= 0; --i) {
    const uint32_t pc = base2index(p[i]);
    cur[cols - 1] = nxt[cols - 1] + 1u;               /* at T: every read base left has no text base */
    for (j = cols - 1; j-- > 0;) {
      uint32_t best = nxt[j + 1] + (pc != base2index(text[lo + j]));
      if (nxt[j] + 1u < best) best = nxt[j] + 1u;     /* a read base with no text base */
      if (cur[j + 1] + 1u < best) best = cur[j + 1] + 1u;   /* a text base skipped */
      cur[j] = best;
    }
    {
      uint32_t *s = cur;
      cur = nxt;
      nxt = s;
    }
  }
  for (j = lo; j <= hi_b; ++j) {                      /* nxt is row 0 */
    const uint32_t v = nxt[j - lo];
    if (v < E) {
      E = v;
      bmin = bmax = (uint32_t) j;
    } else if (v == E) bmax = (uint32_t) j;
  }
  if (E <= max_edits) {
    hit[0] = bmin;
    hit[1] = E | (bmax > bmin ? KFMI_HIT_MULTI : 0u);
  }
}

int32_t kfmi_place_windows_cpu(const char *text, uint64_t n, void *queries, void *windows, void *hits,
                               uint32_t strands, uint32_t max_edits, int32_t nthreads)
{
  const kfmi_qrys_t *q = (const kfmi_qrys_t *) queries;
  const kfmi_res_t *rw = (const kfmi_res_t *) windows;
  kfmi_res_t *rh = (kfmi_res_t *) hits;
  const int nt = nthreads > 0 ? nthreads : (getenv("OMP_NUM_THREADS") ? omp_get_max_threads() : kfmi_process_cpus());
  uint32_t ns;
  char *rev = NULL;
  int64_t ntasks, t;
  int failed = 0;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (!text || n + 1 > 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  if (!q || !rw || !rh || rw == rh) return KFMI_E_BAD_ARGUMENT;
  if (q->size == 0 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (rw->num != (uint64_t) ns * q->num || rh->num != rw->num) return KFMI_E_BAD_ARGUMENT;
  if (q->num && (!q->h_queries || !rw->h_results || !rh->h_results)) return KFMI_E_BAD_ARGUMENT;
  ntasks = (int64_t) (ns * q->num);
  for (t = 0; t < ntasks; ++t)                        /* the refusal comes before anything is written */
    if (rw->h_results[2 * (uint64_t) t + 1] > KFMI_WINDOW_MAX_LEN) return KFMI_E_BAD_ARGUMENT;
  if (strands != KFMI_STRAND_FWD && q->num) {         /* the host form is not the hot path: P' written out */
    int32_t err;
    rev = (char *) kfmi_big_alloc(q->num * (uint64_t) q->size + 1);
    if (!rev) return KFMI_E_ALLOCATING_MFASTA;
    err = kfmi_revcomp_queries(q->h_queries, q->num, q->size, rev);
    if (err) {
      kfmi_big_free(rev);
      return err;
    }
  }
#pragma omp parallel num_threads(nt)
  {
    const size_t cells = (size_t) KFMI_WINDOW_MAX_LEN + 2u * 256u + 1u;
    uint32_t *rows = (uint32_t *) malloc(2 * cells * sizeof(uint32_t));
    if (!rows) {
#pragma omp atomic write
      failed = 1;
    }
#pragma omp for schedule(dynamic, 64)
    for (t = 0; t < ntasks; ++t) {
      const uint64_t r = ns == 2u ? (uint64_t) t >> 1 : (uint64_t) t;
      const int back = strands == KFMI_STRAND_REV || (ns == 2u && (t & 1));
      const uint8_t *p = (const uint8_t *) (back ? rev : q->h_queries) + r * q->size;
      if (rows)
        pw_task((const uint8_t *) text, n, p, q->size, rw->h_results[2 * (uint64_t) t],
                rw->h_results[2 * (uint64_t) t + 1], max_edits, rows, rows + cells, rh->h_results + 2 * (uint64_t) t);
    }
    free(rows);
  }
  kfmi_big_free(rev);
  if (failed) return KFMI_E_ALLOCATING_RESULTS;
  rh->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}

int32_t kfmi_mate_windows_cpu(uint64_t n, void *hits, void *windows, uint32_t read_len, uint32_t min_frag,
                              uint32_t max_frag, uint32_t mode)
{
  const kfmi_res_t *rh = (const kfmi_res_t *) hits;
  kfmi_res_t *rw = (kfmi_res_t *) windows;
  uint64_t t;
  int32_t err;
  if (!rh || !rw || rh == rw || rh->num != rw->num || mode > 1u || n + 1 > 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  err = kfmi_pair_args(rh->num, read_len, min_frag, max_frag);
  if (err) return err;
  if (rh->num && (!rh->h_results || !rw->h_results)) return KFMI_E_BAD_ARGUMENT;
  for (t = 0; t < rh->num; ++t)
    kfmi_mate_window((uint32_t) (t & 3u), rh->h_results + 2 * t, rh->h_results + 2 * (t ^ 3u), n, read_len, min_frag,
                     max_frag, mode, rw->h_results + 2 * t);
  rw->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}

int32_t kfmi_pair_hits_cpu(void *hits, void *rescued, void *paired, uint32_t read_len, uint32_t min_frag,
                           uint32_t max_frag)
{
  const kfmi_res_t *rh = (const kfmi_res_t *) hits, *rr = (const kfmi_res_t *) rescued;
  kfmi_res_t *rp = (kfmi_res_t *) paired;
  uint64_t p;
  int32_t err;
  if (!rh || !rr || !rp || rp == rh || rp == rr || rh == rr || rh->num != rr->num || rh->num != rp->num)
    return KFMI_E_BAD_ARGUMENT;
  err = kfmi_pair_args(rh->num, read_len, min_frag, max_frag);
  if (err) return err;
  if (rh->num && (!rh->h_results || !rr->h_results || !rp->h_results)) return KFMI_E_BAD_ARGUMENT;
  for (p = 0; p < rh->num / 4; ++p)
    kfmi_pair_choice(rh->h_results + 8 * p, rr->h_results + 8 * p, read_len, min_frag, max_frag, rp->h_results + 8 * p);
  rp->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}
