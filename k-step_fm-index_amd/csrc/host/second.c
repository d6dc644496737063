/*
 * second.c -- second placement and mapping quality on the host (kstep_fmi.h
 * section 2, "second placement / mapping quality"; not in the
 * reference, which stops at intervals).  kfmi_align_second_cpu is the
 * definition written out as a plain full table per candidate -- not the
 * bit-parallel code, and no candidate is skipped for lying near X: `counted`
 * is counted, the far test is made per cell -- on the ASCII text and a full
 * suffix array the caller passes in, no index and no device.  Slots, rows and
 * the scored test are those of verify.c and align.c, the table is align.c's.
 * kfmi_map_quality_cpu runs the arithmetic of kfmi_quality.h over the handles'
 * host arrays.
 */
#include <omp.h>
#include <stdlib.h>

#include "../kfmi_internal.h"
#include "../kfmi_quality.h"

#define SE_INF 0x3FFFFFFFu

/* A(i, d) of the candidate with origin o, all of it: a[i][d + w], SE_INF for invalid cells. */
static void se_table(const uint8_t *text, uint64_t n, const uint8_t *pc, uint32_t m, uint64_t o, uint32_t w,
                     uint32_t (*a)[2 * KFMI_ALIGN_MAX_BAND + 1])
{
  const int64_t W = (int64_t) w;
  int64_t i, d;
  for (d = -W; d <= W; ++d) {
    const int64_t j = (int64_t) o + m + d;
    a[m][d + W] = j >= 0 && j <= (int64_t) n ? 0u : SE_INF;
  }
  for (i = (int64_t) m - 1; i >= 0; --i)
    for (d = W; d >= -W; --d) {
      const int64_t j = (int64_t) o + i + d;
      uint32_t v = SE_INF, c;
      if (j >= 0 && j <= (int64_t) n) {
        if (j < (int64_t) n) {
          c = a[i + 1][d + W] + (pc[i] != base2index(text[j]));
          if (c < v) v = c;
        }
        if (d - 1 >= -W) {                      /* a read base with no text base */
          c = a[i + 1][d - 1 + W] + 1u;
          if (c < v) v = c;
        }
        if (d + 1 <= W && j < (int64_t) n) {    /* a text base skipped */
          c = a[i][d + 1 + W] + 1u;
          if (c < v) v = c;
        }
        if (v > SE_INF) v = SE_INF;
      }
      a[i][d + W] = v;
    }
}

/* One task: p its m bases, iv / sp its S slots, X word x of its hit; writes the record's two words. */
static void se_task(const uint8_t *text, uint64_t n, const uint32_t *sa, uint64_t rows, const uint8_t *p, uint32_t m,
                    const uint32_t *iv, const uint32_t *sp, uint32_t S, uint32_t max_occ, uint32_t band, uint32_t X,
                    uint32_t max_second, uint32_t (*a)[2 * KFMI_ALIGN_MAX_BAND + 1], uint32_t *rec)
{
  uint32_t best = SE_INF, counted = 0, trunc = 0, s, j, k;
  int64_t bmin = 0, bmax = 0;
  uint8_t pc[256];
  rec[0] = KFMI_HIT_NONE;
  rec[1] = 0u;
  if (X == KFMI_HIT_NONE) return;
  for (j = 0; j < m; ++j) pc[j] = (uint8_t) base2index(p[j]);
  for (s = 0; s < S; ++s) {
    const uint64_t L = iv[2 * s], R = iv[2 * s + 1], start = sp[2 * s], len = sp[2 * s + 1];
    uint64_t end, r;
    if (R <= L || L >= rows || len == 0 || start + len > m) continue;
    end = R < rows ? R : rows;
    if (end - L > max_occ) {
      trunc = KFMI_SECOND_TRUNCATED;
      end = L + max_occ;
    }
    for (r = L; r < end; ++r) {
      const uint64_t pos = sa[r];
      int64_t o;
      if (pos >= rows || pos < start || pos - start + m > n) continue;
      o = (int64_t) (pos - start);
      if (o - (int64_t) X > (int64_t) band || (int64_t) X - o > (int64_t) band) ++counted;
      se_table(text, n, pc, m, (uint64_t) o, band, a);
      for (k = 0; k <= 2 * band; ++k) {
        const int64_t b = o + (int64_t) k - (int64_t) band, dx = b - (int64_t) X;
        const uint32_t v = a[0][k];
        if (v >= SE_INF || v > best || (dx <= 2 * (int64_t) band && dx >= -2 * (int64_t) band)) continue;
        if (v < best) {
          best = v;
          bmin = bmax = b;
        } else {
          if (b < bmin) bmin = b;
          if (b > bmax) bmax = b;
        }
      }
    }
  }
  rec[1] = trunc | (counted << KFMI_HIT_SCORED_SHIFT);
  if (best < SE_INF && best <= max_second) {
    rec[0] = (uint32_t) bmin;
    rec[1] |= best | (bmax - bmin > 2 * (int64_t) band ? KFMI_HIT_MULTI : 0u);
  }
}

int32_t kfmi_align_second_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows, void *queries,
                              void *intervals, void *spans, void *hits, void *second, uint32_t max_seeds,
                              uint32_t strands, uint32_t max_occ, uint32_t band, uint32_t max_second, int32_t nthreads)
{
  const kfmi_qrys_t *q = (const kfmi_qrys_t *) queries;
  const kfmi_res_t *ri = (const kfmi_res_t *) intervals, *rs = (const kfmi_res_t *) spans;
  const kfmi_res_t *rh = (const kfmi_res_t *) hits;
  kfmi_res_t *r2 = (kfmi_res_t *) second;
  const int nt = nthreads > 0 ? nthreads : (getenv("OMP_NUM_THREADS") ? omp_get_max_threads() : kfmi_process_cpus());
  const uint32_t S = max_seeds;
  uint32_t ns;
  char *rev = NULL;
  int64_t ntasks, t;
  int failed = 0;
  /* kfmi_seed_tasks_cpu's checks in its order, with the two record handles */
  if (band > KFMI_ALIGN_MAX_BAND) return KFMI_E_BAD_ARGUMENT;
  if (S < 1 || S > 8 || strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (max_occ < 1 || max_occ > KFMI_VERIFY_MAX_OCC) return KFMI_E_BAD_ARGUMENT;
  if (!text || !sa || rows != n + 1 || rows > 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  if (!q || !ri || !rs || !rh || !r2 || ri == rs || rh == ri || rh == rs || (const kfmi_res_t *) r2 == ri ||
      (const kfmi_res_t *) r2 == rs || (const kfmi_res_t *) r2 == rh)
    return KFMI_E_BAD_ARGUMENT;
  if (q->size == 0 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (ri->num != (uint64_t) S * ns * q->num || rs->num != ri->num || rh->num != (uint64_t) ns * q->num ||
      r2->num != rh->num)
    return KFMI_E_BAD_ARGUMENT;
  if (q->num && (!q->h_queries || !ri->h_results || !rs->h_results || !rh->h_results || !r2->h_results))
    return KFMI_E_BAD_ARGUMENT;
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
#pragma omp parallel num_threads(nt)
  {
    uint32_t (*a)[2 * KFMI_ALIGN_MAX_BAND + 1] = malloc(257 * sizeof *a);
    if (!a) {
#pragma omp atomic write
      failed = 1;
    }
#pragma omp for schedule(dynamic, 16)
    for (t = 0; t < ntasks; ++t) {
      const uint64_t r = ns == 2u ? (uint64_t) t >> 1 : (uint64_t) t;
      const int back = strands == KFMI_STRAND_REV || (ns == 2u && (t & 1));
      const uint8_t *p = (const uint8_t *) (back ? rev : q->h_queries) + r * q->size;
      if (a)
        se_task((const uint8_t *) text, n, sa, rows, p, q->size, ri->h_results + 2 * (uint64_t) t * S,
                rs->h_results + 2 * (uint64_t) t * S, S, max_occ, band, rh->h_results[2 * (uint64_t) t], max_second, a,
                r2->h_results + 2 * (uint64_t) t);
    }
    free(a);
  }
  kfmi_big_free(rev);
  if (failed) return KFMI_E_ALLOCATING_RESULTS;
  r2->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}

int32_t kfmi_map_quality_cpu(void *hits, void *second, void *quals, uint32_t strands, uint32_t max_second)
{
  const kfmi_res_t *rh = (const kfmi_res_t *) hits, *r2 = (const kfmi_res_t *) second;
  kfmi_res_t *rq = (kfmi_res_t *) quals;
  const int both = strands == KFMI_STRAND_BOTH;
  uint64_t t;
  int32_t err;
  if (!rh || !r2 || !rq || rq == rh || rq == r2 || rh == r2 || rh->num != r2->num || rh->num != rq->num)
    return KFMI_E_BAD_ARGUMENT;
  err = kfmi_quality_args(rh->num, strands);
  if (err) return err;
  if (rh->num && (!rh->h_results || !r2->h_results || !rq->h_results)) return KFMI_E_BAD_ARGUMENT;
  for (t = 0; t < rh->num; ++t) {
    const uint64_t u = both ? t ^ 1u : t;
    kfmi_quality(rh->h_results + 2 * t, r2->h_results + 2 * t, rh->h_results + 2 * u, r2->h_results + 2 * u, both,
                 both && (t & 1u), max_second, rq->h_results + 2 * t);
  }
  rq->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}
