/*
 * verify.c -- seed verification on the host (kstep_fmi.h section 2, "verify
 * seeds"; not in the reference, which stops at intervals): the
 * best Hamming placement of every task among the text positions its seeds
 * imply.  kfmi_verify_seeds_cpu is the definition written out once more, on the
 * ASCII text and a full suffix array the caller passes in -- no index and no
 * device -- so the sanitizer harness links it without the HIP layer.
 *
 * Slot s of task t is {L, R} in `intervals` and {start, len} in `spans`.  Its
 * candidates are the rows L, L + 1, .. below min(R, rows, L + max_occ); row r
 * gives p = sa[r] and the origin o = p - start, scored when sa[r] < rows,
 * p >= start and o + m <= n.  Every value a slot holds is checked before it is
 * used as an index, so hand-made handles with garbage are safe.
 */
#include <omp.h>
#include <stdlib.h>

#include "../kfmi_internal.h"

/* One task: p its m bases, iv / sp its S slots; returns the record's two words. */
static void vs_task(const uint8_t *text, uint64_t n, const uint32_t *sa, uint64_t rows, const uint8_t *p, uint32_t m,
                    const uint32_t *iv, const uint32_t *sp, uint32_t S, uint32_t max_occ, uint32_t band,
                    uint32_t max_mism, uint32_t *hit)
{
  uint32_t best_m = 0xFFFFFFFFu, best_o = 0xFFFFFFFFu, multi = 0, scored = 0, s, j;
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
      uint32_t mm = 0;
      if (pos >= rows || pos < start || pos - start + m > n) continue;
      o = pos - start;
      for (j = 0; j < m; ++j) mm += pc[j] != base2index(text[o + j]);
      ++scored;
      if (mm < best_m) {
        best_m = mm;
        best_o = (uint32_t) o;
        multi = 0;
      } else if (mm == best_m && (uint32_t) o != best_o) {   /* another origin with the same count */
        multi = KFMI_HIT_MULTI;
        if ((uint32_t) o < best_o) best_o = (uint32_t) o;
      }
    }
  }
  if (scored && best_m <= max_mism) {
    hit[0] = best_o;
    hit[1] = best_m | multi | (scored << KFMI_HIT_SCORED_SHIFT);
  } else {
    hit[0] = KFMI_HIT_NONE;
    hit[1] = scored << KFMI_HIT_SCORED_SHIFT;
  }
}

/* The argument checks, the reverse complements and the loop over the tasks,
 * shared with kfmi_align_seeds_cpu (align.c): `task` scores one task. */
int32_t kfmi_seed_tasks_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows, void *queries,
                            void *intervals, void *spans, void *hits, uint32_t max_seeds, uint32_t strands,
                            uint32_t max_occ, uint32_t band, uint32_t bound, int32_t nthreads, kfmi_seed_task_fn task)
{
  const kfmi_qrys_t *q = (const kfmi_qrys_t *) queries;
  const kfmi_res_t *ri = (const kfmi_res_t *) intervals, *rs = (const kfmi_res_t *) spans;
  kfmi_res_t *rh = (kfmi_res_t *) hits;
  const int nt = nthreads > 0 ? nthreads : (getenv("OMP_NUM_THREADS") ? omp_get_max_threads() : kfmi_process_cpus());
  const uint32_t S = max_seeds;
  uint32_t ns;
  char *rev = NULL;
  int64_t ntasks, t;
  if (S < 1 || S > 8 || strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (max_occ < 1 || max_occ > KFMI_VERIFY_MAX_OCC) return KFMI_E_BAD_ARGUMENT;
  if (!text || !sa || rows != n + 1 || rows > 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  if (!q || !ri || !rs || !rh || ri == rs || (const kfmi_res_t *) rh == ri || (const kfmi_res_t *) rh == rs)
    return KFMI_E_BAD_ARGUMENT;
  if (q->size == 0 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (ri->num != (uint64_t) S * ns * q->num || rs->num != ri->num || rh->num != (uint64_t) ns * q->num)
    return KFMI_E_BAD_ARGUMENT;
  if (q->num && (!q->h_queries || !ri->h_results || !rs->h_results || !rh->h_results)) return KFMI_E_BAD_ARGUMENT;
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
    task((const uint8_t *) text, n, sa, rows, p, q->size, ri->h_results + 2 * (uint64_t) t * S,
         rs->h_results + 2 * (uint64_t) t * S, S, max_occ, band, bound, rh->h_results + 2 * (uint64_t) t);
  }
  kfmi_big_free(rev);
  rh->origin = KFMI_RES_FROM_CPU;
  return KFMI_SUCCESS;
}

int32_t kfmi_verify_seeds_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows, void *queries,
                              void *intervals, void *spans, void *hits, uint32_t max_seeds, uint32_t strands,
                              uint32_t max_occ, uint32_t max_mism, int32_t nthreads)
{
  return kfmi_seed_tasks_cpu(text, n, sa, rows, queries, intervals, spans, hits, max_seeds, strands, max_occ, 0u,
                             max_mism, nthreads, vs_task);
}
