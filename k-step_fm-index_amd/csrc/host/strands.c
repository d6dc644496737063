/*
 * strands.c -- the reverse strand on the host (not in the reference, which
 * searches a read as written): kfmi_revcomp_queries writes the reverse
 * complement of every read, and kfmi_search_cpu_strands runs the host search
 * on the read, on its reverse complement or on both (kstep_fmi.h, section 2).
 *
 * The reverse strand of a read P of m bases is defined on codes:
 *   P'[j] = "ACGT"[3 - base2index(P[m-1-j])]
 * so N and every other byte go where base2index sends them (N -> G, lowercase
 * like uppercase) and are complemented from there; P' is always ACGT.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../kfmi_internal.h"

typedef struct {
  const char *in;
  char *out;
  uint64_t q0, q1;     /* reads [q0, q1) */
  uint32_t size;
  uint32_t ostride;    /* read q goes to out row q * ostride + orow ... */
  uint32_t orow;
  int copy_fwd;        /* ... and, when set, the read itself to row q * ostride */
} rc_range;

static void *rc_worker(void *arg)
{
  static const char acgt[4] = { 'A', 'C', 'G', 'T' };
  const rc_range *r = (const rc_range *) arg;
  const uint32_t m = r->size;
  uint64_t q;
  uint32_t j;
  for (q = r->q0; q < r->q1; ++q) {
    const unsigned char *p = (const unsigned char *) r->in + q * m;
    char *o = r->out + (q * r->ostride + r->orow) * m;
    for (j = 0; j < m; ++j) o[j] = acgt[3u - base2index(p[m - 1 - j])];
    if (r->copy_fwd) memcpy(r->out + q * r->ostride * m, p, m);
  }
  return NULL;
}

/* over the host workers like loadQueries; small batches on the calling thread */
static int32_t rc_run(const char *in, uint64_t num, uint32_t size, char *out, uint32_t ostride, uint32_t orow,
                      int copy_fwd)
{
  int nt = kfmi_host_threads(), t;
  rc_range r[64];
  pthread_t th[64];
  if (num * (uint64_t) size < (4u << 20)) nt = 1;
  if ((uint64_t) nt > num) nt = num ? (int) num : 1;
  for (t = 0; t < nt; t++) {
    r[t].in = in;
    r[t].out = out;
    r[t].q0 = num * (uint64_t) t / (uint64_t) nt;
    r[t].q1 = num * (uint64_t) (t + 1) / (uint64_t) nt;
    r[t].size = size;
    r[t].ostride = ostride;
    r[t].orow = orow;
    r[t].copy_fwd = copy_fwd;
  }
  for (t = 1; t < nt; t++)
    if (pthread_create(&th[t], NULL, rc_worker, &r[t])) {
      /* no more threads: the calling thread takes the rest */
      r[t].q1 = num;
      rc_worker(&r[t]);
      nt = t;
      break;
    }
  rc_worker(&r[0]);
  for (t = 1; t < nt; t++) pthread_join(th[t], NULL);
  return KFMI_SUCCESS;
}

int32_t kfmi_revcomp_queries(const char *ascii, uint64_t num, uint32_t size, char *out)
{
  if (size == 0 || ((!ascii || !out) && num)) return KFMI_E_BAD_ARGUMENT;
  return rc_run(ascii, num, size, out, 1, 0, 0);
}

int32_t kfmi_search_cpu_strands(void *index, void *queries, void *results, uint32_t strands, int32_t nthreads)
{
  const kfmi_qrys_t *q = (const kfmi_qrys_t *) queries;
  const kfmi_res_t *r = (const kfmi_res_t *) results;
  kfmi_qrys_t tmp;
  uint32_t ns;
  int32_t err;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (strands == KFMI_STRAND_FWD) return kfmi_search_cpu(index, queries, results, nthreads);
  if (!index || !q || !r || q->size == 0 || (q->num && !q->h_queries)) return KFMI_E_BAD_ARGUMENT;
  ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (r->num < ns * q->num) return KFMI_E_BAD_ARGUMENT;
  /* the host search is not the hot path: the reads of the ns * num tasks are
   * written out (BOTH: read q at row 2q, its reverse strand at 2q + 1) and
   * searched as they stand */
  memset(&tmp, 0, sizeof(tmp));
  tmp.num = ns * q->num;
  tmp.size = q->size;
  tmp.h_queries = (char *) kfmi_big_alloc(tmp.num * tmp.size + 1);
  if (!tmp.h_queries) return KFMI_E_ALLOCATING_MFASTA;
  err = rc_run(q->h_queries, q->num, q->size, tmp.h_queries, ns, ns - 1u, ns == 2u);
  if (!err) err = kfmi_search_cpu(index, &tmp, results, nthreads);
  kfmi_big_free(tmp.h_queries);
  return err;
}
