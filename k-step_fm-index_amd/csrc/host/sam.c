/*
 * sam.c -- SAM lines on the host (kstep_fmi.h section 2, "SAM lines"; DESIGN.md
 * 5o; not in the reference, which stops at intervals): the contig table, the
 * header, the handle of a batch's text, and kfmi_sam_lines_cpu, which is the
 * definition on the handles' host arrays and the ASCII text -- OpenMP over the
 * reads, a length pass, a prefix sum, a write pass; no index and no device.
 * The arithmetic of a line is kfmi_sam.h's, which the kernels compile too.  The
 * reverse complements of REV / BOTH are written to a temporary, as paths.c
 * writes them.
 */
#include <omp.h>
#include <stdlib.h>
#include <string.h>

#include "../kfmi_internal.h"

typedef struct {
  const uint8_t *text;
} kfmi_sam_src;
#define KFMI_SAM_TEXT(src, p) base2index((src).text[p])
#include "../kfmi_sam.h"

/* ---- the contig table ---- */

int32_t kfmi_contigs_create(const char *names, const uint32_t *begins, const uint32_t *lengths, uint32_t count,
                            void **contigs)
{
  kfmi_contigs_t *c;
  const char *s = names;
  uint64_t bytes = 0;
  uint32_t i;
  if (!names || !begins || !lengths || !contigs || count == 0) return KFMI_E_BAD_ARGUMENT;
  for (i = 0; i < count; ++i) {   /* every check before anything is made */
    const size_t len = strnlen(s, 255);
    size_t k;
    if (len == 0 || len > 254) return KFMI_E_BAD_ARGUMENT;
    for (k = 0; k < len; ++k)
      if ((unsigned char) s[k] < 33 || (unsigned char) s[k] > 126) return KFMI_E_BAD_ARGUMENT;
    if (lengths[i] == 0 || (uint64_t) begins[i] + lengths[i] > 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
    if (i + 1 < count && (uint64_t) begins[i] + lengths[i] > begins[i + 1]) return KFMI_E_BAD_ARGUMENT;
    bytes += len;
    s += len + 1;
  }
  c = (kfmi_contigs_t *) calloc(1, sizeof *c);
  if (!c) return KFMI_E_ALLOCATING_RESULTS;
  c->begins = (uint32_t *) malloc(4ull * count);
  c->lengths = (uint32_t *) malloc(4ull * count);
  c->name_off = (uint32_t *) malloc(4ull * count + 4);
  c->names = (char *) malloc(bytes);
  if (!c->begins || !c->lengths || !c->name_off || !c->names) {
    free(c->begins);
    free(c->lengths);
    free(c->name_off);
    free(c->names);
    free(c);
    return KFMI_E_ALLOCATING_RESULTS;
  }
  c->count = count;
  memcpy(c->begins, begins, 4ull * count);
  memcpy(c->lengths, lengths, 4ull * count);
  s = names;
  bytes = 0;
  for (i = 0; i < count; ++i) {
    const size_t len = strlen(s);
    c->name_off[i] = (uint32_t) bytes;
    memcpy(c->names + bytes, s, len);
    bytes += len;
    s += len + 1;
  }
  c->name_off[count] = (uint32_t) bytes;
  pthread_mutex_init(&c->mu, NULL);
  *contigs = c;
  return KFMI_SUCCESS;
}

int32_t kfmi_contigs_free(void **contigs)
{
  kfmi_contigs_t *c = contigs ? (kfmi_contigs_t *) *contigs : NULL;
  if (!c) return KFMI_SUCCESS;
  if (c->d_mem && c->d_free) c->d_free(c->d_mem, c->d_device);
  pthread_mutex_destroy(&c->mu);
  free(c->begins);
  free(c->lengths);
  free(c->name_off);
  free(c->names);
  free(c);
  *contigs = NULL;
  return KFMI_SUCCESS;
}

int64_t kfmi_sam_header(void *contigs, char *buf, uint64_t cap)
{
  static const char hd[] = "@HD\tVN:1.6\tSO:unknown\n";
  const kfmi_contigs_t *c = (const kfmi_contigs_t *) contigs;
  uint64_t need = sizeof hd - 1, pos;
  uint32_t i;
  if (!c) return -(int64_t) KFMI_E_BAD_ARGUMENT;
  for (i = 0; i < c->count; ++i)   /* "@SQ\tSN:" 7, "\tLN:" 4, the newline */
    need += 12u + (c->name_off[i + 1] - c->name_off[i]) + kfmi_sam_digits(c->lengths[i]);
  if (!buf || cap < need) return (int64_t) need;
  memcpy(buf, hd, sizeof hd - 1);
  pos = sizeof hd - 1;
  for (i = 0; i < c->count; ++i) {
    const uint32_t len = c->name_off[i + 1] - c->name_off[i];
    memcpy(buf + pos, "@SQ\tSN:", 7);
    memcpy(buf + pos + 7, c->names + c->name_off[i], len);
    memcpy(buf + pos + 7 + len, "\tLN:", 4);
    pos += 11u + len;
    pos += kfmi_sam_put_dec((uint8_t *) buf + pos, 0u, c->lengths[i]);
    buf[pos++] = '\n';
  }
  return (int64_t) need;
}

/* ---- the handle of a batch's text ---- */

kfmi_sam_t *kfmi_sam_alloc(uint64_t num)
{
  kfmi_sam_t *s = (kfmi_sam_t *) calloc(1, sizeof *s);
  if (!s) return NULL;
  s->h_off = (uint64_t *) calloc(num + 1, 8);
  if (!s->h_off) {
    free(s);
    return NULL;
  }
  s->num = num;
  pthread_mutex_init(&s->mu, NULL);
  return s;
}

uint64_t kfmi_sam_num(void *sam) { return sam ? ((kfmi_sam_t *) sam)->num : 0; }
uint64_t kfmi_sam_bytes(void *sam) { return sam ? ((kfmi_sam_t *) sam)->bytes : 0; }
const uint64_t *kfmi_sam_offsets(void *sam) { return sam ? ((kfmi_sam_t *) sam)->h_off : NULL; }

const char *kfmi_sam_text(void *sam)
{
  kfmi_sam_t *s = (kfmi_sam_t *) sam;
  if (!s) return NULL;
  pthread_mutex_lock(&s->mu);
  if (!s->h_text) {
    char *t = (char *) kfmi_big_alloc(s->bytes + 1);
    if (t && s->bytes && (!s->d_text || !s->d_fetch || s->d_fetch(s->d_text, s->d_device, t, s->bytes))) {
      kfmi_big_free(t);
      t = NULL;
    }
    s->h_text = t;
  }
  pthread_mutex_unlock(&s->mu);
  return s->h_text;
}

int32_t kfmi_sam_free(void **sam)
{
  kfmi_sam_t *s = sam ? (kfmi_sam_t *) *sam : NULL;
  if (!s) return KFMI_SUCCESS;
  if (s->d_text && s->d_free) s->d_free(s->d_text, s->d_device);
  pthread_mutex_destroy(&s->mu);
  kfmi_big_free(s->h_text);
  free(s->h_off);
  free(s);
  *sam = NULL;
  return KFMI_SUCCESS;
}

/* ---- kfmi_sam_lines_cpu ---- */

typedef struct {
  const uint8_t *text, *fwd, *rev;   /* rev: the reads' reverse complements, NULL under FWD */
  const uint32_t *hits, *paths, *cigars, *quals;
  kfmi_sam_table tab;
  uint64_t name_base;
  uint32_t n, m, band, C, options, strands;
} sam_job;

/* Read q's line: its length, and its bytes at dst where dst is not NULL. */
static uint32_t sam_read_line(const sam_job *j, uint64_t q, uint8_t *dst)
{
  const int both = j->strands == KFMI_STRAND_BOTH;
  const uint32_t ns = both ? 2u : 1u, m = j->m;
  uint32_t st[2] = {0, 0}, ed[2] = {0, 0}, contig[2] = {0, 0}, s, choice = 0, pos = 0, k;
  kfmi_sam_runs walk[2];
  uint64_t t = 0;
  int rev = 0;
  for (s = 0; s < ns; ++s) {
    const uint64_t u = ns * q + s;
    st[s] = kfmi_sam_status(&j->tab, j->n, m, j->band, j->C, j->options, j->hits[2 * u], j->paths[2 * u],
                            j->paths[2 * u + 1], j->cigars + 2 * u * j->C, &contig[s], &walk[s]);
    ed[s] = j->paths[2 * u + 1] & KFMI_PATH_EDITS_MASK;
  }
  for (s = 0; s < ns; ++s) {   /* the one task of the read that writes */
    const int r = both ? (int) s : j->strands == KFMI_STRAND_REV;
    const uint32_t c = kfmi_sam_choice(both, r, st[s], ed[s], st[s ^ 1u], ed[s ^ 1u]);
    if (c) {
      choice = c;
      t = ns * q + s;
      rev = r;
      break;
    }
  }
  s = (uint32_t) (t - ns * q);
  if (choice & KFMI_SAM_MAPPED) {
    const uint32_t mapq = kfmi_sam_mapq(j->quals != NULL, j->quals ? j->quals[2 * t] : 0u), B = j->hits[2 * t];
    const uint32_t runs = (j->paths[2 * t + 1] >> KFMI_PATH_RUNS_SHIFT) & KFMI_PATH_RUNS_MASK;
    const uint8_t *p = (rev ? j->rev : j->fwd) + q * m;
    const kfmi_sam_src src = {j->text};
    if (!dst) return kfmi_sam_mapped_len(&j->tab, contig[s], j->name_base + q, rev, B, mapq, m, ed[s], &walk[s]);
    pos = kfmi_sam_put_front(dst, 0, &j->tab, contig[s], j->name_base + q, rev, B, mapq, j->cigars + 2 * t * j->C, runs,
                             j->options);
    for (k = 0; k < m; ++k) dst[pos++] = kfmi_sam_letter(base2index(p[k]));
    return kfmi_sam_put_back(dst, pos, ed[s], j->cigars + 2 * t * j->C, runs, B, src);
  }
  if (!dst) return kfmi_sam_unmapped_len(j->name_base + q, m);
  pos = kfmi_sam_put_unmapped_front(dst, 0, j->name_base + q);
  for (k = 0; k < m; ++k) dst[pos++] = kfmi_sam_letter(base2index(j->fwd[q * m + k]));
  return kfmi_sam_put_unmapped_back(dst, pos, choice >> KFMI_SAM_CODE_SHIFT);
}

int32_t kfmi_sam_lines_cpu(const char *text, uint64_t n, void *queries, void *contigs, void *hits, void *paths,
                           void *cigars, void *quals, uint32_t strands, uint32_t cigar_entries, uint32_t band,
                           uint32_t options, uint64_t name_base, int32_t nthreads, void **sam)
{
  const kfmi_qrys_t *q = (const kfmi_qrys_t *) queries;
  const kfmi_contigs_t *ct = (const kfmi_contigs_t *) contigs;
  const kfmi_res_t *rh = (const kfmi_res_t *) hits, *rp = (const kfmi_res_t *) paths;
  const kfmi_res_t *rc = (const kfmi_res_t *) cigars, *rq = (const kfmi_res_t *) quals;
  const int nt = nthreads > 0 ? nthreads : (getenv("OMP_NUM_THREADS") ? omp_get_max_threads() : kfmi_process_cpus());
  const uint32_t C = cigar_entries;
  uint32_t ns;
  char *rev = NULL;
  kfmi_sam_t *s;
  sam_job j;
  int64_t num, i;
  if (band > KFMI_ALIGN_MAX_BAND || C < 1 || C > KFMI_PATH_MAX_ENTRIES) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (options & ~KFMI_SAM_CIGAR_M) return KFMI_E_BAD_ARGUMENT;
  if (!text || n + 1 > 0xFFFFFFFFull || !sam) return KFMI_E_BAD_ARGUMENT;
  if (!q || !ct || !rh || !rp || !rc || rp == rh || rc == rh || rc == rp) return KFMI_E_BAD_ARGUMENT;
  if (rq && (rq == rh || rq == rp || rq == rc)) return KFMI_E_BAD_ARGUMENT;
  if (q->size == 0 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (rh->num != (uint64_t) ns * q->num || rp->num != rh->num || rc->num != (uint64_t) C * rh->num)
    return KFMI_E_BAD_ARGUMENT;
  if (rq && rq->num != rh->num) return KFMI_E_BAD_ARGUMENT;
  if (name_base + q->num < name_base) return KFMI_E_BAD_ARGUMENT;
  if ((uint64_t) ct->begins[ct->count - 1] + ct->lengths[ct->count - 1] > n) return KFMI_E_BAD_ARGUMENT;
  if (q->num && (!q->h_queries || !rh->h_results || !rp->h_results || !rc->h_results || (rq && !rq->h_results)))
    return KFMI_E_BAD_ARGUMENT;
  if (strands != KFMI_STRAND_FWD && q->num) {
    int32_t err;
    rev = (char *) kfmi_big_alloc(q->num * (uint64_t) q->size + 1);
    if (!rev) return KFMI_E_ALLOCATING_MFASTA;
    err = kfmi_revcomp_queries(q->h_queries, q->num, q->size, rev);
    if (err) {
      kfmi_big_free(rev);
      return err;
    }
  }
  s = kfmi_sam_alloc(q->num);
  if (!s) {
    kfmi_big_free(rev);
    return KFMI_E_ALLOCATING_RESULTS;
  }
  j.text = (const uint8_t *) text;
  j.fwd = (const uint8_t *) q->h_queries;
  j.rev = (const uint8_t *) rev;
  j.hits = rh->h_results;
  j.paths = rp->h_results;
  j.cigars = rc->h_results;
  j.quals = rq ? rq->h_results : NULL;
  j.tab.begins = ct->begins;
  j.tab.lengths = ct->lengths;
  j.tab.name_off = ct->name_off;
  j.tab.names = (const uint8_t *) ct->names;
  j.tab.count = ct->count;
  j.name_base = name_base;
  j.n = (uint32_t) n;
  j.m = q->size;
  j.band = band;
  j.C = C;
  j.options = options;
  j.strands = strands;
  num = (int64_t) q->num;
#pragma omp parallel for schedule(static) num_threads(nt)
  for (i = 0; i < num; ++i) s->h_off[i + 1] = sam_read_line(&j, (uint64_t) i, NULL);
  for (i = 0; i < num; ++i) s->h_off[i + 1] += s->h_off[i];
  s->bytes = s->h_off[num];
  s->h_text = (char *) kfmi_big_alloc(s->bytes + 1);
  if (!s->h_text) {
    kfmi_big_free(rev);
    kfmi_sam_free((void **) &s);
    return KFMI_E_ALLOCATING_RESULTS;
  }
#pragma omp parallel for schedule(static) num_threads(nt)
  for (i = 0; i < num; ++i) (void) sam_read_line(&j, (uint64_t) i, (uint8_t *) s->h_text + s->h_off[i]);
  kfmi_big_free(rev);
  *sam = s;
  return KFMI_SUCCESS;
}
