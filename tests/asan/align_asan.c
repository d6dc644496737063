/*
 * align_asan.c -- TEST HARNESS: kfmi_align_seeds_cpu (csrc/host/align.c) built
 * with the host C layer alone under AddressSanitizer + UBSan (gcc) and driven
 * over a small text: hand-made slot arrays with every ignored-slot form and
 * garbage values, suffix array entries of 0xFFFFFFFF, origins at both text ends
 * at band 15 (band cells off the text), reads of 1 and of 256 bases.  The HIP
 * layer is replaced by the stubs below, as in verify_asan.c.
 *
 *   align_asan
 * Prints "OK <checks>" and exits 0 when every check passes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../k-step_fm-index_amd/csrc/kfmi_internal.h"

/* ---- stubs for the HIP layer (csrc/hip) ---- */
int32_t freeIndexGPU(void **index) { (void) index; return KFMI_SUCCESS; }
int32_t kfmi_host_entries(kfmi_fmi_t *f) { return f->h_index ? KFMI_SUCCESS : KFMI_E_NOT_ON_DEVICE; }
void kfmi_free_dev_entries(kfmi_fmi_t *f) { f->d_entries = NULL; }
int32_t freeQueriesGPU(void **q) { (void) q; return KFMI_SUCCESS; }
int32_t freeResultsGPU(void **r) { (void) r; return KFMI_SUCCESS; }
kfmi_backend_t kfmi_backend(void) { return KFMI_BK_TASK_MID; }
uint32_t kfmi_backend_tag(kfmi_backend_t b) { (void) b; return 101u; }
int32_t kfmi_device_count(void) { return 0; }
int32_t kfmi_build_index_gpu_sa(const char *t, uint64_t n, uint32_t k, uint32_t d, uint32_t r, void **i)
{ (void) t; (void) n; (void) k; (void) d; (void) r; (void) i; return KFMI_E_NO_DEVICE; }
int32_t kfmi_build_index_gpu(const char *t, uint64_t n, uint32_t k, uint32_t d, int32_t h, void **i)
{ (void) h; return kfmi_build_index_gpu_sa(t, n, k, d, 0, i); }
static __thread int32_t last_error;
void kfmi_set_last_error(int32_t e) { last_error = e; }
int32_t kfmi_last_error(void) { return last_error; }

static int checks = 0, failures = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
  fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

enum { N = 523, ROWS = N + 1, S = 8, FILL = 0x5A5A5A5A, INF = 1 << 28 };

static char text[N + 1];

static int by_suffix(const void *a, const void *b)
{
  const uint32_t x = *(const uint32_t *) a, y = *(const uint32_t *) b;
  const int c = strcmp(text + x, text + y);   /* the terminator sorts first, like '$' */
  return c ? c : (x < y) - (x > y);
}

/* the definition once more in its prefix form's mirror: a full table, one candidate */
static void row0(const char *p, int m, long o, int w, int *row)
{
  static int a[257][31];
  int i, d;
  for (d = -w; d <= w; ++d) a[m][d + w] = o + m + d >= 0 && o + m + d <= N ? 0 : INF;
  for (i = m - 1; i >= 0; --i)
    for (d = w; d >= -w; --d) {
      const long j = o + i + d;
      int v = INF;
      if (j >= 0 && j <= N) {
        if (j < N && a[i + 1][d + w] + (base2index((unsigned char) p[i]) != base2index((unsigned char) text[j])) < v)
          v = a[i + 1][d + w] + (base2index((unsigned char) p[i]) != base2index((unsigned char) text[j]));
        if (d - 1 >= -w && a[i + 1][d - 1 + w] + 1 < v) v = a[i + 1][d - 1 + w] + 1;
        if (d + 1 <= w && j < N && a[i][d + 1 + w] + 1 < v) v = a[i][d + 1 + w] + 1;
        if (v > INF) v = INF;
      }
      a[i][d + w] = v;
    }
  for (d = 0; d <= 2 * w; ++d) row[d] = a[0][d];
}

/* one task's record, forward strand */
static void expect(const uint32_t *sa, const char *p, int m, const uint32_t *iv, const uint32_t *sp, uint32_t max_occ,
                   int w, uint32_t max_edits, uint32_t *hit)
{
  long best = INF, bmin = 0, bmax = 0;
  uint64_t scored = 0;
  uint32_t s;
  int row[31], k;
  for (s = 0; s < S; ++s) {
    const uint64_t L = iv[2 * s], R = iv[2 * s + 1], start = sp[2 * s], len = sp[2 * s + 1];
    uint64_t r;
    if (R <= L || L >= ROWS || len == 0 || start + len > (uint64_t) m) continue;
    for (r = L; r < R && r < ROWS && r < L + max_occ; ++r) {
      const uint64_t pos = sa[r];
      long o;
      if (pos >= ROWS || pos < start || pos - start + m > N) continue;
      o = (long) (pos - start);
      ++scored;
      row0(p, m, o, w, row);
      for (k = 0; k <= 2 * w; ++k) {
        const long b = o + k - w;
        if (row[k] >= INF || row[k] > best) continue;
        if (row[k] < best) { best = row[k]; bmin = bmax = b; }
        else { if (b < bmin) bmin = b; if (b > bmax) bmax = b; }
      }
    }
  }
  if (scored && (uint64_t) best <= max_edits) {
    hit[0] = (uint32_t) bmin;
    hit[1] = (uint32_t) best | (bmax - bmin > 2 * w ? KFMI_HIT_MULTI : 0u) | (uint32_t) (scored << KFMI_HIT_SCORED_SHIFT);
  } else {
    hit[0] = KFMI_HIT_NONE;
    hit[1] = (uint32_t) (scored << KFMI_HIT_SCORED_SHIFT);
  }
}

/* one read length: NUM reads, hand-made slots, every band / max_occ / bound, both suffix arrays */
static void run_length(const uint32_t *sa, const uint32_t *holes, int m)
{
  enum { NUM = 8 };
  static char reads[NUM * 256];
  void *q = NULL, *iv = NULL, *sp = NULL, *hits = NULL;
  uint32_t *hi, *hs, *hh, s, t, i, pass;
  const long origins[NUM] = { 0, 1, N - m, N - m - 1, 60, 60, 7, N - m - 9 };
  for (t = 0; t < NUM; ++t) memcpy(reads + t * m, text + origins[t], m);
  if (m > 4) {
    memmove(reads + 1 * m + m / 2, reads + 1 * m + m / 2 + 1, m - m / 2 - 1);   /* a base deleted near the text's start */
    reads[1 * m + m - 1] = text[1 + m];
    memmove(reads + 2 * m + m / 2 + 1, reads + 2 * m + m / 2, m - m / 2 - 1);   /* a base inserted at the text's end */
    reads[2 * m + m / 2] = 'n';
    memmove(reads + 3 * m + 1, reads + 3 * m + 2, m - 2);                       /* a base deleted, refilled to the end */
    reads[3 * m + m - 1] = text[N - 1];
    reads[5 * m + m / 3] = (char) (reads[5 * m + m / 3] ^ 6);
  }
  CHECK(kfmi_queries_from_buffer(reads, NUM, m, &q) == 0, "queries");
  CHECK(kfmi_results_alloc((uint64_t) S * NUM, &iv) == 0 && kfmi_results_alloc((uint64_t) S * NUM, &sp) == 0 &&
        kfmi_results_alloc(NUM, &hits) == 0, "handles");
  if (failures) exit(1);
  hi = kfmi_results_host(iv); hs = kfmi_results_host(sp); hh = kfmi_results_host(hits);
#define SLOT(t, s, L, R, st, ln) do { uint32_t *a = hi + 2 * ((t) * S + (s)), *b = hs + 2 * ((t) * S + (s)); \
  a[0] = (L); a[1] = (R); b[0] = (st); b[1] = (ln); } while (0)
  memset(hi, 0, 8ull * S * NUM); memset(hs, 0, 8ull * S * NUM);
  SLOT(0, 0, 0, ROWS, 0, m);                      /* the whole array, cut by max_occ */
  SLOT(0, 1, 3, 0xFFFFFFFFu, 0, 1);               /* R far past rows */
  SLOT(1, 0, ROWS, ROWS + 9, 0, m);               /* L >= rows */
  SLOT(1, 1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, m);
  SLOT(1, 2, 7, 7, 0, m);                         /* R <= L */
  SLOT(1, 3, 9, 2, 0, m);
  SLOT(1, 4, 0, ROWS, 0, 0);                      /* len == 0 */
  SLOT(1, 5, 0, ROWS, m - 1, 2);                  /* start + len > m */
  SLOT(1, 6, 0, ROWS, 0xFFFFFFFFu, 2);            /* ... and a sum that wraps in 32 bits */
  SLOT(1, 7, 0, ROWS, 0, 1);                      /* every row: the read's true origin is among the first 256 or not */
  SLOT(2, 7, 0, ROWS, m - 1, 1);                  /* origins off the start, and the text's last window */
  SLOT(3, 0, ROWS - 40, ROWS + 1000, 0, m);       /* the last rows, R > rows */
  for (i = 0; i < ROWS; ++i)                      /* tasks 2 and 3: the row of the unchanged part's own position */
    for (t = 2; t < 4; ++t)
      if ((long) sa[i] == origins[t]) SLOT(t, 1, i, i + 1, 0, 1);
  for (s = 0; s < S; ++s) SLOT(4, s, 0xFFFFFFFFu - s, s, 0xFFFFFFFFu, 0xFFFFFFFFu);   /* garbage */
  for (s = 0; s < S; ++s) SLOT(5, s, s * 25, s * 25 + 300, s < (uint32_t) m ? s : 0, m - (s < (uint32_t) m ? s : 0));
  for (s = 0; s < 2; ++s) SLOT(6, s, s * 200, ROWS, 0, 1);
  for (s = 0; s < S; ++s) SLOT(7, s, s * 60, s * 60 + 9, 0, m);
  for (pass = 0; pass < 2; ++pass) {
    const uint32_t *use = pass ? holes : sa;
    const uint32_t occs[3] = { 1, 17, KFMI_VERIFY_MAX_OCC }, bounds[2] = { 1, 0xFFFFFFFFu }, bands[3] = { 0, 2, 15 };
    uint32_t a, b, c;
    for (a = 0; a < 3; ++a)
      for (b = 0; b < 2; ++b)
        for (c = 0; c < 3; ++c) {
          for (i = 0; i < 2 * NUM; ++i) hh[i] = FILL;
          CHECK(kfmi_align_seeds_cpu(text, N, use, ROWS, q, iv, sp, hits, S, KFMI_STRAND_FWD, occs[a], bands[c],
                                     bounds[b], 3) == 0, "align m %d pass %u", m, pass);
          for (t = 0; t < NUM; ++t) {
            uint32_t want[2];
            expect(use, reads + t * m, m, hi + 2 * t * S, hs + 2 * t * S, occs[a], (int) bands[c], bounds[b], want);
            CHECK(hh[2 * t] == want[0] && hh[2 * t + 1] == want[1],
                  "m %d task %u pass %u occ %u band %u bound %u: %08x %08x, want %08x %08x", m, t, pass, occs[a], bands[c],
                  bounds[b], hh[2 * t], hh[2 * t + 1], want[0], want[1]);
          }
        }
  }
  /* both strands and the reverse strand run the same task function on P' */
  {
    void *iv2 = NULL, *sp2 = NULL, *hits2 = NULL;
    static char rev[NUM * 256];
    uint32_t *bi, *bs, *bh;
    CHECK(kfmi_results_alloc(2ull * S * NUM, &iv2) == 0 && kfmi_results_alloc(2ull * S * NUM, &sp2) == 0 &&
          kfmi_results_alloc(2ull * NUM, &hits2) == 0, "handles of BOTH");
    CHECK(kfmi_revcomp_queries(reads, NUM, m, rev) == 0, "revcomp");
    if (failures) exit(1);
    bi = kfmi_results_host(iv2); bs = kfmi_results_host(sp2); bh = kfmi_results_host(hits2);
    for (t = 0; t < 2 * NUM; ++t) {
      memcpy(bi + 2 * t * S, hi + 2 * (t >> 1) * S, 8 * S);
      memcpy(bs + 2 * t * S, hs + 2 * (t >> 1) * S, 8 * S);
    }
    CHECK(kfmi_align_seeds_cpu(text, N, holes, ROWS, q, iv2, sp2, hits2, S, KFMI_STRAND_BOTH, 9, 15, 40, 2) == 0, "both");
    for (t = 0; t < 2 * NUM; ++t) {
      uint32_t want[2];
      expect(holes, ((t & 1) ? rev : reads) + (t >> 1) * m, m, bi + 2 * t * S, bs + 2 * t * S, 9, 15, 40, want);
      CHECK(bh[2 * t] == want[0] && bh[2 * t + 1] == want[1], "both, m %d task %u", m, t);
    }
    /* refusals write nothing */
    for (i = 0; i < 2 * NUM; ++i) hh[i] = FILL;
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits, S, 1, 8, 16, 0, 1) == KFMI_E_BAD_ARGUMENT, "band 16");
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits, S, 1, 8, 0xFFFFFFFFu, 0, 1) == KFMI_E_BAD_ARGUMENT, "band -1");
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits, 0, 1, 8, 3, 0, 1) == KFMI_E_BAD_ARGUMENT, "S = 0");
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits, S, 4, 8, 3, 0, 1) == KFMI_E_BAD_ARGUMENT, "strands 4");
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits, S, 1, 257, 3, 0, 1) == KFMI_E_BAD_ARGUMENT, "max_occ 257");
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits2, S, 1, 8, 3, 0, 1) == KFMI_E_BAD_ARGUMENT, "hits too large");
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS - 1, q, iv, sp, hits, S, 1, 8, 3, 0, 1) == KFMI_E_BAD_ARGUMENT, "rows != n + 1");
    for (i = 0; i < 2 * NUM; ++i) CHECK(hh[i] == (uint32_t) FILL, "a refused call wrote hits[%u]", i);
    freeResults(&iv2); freeResults(&sp2); freeResults(&hits2);
  }
  /* the deleted and the inserted base at the text's ends cost one edit from band 1 on */
  if (m > 4) {
    CHECK(kfmi_align_seeds_cpu(text, N, sa, ROWS, q, iv, sp, hits, S, KFMI_STRAND_FWD, 256, 15, 0xFFFFFFFFu, 1) == 0, "align");
    CHECK((hh[2 * 2 + 1] & KFMI_HIT_MISM_MASK) <= 1 && hh[2 * 2] != KFMI_HIT_NONE, "m %d: inserted base at the end: %08x %08x",
          m, hh[4], hh[5]);
    CHECK((hh[2 * 3 + 1] & KFMI_HIT_MISM_MASK) <= 1 && hh[2 * 3] != KFMI_HIT_NONE, "m %d: deleted base at the end: %08x %08x",
          m, hh[6], hh[7]);
  }
  freeQueries(&q);
  freeResults(&iv); freeResults(&sp); freeResults(&hits);
}

int main(void)
{
  static uint32_t sa[ROWS], holes[ROWS];
  uint32_t x = 4321u, i;
  const int lengths[4] = { 1, 2, 37, 256 };
  for (i = 0; i < N; ++i) { x = x * 1664525u + 1013904223u; text[i] = "ACGT"[x >> 30]; }
  memcpy(text + 400, text + 20, 60);   /* a repeat: two distant placements for reads inside it */
  text[N] = 0;
  for (i = 0; i < ROWS; ++i) sa[i] = i;
  qsort(sa, ROWS, sizeof sa[0], by_suffix);
  CHECK(sa[0] == N, "the terminator's suffix is row 0");
  memcpy(holes, sa, sizeof sa);
  for (i = 0; i < ROWS; i += 3) holes[i] = 0xFFFFFFFFu;   /* rows without a suffix */
  for (i = 0; i < 4; ++i) run_length(sa, holes, lengths[i]);
  if (failures) { printf("FAILED %d of %d\n", failures, checks); return 1; }
  printf("OK %d\n", checks);
  return 0;
}
