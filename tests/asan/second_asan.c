/*
 * second_asan.c -- TEST HARNESS: kfmi_align_second_cpu and kfmi_map_quality_cpu
 * (csrc/host/second.c) built with the host C layer alone under
 * AddressSanitizer + UBSan (gcc) and driven over a small text with a repeat:
 * hand-made slot arrays with every ignored-slot form and garbage values, suffix
 * array entries of 0xFFFFFFFF, hits from kfmi_align_seeds_cpu and hand-made
 * ones (KFMI_HIT_NONE, X past the text, X = 0), band 15 at both text ends,
 * reads of 1 and of 256 bases, all three strand modes of the quality.  The HIP
 * layer is replaced by the stubs below, as in align_asan.c.
 *
 *   second_asan
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

enum { N = 523, ROWS = N + 1, S = 8, NUM = 8, FILL = 0x5A5A5A5A, INF = 1 << 28 };

static char text[N + 1];

static int by_suffix(const void *a, const void *b)
{
  const uint32_t x = *(const uint32_t *) a, y = *(const uint32_t *) b;
  const int c = strcmp(text + x, text + y);   /* the terminator sorts first, like '$' */
  return c ? c : (x < y) - (x > y);
}

/* the definition once more: a full table, one candidate */
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
        const int mis = j < N && base2index((unsigned char) p[i]) != base2index((unsigned char) text[j]);
        if (j < N && a[i + 1][d + w] + mis < v) v = a[i + 1][d + w] + mis;
        if (d - 1 >= -w && a[i + 1][d - 1 + w] + 1 < v) v = a[i + 1][d - 1 + w] + 1;
        if (d + 1 <= w && j < N && a[i][d + 1 + w] + 1 < v) v = a[i][d + 1 + w] + 1;
        if (v > INF) v = INF;
      }
      a[i][d + w] = v;
    }
  for (d = 0; d <= 2 * w; ++d) row[d] = a[0][d];
}

/* one task's second record, forward strand */
static void expect(const uint32_t *sa, const char *p, int m, const uint32_t *iv, const uint32_t *sp, uint32_t max_occ,
                   int w, uint32_t X, uint32_t max_second, uint32_t *rec)
{
  long best = INF, bmin = 0, bmax = 0;
  uint32_t counted = 0, trunc = 0, s;
  int row[31], k;
  rec[0] = KFMI_HIT_NONE;
  rec[1] = 0;
  if (X == KFMI_HIT_NONE) return;
  for (s = 0; s < S; ++s) {
    const uint64_t L = iv[2 * s], R = iv[2 * s + 1], start = sp[2 * s], len = sp[2 * s + 1];
    uint64_t r;
    if (R <= L || L >= ROWS || len == 0 || start + len > (uint64_t) m) continue;
    if ((R < ROWS ? R : ROWS) - L > max_occ) trunc = KFMI_SECOND_TRUNCATED;
    for (r = L; r < R && r < ROWS && r < L + max_occ; ++r) {
      const uint64_t pos = sa[r];
      long o, far;
      if (pos >= ROWS || pos < start || pos - start + m > N) continue;
      o = (long) (pos - start);
      far = o - (long) X;
      if (far > w || far < -w) ++counted;
      row0(p, m, o, w, row);
      for (k = 0; k <= 2 * w; ++k) {
        const long b = o + k - w, dx = b - (long) X;
        if (row[k] >= INF || row[k] > best || (dx <= 2 * w && dx >= -2 * w)) continue;
        if (row[k] < best) { best = row[k]; bmin = bmax = b; }
        else { if (b < bmin) bmin = b; if (b > bmax) bmax = b; }
      }
    }
  }
  rec[1] = trunc | (counted << KFMI_HIT_SCORED_SHIFT);
  if (best < INF && (uint64_t) best <= max_second) {
    rec[0] = (uint32_t) bmin;
    rec[1] |= (uint32_t) best | (bmax - bmin > 2 * w ? KFMI_HIT_MULTI : 0u);
  }
}

/* the quality of one task, written out from the header's text */
static void expect_quality(const uint32_t *h, const uint32_t *s2, uint64_t t, uint32_t strands, uint32_t max_second,
                           uint32_t *out)
{
  const uint64_t u = t ^ 1u;
  uint64_t E = h[2 * t + 1] & 0xFFFFu, C = (uint64_t) max_second + 1u, gap, q;
  int trunc = (s2[2 * t + 1] & KFMI_SECOND_TRUNCATED) != 0;
  out[0] = out[1] = 0;
  if (h[2 * t] == KFMI_HIT_NONE) return;
  if (s2[2 * t] != KFMI_HIT_NONE && (s2[2 * t + 1] & 0xFFFFu) < C) C = s2[2 * t + 1] & 0xFFFFu;
  if (strands == KFMI_STRAND_BOTH) {
    if (h[2 * u] != KFMI_HIT_NONE && (h[2 * u + 1] & 0xFFFFu) < C) C = h[2 * u + 1] & 0xFFFFu;
    trunc |= (s2[2 * u + 1] & KFMI_SECOND_TRUNCATED) != 0;
  }
  gap = C > E ? C - E : 0;
  if (strands == KFMI_STRAND_BOTH && h[2 * u] != KFMI_HIT_NONE && (h[2 * u + 1] & 0xFFFFu) == E && (t & 1)) gap = 0;
  if (gap > 0xFFFFFFFFull) gap = 0xFFFFFFFFull;
  q = 10 * gap < 60 ? 10 * gap : 60;
  if (trunc && q > 3) q = 3;
  out[0] = (uint32_t) q;
  out[1] = (uint32_t) gap;
}

static void run_length(const uint32_t *sa, const uint32_t *holes, int m)
{
  static char reads[NUM * 256];
  void *q = NULL, *iv = NULL, *sp = NULL, *hits = NULL, *second = NULL, *quals = NULL;
  uint32_t *hi, *hs, *hh, *h2, *hq, s, t, i, pass;
  const long origins[NUM] = { 0, 1, N - m, N - m - 1, 60, 60, 7, N - m - 9 };
  for (t = 0; t < NUM; ++t) memcpy(reads + t * m, text + origins[t], m);
  if (m <= 60) memcpy(reads + 4 * m, text + 20, m);                  /* inside the repeat: two distant placements */
  if (m > 4) {
    memmove(reads + 1 * m + m / 2, reads + 1 * m + m / 2 + 1, m - m / 2 - 1);   /* a base deleted near the text's start */
    reads[1 * m + m - 1] = text[1 + m];
    reads[5 * m + m / 3] = (char) (reads[5 * m + m / 3] ^ 6);
  }
  CHECK(kfmi_queries_from_buffer(reads, NUM, m, &q) == 0, "queries");
  CHECK(kfmi_results_alloc((uint64_t) S * NUM, &iv) == 0 && kfmi_results_alloc((uint64_t) S * NUM, &sp) == 0 &&
        kfmi_results_alloc(NUM, &hits) == 0 && kfmi_results_alloc(NUM, &second) == 0 &&
        kfmi_results_alloc(NUM, &quals) == 0, "handles");
  if (failures) exit(1);
  hi = kfmi_results_host(iv); hs = kfmi_results_host(sp); hh = kfmi_results_host(hits);
  h2 = kfmi_results_host(second); hq = kfmi_results_host(quals);
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
  SLOT(1, 7, 0, ROWS, 0, 1);
  SLOT(2, 7, 0, ROWS, m - 1, 1);                  /* origins off the start, and the text's last window */
  SLOT(3, 0, ROWS - 40, ROWS + 1000, 0, m);       /* the last rows, R > rows */
  for (s = 0; s < S; ++s) SLOT(4, s, 0xFFFFFFFFu - s, s, 0xFFFFFFFFu, 0xFFFFFFFFu);   /* garbage */
  SLOT(4, 0, 0, ROWS, 0, m < 8 ? m : 8);          /* and one slot over every row */
  for (s = 0; s < S; ++s) SLOT(5, s, s * 25, s * 25 + 300, s < (uint32_t) m ? s : 0, m - (s < (uint32_t) m ? s : 0));
  for (s = 0; s < 2; ++s) SLOT(6, s, s * 200, ROWS, 0, 1);
  for (s = 0; s < S; ++s) SLOT(7, s, s * 60, s * 60 + 9, 0, m);
  for (pass = 0; pass < 2; ++pass) {
    const uint32_t *use = pass ? holes : sa;
    const uint32_t occs[3] = { 1, 17, KFMI_VERIFY_MAX_OCC }, bounds[3] = { 0, 3, 0xFFFFFFFFu }, bands[3] = { 0, 2, 15 };
    uint32_t a, b, c;
    for (a = 0; a < 3; ++a)
      for (c = 0; c < 3; ++c) {
        CHECK(kfmi_align_seeds_cpu(text, N, use, ROWS, q, iv, sp, hits, S, KFMI_STRAND_FWD, occs[a], bands[c], 0xFFFFFFFFu,
                                   2) == 0, "align m %d", m);
        if (c == 1) { hh[2 * 6] = KFMI_HIT_NONE; hh[2 * 7] = N + 77; hh[2 * 5] = 0; }   /* hand-made X */
        for (b = 0; b < 3; ++b) {
          for (i = 0; i < 2 * NUM; ++i) h2[i] = hq[i] = FILL;
          CHECK(kfmi_align_second_cpu(text, N, use, ROWS, q, iv, sp, hits, second, S, KFMI_STRAND_FWD, occs[a], bands[c],
                                      bounds[b], 3) == 0, "second m %d pass %u", m, pass);
          for (t = 0; t < NUM; ++t) {
            uint32_t want[2];
            expect(use, reads + t * m, m, hi + 2 * t * S, hs + 2 * t * S, occs[a], (int) bands[c], hh[2 * t], bounds[b], want);
            CHECK(h2[2 * t] == want[0] && h2[2 * t + 1] == want[1],
                  "m %d task %u pass %u occ %u band %u bound %u: %08x %08x, want %08x %08x", m, t, pass, occs[a], bands[c],
                  bounds[b], h2[2 * t], h2[2 * t + 1], want[0], want[1]);
          }
          for (s = KFMI_STRAND_FWD; s <= KFMI_STRAND_BOTH; ++s) {
            CHECK(kfmi_map_quality_cpu(hits, second, quals, s, bounds[b]) == 0, "quality");
            for (t = 0; t < NUM; ++t) {
              uint32_t want[2];
              expect_quality(hh, h2, t, s, bounds[b], want);
              CHECK(hq[2 * t] == want[0] && hq[2 * t + 1] == want[1], "quality m %d task %u strands %u bound %u: %u %u, want %u %u",
                    m, t, s, bounds[b], hq[2 * t], hq[2 * t + 1], want[0], want[1]);
            }
          }
        }
      }
  }
  /* both strands run the same task function on P' */
  {
    void *iv2 = NULL, *sp2 = NULL, *hits2 = NULL, *sec2 = NULL;
    static char rev[NUM * 256];
    uint32_t *bi, *bs, *bh, *b2;
    CHECK(kfmi_results_alloc(2ull * S * NUM, &iv2) == 0 && kfmi_results_alloc(2ull * S * NUM, &sp2) == 0 &&
          kfmi_results_alloc(2ull * NUM, &hits2) == 0 && kfmi_results_alloc(2ull * NUM, &sec2) == 0, "handles of BOTH");
    CHECK(kfmi_revcomp_queries(reads, NUM, m, rev) == 0, "revcomp");
    if (failures) exit(1);
    bi = kfmi_results_host(iv2); bs = kfmi_results_host(sp2); bh = kfmi_results_host(hits2); b2 = kfmi_results_host(sec2);
    for (t = 0; t < 2 * NUM; ++t) {
      memcpy(bi + 2 * t * S, hi + 2 * (t >> 1) * S, 8 * S);
      memcpy(bs + 2 * t * S, hs + 2 * (t >> 1) * S, 8 * S);
    }
    CHECK(kfmi_align_seeds_cpu(text, N, holes, ROWS, q, iv2, sp2, hits2, S, KFMI_STRAND_BOTH, 9, 15, 0xFFFFFFFFu, 2) == 0, "both");
    CHECK(kfmi_align_second_cpu(text, N, holes, ROWS, q, iv2, sp2, hits2, sec2, S, KFMI_STRAND_BOTH, 9, 15, 40, 2) == 0, "both");
    for (t = 0; t < 2 * NUM; ++t) {
      uint32_t want[2];
      expect(holes, ((t & 1) ? rev : reads) + (t >> 1) * m, m, bi + 2 * t * S, bs + 2 * t * S, 9, 15, bh[2 * t], 40, want);
      CHECK(b2[2 * t] == want[0] && b2[2 * t + 1] == want[1], "both, m %d task %u", m, t);
    }
    /* refusals write nothing */
    for (i = 0; i < 2 * NUM; ++i) h2[i] = hq[i] = FILL;
#define REFUSED(call, what) CHECK((call) == KFMI_E_BAD_ARGUMENT, what)
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, hits, second, S, 1, 8, 16, 0, 1), "band 16");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, hits, second, 0, 1, 8, 3, 0, 1), "S = 0");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, hits, second, S, 4, 8, 3, 0, 1), "strands 4");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, hits, second, S, 1, 257, 3, 0, 1), "max_occ 257");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, hits2, second, S, 1, 8, 3, 0, 1), "hits too large");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, hits, sec2, S, 1, 8, 3, 0, 1), "second too large");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS, q, iv, sp, second, second, S, 1, 8, 3, 0, 1), "hits is second");
    REFUSED(kfmi_align_second_cpu(text, N, sa, ROWS - 1, q, iv, sp, hits, second, S, 1, 8, 3, 0, 1), "rows != n + 1");
    REFUSED(kfmi_map_quality_cpu(hits, second, quals, 0, 3), "strands 0");
    REFUSED(kfmi_map_quality_cpu(hits, second, quals, 4, 3), "strands 4");
    REFUSED(kfmi_map_quality_cpu(hits, second, second, 1, 3), "quals is second");
    REFUSED(kfmi_map_quality_cpu(hits2, second, quals, 1, 3), "sizes");
    for (i = 0; i < 2 * NUM; ++i) CHECK(h2[i] == (uint32_t) FILL && hq[i] == (uint32_t) FILL, "a refused call wrote entry %u", i);
    freeResults(&iv2); freeResults(&sp2); freeResults(&hits2); freeResults(&sec2);
  }
  freeQueries(&q);
  freeResults(&iv); freeResults(&sp); freeResults(&hits); freeResults(&second); freeResults(&quals);
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
