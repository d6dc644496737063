/*
 * sam_asan.c -- TEST HARNESS: kfmi_sam_lines_cpu, the contig table and the SAM
 * handle (csrc/host/sam.c) built with the host C layer alone under
 * AddressSanitizer + UBSan (gcc) and driven over the records of
 * tests/sam_ref.py's world, which tests/test_sam_host.py writes to files: the
 * text, the reads, the table, the hits / paths / cigars / quals records and
 * the bytes the model expects.  Every line is compared, then the records are
 * overwritten with garbage (run words of every op and length, ends before
 * begins, ends past the text) and the call must still return whole lines.  The
 * HIP layer is replaced by the stubs below, as in second_asan.c.
 *
 *   sam_asan case.bin ...
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

static void *slurp(FILE *f, size_t bytes)
{
  void *p = malloc(bytes ? bytes : 1);
  if (!p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short case file\n"); exit(2); }
  return p;
}

static void *results_of(const uint32_t *src, uint64_t entries)
{
  void *r = NULL;
  if (kfmi_results_alloc(entries, &r) != 0) { fprintf(stderr, "results\n"); exit(2); }
  memcpy(kfmi_results_host(r), src, 8 * entries);
  return r;
}

static void run_case(const char *fn)
{
  FILE *f = fopen(fn, "rb");
  uint32_t hd[9], *begins, *lengths, *hits, *paths, *cig, *quals = NULL, x = 99u;
  uint64_t base, wide[3], *want_off, i;
  char *text, *reads, *names, *want;
  void *q = NULL, *ct = NULL, *rh, *rp, *rc, *rq = NULL, *sam = NULL;
  if (!f || fread(hd, 4, 9, f) != 9 || fread(&base, 8, 1, f) != 1 || fread(wide, 8, 3, f) != 3) {
    fprintf(stderr, "cannot read %s\n", fn);
    exit(2);
  }
  {
    const uint32_t n = hd[0], m = hd[1], num = hd[2], strands = hd[3], band = hd[4], C = hd[5], options = hd[6];
    const uint32_t count = hd[8];
    const uint64_t T = wide[2], bytes = wide[1];
    text = (char *) slurp(f, n);
    reads = (char *) slurp(f, (size_t) num * m);
    names = (char *) slurp(f, wide[0]);
    begins = (uint32_t *) slurp(f, 4 * count);
    lengths = (uint32_t *) slurp(f, 4 * count);
    hits = (uint32_t *) slurp(f, 8 * T);
    paths = (uint32_t *) slurp(f, 8 * T);
    cig = (uint32_t *) slurp(f, 8 * T * C);
    if (hd[7]) quals = (uint32_t *) slurp(f, 8 * T);
    want_off = (uint64_t *) slurp(f, 8 * ((size_t) num + 1));
    want = (char *) slurp(f, bytes);
    fclose(f);
    CHECK(kfmi_queries_from_buffer(reads, num, m, &q) == 0, "queries");
    CHECK(kfmi_contigs_create(names, begins, lengths, count, &ct) == 0, "contigs");
    rh = results_of(hits, T);
    rp = results_of(paths, T);
    rc = results_of(cig, T * C);
    if (quals) rq = results_of(quals, T);
    if (failures) exit(1);
    {
      const int64_t need = kfmi_sam_header(ct, NULL, 0);
      char *hb = (char *) malloc((size_t) need);
      CHECK(need > 23 && kfmi_sam_header(ct, hb, (uint64_t) need - 1) == need, "a short buffer is not written");
      CHECK(kfmi_sam_header(ct, hb, (uint64_t) need) == need && !memcmp(hb, "@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:", 29) &&
            hb[need - 1] == '\n', "header");
      free(hb);
    }
    CHECK(kfmi_sam_lines_cpu(text, n, q, ct, rh, rp, rc, rq, strands, C, band, options, base, 3, &sam) == 0, "%s", fn);
    if (!sam) exit(1);
    CHECK(kfmi_sam_num(sam) == num && kfmi_sam_bytes(sam) == bytes, "%s: %llu bytes, want %llu", fn,
          (unsigned long long) kfmi_sam_bytes(sam), (unsigned long long) bytes);
    for (i = 0; i <= num; ++i) CHECK(kfmi_sam_offsets(sam)[i] == want_off[i], "%s: offset %llu", fn, (unsigned long long) i);
    if (kfmi_sam_bytes(sam) == bytes)
      for (i = 0; i < num; ++i)
        CHECK(!memcmp(kfmi_sam_text(sam) + want_off[i], want + want_off[i], want_off[i + 1] - want_off[i]), "%s: line %llu",
              fn, (unsigned long long) i);
    CHECK(kfmi_sam_free(&sam) == 0 && sam == NULL, "free");
    /* refusals leave the pointer alone */
    sam = (void *) &x;
    CHECK(kfmi_sam_lines_cpu(text, n, q, ct, rh, rp, rc, rq, strands, C, band, 2, base, 1, &sam) == KFMI_E_BAD_ARGUMENT &&
          sam == (void *) &x, "an unknown option");
    CHECK(kfmi_sam_lines_cpu(text, begins[count - 1] + lengths[count - 1] - 1u, q, ct, rh, rp, rc, rq, strands, C, band,
                             options, base, 1, &sam) == KFMI_E_BAD_ARGUMENT && sam == (void *) &x, "a table past n");
    CHECK(kfmi_sam_lines_cpu(text, n, q, ct, rh, rh, rc, rq, strands, C, band, options, base, 1, &sam) ==
          KFMI_E_BAD_ARGUMENT && sam == (void *) &x, "paths is hits");
    sam = NULL;
    /* garbage records: whole lines all the same, every byte inside the allocation */
    {
      uint32_t *p = kfmi_results_host(rp), *g = kfmi_results_host(rc), *h = kfmi_results_host(rh), s = 12345u;
      for (i = 0; i < T; ++i) {
        s = s * 1664525u + 1013904223u;
        if ((s >> 28) < 3) h[2 * i] = s >> 4;
        if ((s >> 24 & 15u) < 6) p[2 * i] = (s >> 20 & 1u) ? s : h[2 * i] + (s >> 8) % (2 * m + 40u);
        if ((s >> 16 & 15u) < 8) p[2 * i + 1] = (p[2 * i + 1] & 0xFFFFu) | (s & 0x0FFF0000u);
      }
      for (i = 0; i < 2 * T * C; ++i) {
        s = s * 1664525u + 1013904223u;
        if ((s >> 29) == 0) g[i] = (s >> 3 & 1u) ? s : ((s >> 8) % (m + 2u)) << 4 | (s & 15u);
      }
      CHECK(kfmi_sam_lines_cpu(text, n, q, ct, rh, rp, rc, rq, strands, C, band, options, base, 2, &sam) == 0, "garbage");
      if (sam) {
        const uint64_t *off = kfmi_sam_offsets(sam);
        const char *t = kfmi_sam_text(sam);
        for (i = 0; i < num; ++i)
          CHECK(off[i + 1] > off[i] && t[off[i + 1] - 1] == '\n' && !memchr(t + off[i], '\n', off[i + 1] - off[i] - 1),
                "garbage: line %llu is not one line", (unsigned long long) i);
        CHECK(off[num] == kfmi_sam_bytes(sam), "garbage: total");
        kfmi_sam_free(&sam);
      }
    }
    freeQueries(&q);
    freeResults(&rh); freeResults(&rp); freeResults(&rc);
    if (rq) freeResults(&rq);
    CHECK(kfmi_contigs_free(&ct) == 0 && ct == NULL, "contigs free");
    free(text); free(reads); free(names); free(begins); free(lengths); free(hits); free(paths); free(cig); free(quals);
    free(want_off); free(want);
  }
}

int main(int argc, char **argv)
{
  static const uint32_t b2[2] = { 0, 9 }, l2[2] = { 10, 5 }, l0[2] = { 10, 0 };
  void *ct = (void *) b2;
  int i;
  CHECK(kfmi_contigs_create("a\0b\0", b2, l2, 2, &ct) == KFMI_E_BAD_ARGUMENT && ct == (void *) b2, "overlap");
  CHECK(kfmi_contigs_create("a\0b\0", b2, l0, 2, &ct) == KFMI_E_BAD_ARGUMENT && ct == (void *) b2, "length 0");
  CHECK(kfmi_contigs_create("a\0\0", b2, l2, 2, &ct) == KFMI_E_BAD_ARGUMENT && ct == (void *) b2, "empty name");
  CHECK(kfmi_contigs_create("a b\0", b2, l2, 1, &ct) == KFMI_E_BAD_ARGUMENT && ct == (void *) b2, "a space");
  CHECK(kfmi_contigs_create("a\0", b2, l2, 0, &ct) == KFMI_E_BAD_ARGUMENT && ct == (void *) b2, "count 0");
  CHECK(kfmi_sam_header(NULL, NULL, 0) < 0, "no table");
  for (i = 1; i < argc; ++i) run_case(argv[i]);
  if (failures) { printf("FAILED %d of %d\n", failures, checks); return 1; }
  printf("OK %d\n", checks);
  return 0;
}
