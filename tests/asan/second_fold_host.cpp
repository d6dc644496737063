/*
 * second_fold_host.cpp -- TEST HARNESS: band_fold_far of csrc/hip/
 * kfmi_align_dp.h compiled for the host (g++, AddressSanitizer + UBSan) and
 * compared with a fold over row 0 of a plain full table written from the
 * definition of kstep_fmi.h ("second placement / mapping quality").
 *
 * The words come from band_rows<16>, staged the way the kernels stage them (as
 * in align_dp_host.cpp).  Cases: three text kinds (period 5, runs, random) of
 * 303 bases; reads of 17, 100 and 256 bases with 0-3 random edits; the origins
 * 0, 1, 7, a middle one, n - m - 3 and n - m, so that cells fall off either text
 * end; every band 0 .. 15; every X = o + x with x from -3w - 1 to 3w + 1 that is
 * no negative position, and X = 0xFFFFFFFE, far from everything.  Each case
 * folds the candidate and then its neighbour at o + w + 1 into one running
 * record.  Prints "OK <cases>"; exits 0 when every case agrees.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../k-step_fm-index_amd/csrc/hip/kfmi_align_dp.h"

namespace {

enum { N = 303, MAXM = 256, INF = 1 << 28 };

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); }
  uint32_t below(uint32_t k) { return next() % k; }
};

uint8_t text[N];
uint32_t stream[N / 16 + 1];   /* bit 2g: text base n - 1 - g; zero past the text */

void make_text(int kind, Rng& rng)
{
  int run = 0;
  uint8_t cur = 0;
  for (int i = 0; i < N; ++i) switch (kind) {
      case 0: text[i] = (uint8_t) ("\0\1\2\3\1"[i % 5]); break;   /* ACGTC ACGTC .. */
      case 1:
        if (run == 0) { run = 5 + (int) rng.below(5); cur = (uint8_t) ((cur + 1 + rng.below(3)) & 3); }
        text[i] = cur; --run; break;
      default: text[i] = (uint8_t) rng.below(4);
    }
  memset(stream, 0, sizeof stream);
  for (int g = 0; g < N; ++g) stream[g >> 4] |= (uint32_t) text[N - 1 - g] << (2 * (g & 15));
}

/* the definition: A(i, d), cell (i, d) at j = o + i + d, valid iff 0 <= j <= n */
void plain_row0(const uint8_t* p, int m, long o, int w, int* row)
{
  static int A[MAXM + 1][31];
  for (int i = m; i >= 0; --i)
    for (int d = w; d >= -w; --d) {
      const long j = o + i + d;
      int v = INF;
      if (j >= 0 && j <= N) {
        if (i == m) v = 0;
        else {
          if (j < N) { const int x = A[i + 1][d + w] + (p[i] != text[j]); if (x < v) v = x; }
          if (d - 1 >= -w) { const int x = A[i + 1][d - 1 + w] + 1; if (x < v) v = x; }
          if (d + 1 <= w && j < N) { const int x = A[i][d + 1 + w] + 1; if (x < v) v = x; }
          if (v > INF) v = INF;
        }
      }
      A[i][d + w] = v;
    }
  for (int k = 0; k <= 2 * w; ++k) row[k] = A[0][k];
}

struct Rec { long E, bmin, bmax; };

/* the far cells alone: |b - X| > 2w */
void plain_fold_far(const int* row, long o, int w, long X, Rec& r)
{
  for (int k = 0; k <= 2 * w; ++k) {
    const long b = o + k - w, dx = b > X ? b - X : X - b;
    if (row[k] >= INF || dx <= 2 * w || row[k] > r.E) continue;
    if (row[k] < r.E) { r.E = row[k]; r.bmin = r.bmax = b; }
    else { if (b < r.bmin) r.bmin = b; if (b > r.bmax) r.bmax = b; }
  }
}

void header_rows(const uint8_t* p, int m, uint32_t o, uint32_t w, uint32_t& vp, uint32_t& vn, uint32_t& s0)
{
  uint32_t cw[16], tx[19];
  for (int j = 0; j < 16; ++j) cw[j] = 0u;
  for (int i = 0; i < m; ++i) {
    const int r = m - 1 - i;
    cw[r >> 4] |= (uint32_t) p[i] << (2 * (r & 15));
  }
  const uint32_t n = N, off = n - o - (uint32_t) m, g = off + 16u - w, w0 = g >> 4, sh = g & 15u;
  const uint32_t lim = ((sh + (uint32_t) m - 1u + 2u * w) >> 4) + 1u, wtext = (n - 1u) >> 4;
  for (int j = 0; j < 19; ++j) {
    const uint32_t x = w0 + (uint32_t) j;
    tx[j] = ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) ? stream[x - 1u] : 0u;
  }
  kfmi::band_rows<16>(cw, tx, (uint32_t) m, w, sh, w > off ? w - off : 0u, vp, vn, s0);
}

long cases = 0, failures = 0;

void check(const uint8_t* p, int m, int o, int w, long X)
{
  uint32_t E = 0xFFFFFFFFu, bmin = 0xFFFFFFFFu, bmax = 0u;
  Rec r = { INF, 0, 0 };
  int row[31];
  for (int pass = 0; pass < 2; ++pass) {
    const int oo = pass ? o + w + 1 : o;
    if (oo + m > N) break;
    uint32_t vp, vn, s0;
    header_rows(p, m, (uint32_t) oo, (uint32_t) w, vp, vn, s0);
    kfmi::band_fold_far(vp, vn, s0, (uint32_t) w, (uint32_t) oo, (uint32_t) N, (uint32_t) X, E, bmin, bmax);
    plain_row0(p, m, oo, w, row);
    plain_fold_far(row, oo, w, X, r);
    ++cases;
    const bool none = r.E >= INF;
    if (none ? E != 0xFFFFFFFFu : ((long) E != r.E || (long) bmin != r.bmin || (long) bmax != r.bmax)) {
      if (++failures <= 20)
        fprintf(stderr, "FAIL m %d o %d w %d X %ld pass %d: got %u %u %u, want %ld %ld %ld\n", m, oo, w, X, pass, E, bmin,
                bmax, r.E, r.bmin, r.bmax);
    }
  }
}

}  // namespace

int main()
{
  Rng rng = { 2626 };
  const int lengths[3] = { 17, 100, 256 };
  for (int kind = 0; kind < 3; ++kind) {
    make_text(kind, rng);
    for (int li = 0; li < 3; ++li) {
      const int m = lengths[li];
      const int origins[6] = { 0, 1, 7, (N - m) / 2, N - m - 3, N - m };
      for (int oi = 0; oi < 6; ++oi) {
        const int o = origins[oi];
        uint8_t p[MAXM];
        memcpy(p, text + o, (size_t) m);
        for (uint32_t e = rng.below(4); e > 0; --e) {
          const uint32_t at = rng.below((uint32_t) m);
          switch (rng.below(3)) {
            case 0: p[at] = (uint8_t) ((p[at] + 1 + rng.below(3)) & 3); break;
            case 1: memmove(p + at, p + at + 1, (size_t) (m - 1 - (int) at)); p[m - 1] = (uint8_t) rng.below(4); break;
            default: memmove(p + at + 1, p + at, (size_t) (m - 1 - (int) at)); p[at] = (uint8_t) rng.below(4);
          }
        }
        for (int w = 0; w <= 15; ++w) {
          for (int x = -3 * w - 1; x <= 3 * w + 1; ++x)
            if (o + x >= 0) check(p, m, o, w, (long) o + x);
          check(p, m, o, w, 0xFFFFFFFEl);
        }
      }
    }
  }
  if (failures) { printf("FAILED %ld of %ld\n", failures, cases); return 1; }
  printf("OK %ld\n", cases);
  return 0;
}
