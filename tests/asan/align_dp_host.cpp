/*
 * align_dp_host.cpp -- TEST HARNESS: csrc/hip/kfmi_align_dp.h compiled for the
 * host (g++, AddressSanitizer + UBSan) and compared with a plain full-table
 * dynamic programme written from the definition of kstep_fmi.h ("align seeds").
 *
 * The code words and the window words are built the way align_kernel builds
 * them: the read's last base in the low bits of cw[0]; the text's word stream
 * with bit 2g = text base n - 1 - g, addressed through a stream with one word
 * in front (g = off + 16 - w, w0 = g >> 4, sh = g & 15, lim words, zero where
 * the stream holds no text).  band_rows<16> runs at every length, band_rows<8>
 * as well up to 128 bases, band_fold folds one candidate and then a second one
 * (a neighbouring origin) into the same running record.
 *
 * Families of cases (six text kinds each: all-A, period 2, period 3, random
 * over two letters, runs of 5-9 equal bases, random):
 *   sweep   n in 40, 257, 300, 303, 320; every m of 1, 2, 15, 16, 17, 33, 100,
 *           128, 129, 255, 256 that fits; every band 0..15; the 16 first and 16
 *           last origins and 8 random ones; the read is the window shifted by
 *           up to +-w with 0-3 random edits;
 *   ends    n in 303, 320; m in 17, 100, 129, 256; every band; the 16 first
 *           and 16 last origins x every pinned read position x {one base
 *           deleted, one inserted};
 *   edge    every w >= 1: the exact window at o + w and at o - w scored at o
 *           (the only best cell on the band's edge, E = 0 on a text without
 *           repeats);
 *   indel   every w >= 1: one deletion and one insertion of w and of w + 1
 *           bases at m / 2;
 *   leave   every w >= 1: w + 1 bases deleted at m / 3 and w + 1 inserted at
 *           2m / 3: the path leaves the band, the plain table says what that
 *           costs inside it;
 *   comeback  the mirror image: w + 1 foreign bases inserted at m / 3 and w + 1
 *           text bases deleted at 2m / 3.  This path leaves the band on the
 *           side of the bits above 2w, which the words do hold: only the
 *           +infinity bit keeps it out.
 *
 * Prints one line "<family> <cases>" per family and "OK <cases>"; exits 0 when
 * every case agrees.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../k-step_fm-index_amd/csrc/hip/kfmi_align_dp.h"

namespace {

enum { MAXN = 320, MAXM = 256, INF = 1 << 28 };

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); }
  uint32_t below(uint32_t k) { return next() % k; }
};

struct Text {
  int n;
  uint8_t c[MAXN];
  uint32_t stream[MAXN / 16 + 1];   /* bit 2g: text base n - 1 - g; zero past the text */
};

const char* const KINDS[6] = { "all-A", "period-2", "period-3", "two-letter", "runs", "random" };

void make_text(Text& T, int kind, int n, Rng& rng)
{
  T.n = n;
  int run = 0;
  uint8_t cur = 0;
  for (int i = 0; i < n; ++i) switch (kind) {
      case 0: T.c[i] = 0; break;
      case 1: T.c[i] = (uint8_t) (1 + (i & 1)); break;          /* CGCG.. */
      case 2: T.c[i] = (uint8_t) ("\0\1\3"[i % 3]); break;       /* ACTACT.. */
      case 3: T.c[i] = (uint8_t) (rng.below(2) ? 3 : 0); break;
      case 4:
        if (run == 0) { run = 5 + (int) rng.below(5); cur = (uint8_t) ((cur + 1 + rng.below(3)) & 3); }
        T.c[i] = cur; --run; break;
      default: T.c[i] = (uint8_t) rng.below(4);
    }
  memset(T.stream, 0, sizeof T.stream);
  for (int g = 0; g < n; ++g) T.stream[g >> 4] |= (uint32_t) T.c[n - 1 - g] << (2 * (g & 15));
}

/* the definition: A(i, d), cell (i, d) at j = o + i + d, valid iff 0 <= j <= n */
void plain_row0(const Text& T, const uint8_t* p, int m, long o, int w, int* row)
{
  static int A[MAXM + 1][31];
  const long n = T.n;
  for (int i = m; i >= 0; --i)
    for (int d = w; d >= -w; --d) {          /* d + 1 of the same row first */
      const long j = o + i + d;
      int v = INF;
      if (j >= 0 && j <= n) {
        if (i == m) v = 0;
        else {
          if (j < n) { const int x = A[i + 1][d + w] + (p[i] != T.c[j]); if (x < v) v = x; }
          if (d - 1 >= -w) { const int x = A[i + 1][d - 1 + w] + 1; if (x < v) v = x; }
          if (d + 1 <= w && j < n) { const int x = A[i][d + 1 + w] + 1; if (x < v) v = x; }
          if (v > INF) v = INF;
        }
      }
      A[i][d + w] = v;
    }
  for (int k = 0; k <= 2 * w; ++k) row[k] = A[0][k];
}

struct Rec { long E, bmin, bmax; };

void plain_fold(const int* row, long o, int w, Rec& r)
{
  for (int k = 0; k <= 2 * w; ++k) {
    const long b = o + k - w;
    if (row[k] >= INF || row[k] > r.E) continue;
    if (row[k] < r.E) { r.E = row[k]; r.bmin = r.bmax = b; }
    else { if (b < r.bmin) r.bmin = b; if (b > r.bmax) r.bmax = b; }
  }
}

int bad_lim = 0;

/* row m of one candidate through the header, the words staged as align_kernel stages them */
template <int MAXW>
void header_rows(const Text& T, const uint8_t* p, int m, uint32_t o, uint32_t w, uint32_t& vp, uint32_t& vn, uint32_t& s0)
{
  uint32_t cw[MAXW], tx[MAXW + 3];
  for (int j = 0; j < MAXW; ++j) cw[j] = 0u;
  for (int i = 0; i < m; ++i) {
    const int r = m - 1 - i;
    cw[r >> 4] |= (uint32_t) p[i] << (2 * (r & 15));
  }
  const uint32_t n = (uint32_t) T.n, off = n - o - (uint32_t) m, g = off + 16u - w, w0 = g >> 4, sh = g & 15u;
  const uint32_t lim = ((sh + (uint32_t) m - 1u + 2u * w) >> 4) + 1u, wtext = (n - 1u) >> 4;
  if (lim > (uint32_t) MAXW + 3u) ++bad_lim;
  for (int j = 0; j < MAXW + 3; ++j) {
    const uint32_t x = w0 + (uint32_t) j;
    tx[j] = ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) ? T.stream[x - 1u] : 0u;
  }
  kfmi::band_rows<MAXW>(cw, tx, (uint32_t) m, w, sh, w > off ? w - off : 0u, vp, vn, s0);
}

long cases = 0, failures = 0;

struct State { uint32_t E, bmin, bmax; };

bool agree(const State& s, const Rec& r)
{
  return (long) s.E == r.E && (long) s.bmin == r.bmin && (long) s.bmax == r.bmax;
}

/* one case: the read p scored at origin o under band w, then a neighbouring origin folded in */
void check(const Text& T, int kind, const uint8_t* p, int m, int o, int w, const char* family, bool second)
{
  int row[31];
  Rec want = { INF, 0, 0 };
  State s16 = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0u }, s8 = s16;
  ++cases;
  for (int pass = 0; pass < (second ? 2 : 1); ++pass) {
    const int oo = pass == 0 ? o : (o + 1 + m <= T.n ? o + 1 : o - 1);
    if (oo < 0) break;
    plain_row0(T, p, m, oo, w, row);
    plain_fold(row, oo, w, want);
    uint32_t vp, vn, s0;
    header_rows<16>(T, p, m, (uint32_t) oo, (uint32_t) w, vp, vn, s0);
    kfmi::band_fold(vp, vn, s0, (uint32_t) w, (uint32_t) oo, (uint32_t) T.n, s16.E, s16.bmin, s16.bmax);
    bool ok = agree(s16, want);
    if (m <= 128) {
      header_rows<8>(T, p, m, (uint32_t) oo, (uint32_t) w, vp, vn, s0);
      kfmi::band_fold(vp, vn, s0, (uint32_t) w, (uint32_t) oo, (uint32_t) T.n, s8.E, s8.bmin, s8.bmax);
      ok = ok && agree(s8, want);
    }
    if (!ok) {
      if (++failures <= 20)
        fprintf(stderr, "FAIL %s %s n %d m %d o %d band %d pass %d: 16 words (%u %u %u) 8 words (%u %u %u), want (%ld %ld %ld)\n",
                family, KINDS[kind], T.n, m, oo, w, pass, s16.E, s16.bmin, s16.bmax, s8.E, s8.bmin, s8.bmax, want.E,
                want.bmin, want.bmax);
      return;
    }
  }
}

uint8_t other(uint8_t a, uint8_t b, Rng& rng)
{
  for (;;) {
    const uint8_t x = (uint8_t) rng.below(4);
    if (x != a && x != b) return x;
  }
}

int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

/* the window at a without the k text bases from a + p on: refilled at its right end, or at its left where the text ends */
void deleted(const Text& T, int a, int m, int p, int k, uint8_t* out)
{
  if (a + m + k <= T.n) {
    memcpy(out, T.c + a, (size_t) p);
    memcpy(out + p, T.c + a + p + k, (size_t) (m - p));
  } else {
    memcpy(out, T.c + a - k, (size_t) p);
    memcpy(out + p, T.c + a + p, (size_t) (m - p));
  }
}

/* the window at a with k foreign bases before its base p, cut to m bases */
void inserted(const Text& T, int a, int m, int p, int k, Rng& rng, uint8_t* out)
{
  memcpy(out, T.c + a, (size_t) p);
  for (int i = 0; i < k; ++i) out[p + i] = other(T.c[a + p], i ? out[p + i - 1] : (p ? T.c[a + p - 1] : T.c[a + p]), rng);
  memcpy(out + p + k, T.c + a + p, (size_t) (m - p - k));
}

const int SWEEP_N[5] = { 40, 257, 300, 303, 320 };
const int SWEEP_M[11] = { 1, 2, 15, 16, 17, 33, 100, 128, 129, 255, 256 };
const int PIN_M[4] = { 17, 100, 129, 256 };

int pinned(int m, int* out)
{
  const int all[8] = { 1, 15, 16, 17, m / 2, m - 17, m - 16, m - 2 };
  int cnt = 0;
  for (int p = 1; p <= m - 2; ++p)
    for (int i = 0; i < 8; ++i)
      if (all[i] == p) { out[cnt++] = p; break; }
  return cnt;
}

long sweep(Rng& rng)
{
  const long before = cases;
  Text T;
  uint8_t p[MAXM + 4];
  for (int kind = 0; kind < 6; ++kind)
    for (int ni = 0; ni < 5; ++ni) {
      make_text(T, kind, SWEEP_N[ni], rng);
      const int n = T.n;
      for (int mi = 0; mi < 11; ++mi) {
        const int m = SWEEP_M[mi];
        if (m > n) continue;
        for (int w = 0; w <= 15; ++w)
          for (int oi = 0; oi < 40; ++oi) {
            const int last = n - m;
            const int o = oi < 16 ? (oi < last ? oi : last) : oi < 32 ? (last - (oi - 16) > 0 ? last - (oi - 16) : 0)
                                                                       : (int) rng.below((uint32_t) last + 1u);
            const int a = clampi(o + (int) rng.below(2u * (uint32_t) w + 1u) - w, 0, last);
            memcpy(p, T.c + a, (size_t) m);
            for (int e = (int) (cases & 3); e > 0; --e) {
              const int at = (int) rng.below((uint32_t) m), what = m >= 2 ? (int) rng.below(3) : 0;
              if (what == 0) p[at] = other(p[at], p[at], rng);
              else if (what == 1) { memmove(p + at + 1, p + at, (size_t) (m - 1 - at)); p[at] = (uint8_t) rng.below(4); }
              else { memmove(p + at, p + at + 1, (size_t) (m - 1 - at)); p[m - 1] = (uint8_t) rng.below(4); }
            }
            check(T, kind, p, m, o, w, "sweep", true);
          }
      }
    }
  return cases - before;
}

long ends(Rng& rng)
{
  const long before = cases;
  Text T;
  uint8_t p[MAXM + 4];
  const int ns[2] = { 303, 320 };
  for (int kind = 0; kind < 6; ++kind)
    for (int ni = 0; ni < 2; ++ni) {
      make_text(T, kind, ns[ni], rng);
      for (int mi = 0; mi < 4; ++mi) {
        const int m = PIN_M[mi];
        int pins[8];
        const int np = pinned(m, pins);
        for (int w = 0; w <= 15; ++w)
          for (int oi = 0; oi < 32; ++oi) {
            const int a = oi < 16 ? oi : T.n - m - (oi - 16);
            for (int pi = 0; pi < np; ++pi) {
              deleted(T, a, m, pins[pi], 1, p);
              check(T, kind, p, m, a, w, "ends", false);
              inserted(T, a, m, pins[pi], 1, rng, p);
              check(T, kind, p, m, a, w, "ends", false);
            }
          }
      }
    }
  return cases - before;
}

bool fits(int m, int k) { return 3 * k <= m; }

/* edge, indel and leave: every w >= 1 at the band w (and the bands beside it), three origins per text */
void bands_of(int w, int* out, int& cnt)
{
  cnt = 0;
  out[cnt++] = w;
  if (w > 1) out[cnt++] = w - 1;
  if (w < 15) out[cnt++] = w + 1;
}

long edge(Rng& rng)
{
  const long before = cases;
  Text T;
  const int ns[3] = { 300, 303, 320 };
  for (int kind = 0; kind < 6; ++kind)
    for (int ni = 0; ni < 3; ++ni) {
      make_text(T, kind, ns[ni], rng);
      for (int mi = 0; mi < 4; ++mi) {
        const int m = PIN_M[mi], last = T.n - m;
        for (int w = 1; w <= 15; ++w) {
          const int os[3] = { w, last - w, last / 2 };
          for (int oi = 0; oi < 3; ++oi) {
            check(T, kind, T.c + os[oi] + w, m, os[oi], w, "edge", true);   /* the only zero at d = +w */
            check(T, kind, T.c + os[oi] - w, m, os[oi], w, "edge", true);   /* ... at d = -w */
          }
        }
      }
    }
  return cases - before;
}

long indel(Rng& rng)
{
  const long before = cases;
  Text T;
  uint8_t p[MAXM + 4];
  const int ns[3] = { 300, 303, 320 };
  for (int kind = 0; kind < 6; ++kind)
    for (int ni = 0; ni < 3; ++ni) {
      make_text(T, kind, ns[ni], rng);
      for (int mi = 0; mi < 4; ++mi) {
        const int m = PIN_M[mi], last = T.n - m;
        for (int w = 1; w <= 15; ++w)
          for (int k = w; k <= w + 1; ++k) {
            if (!fits(m, k)) continue;
            int bs[3], nb;
            bands_of(w, bs, nb);
            const int os[3] = { 3, last - 2, last / 2 };
            for (int oi = 0; oi < 3; ++oi)
              for (int bi = 0; bi < nb; ++bi) {
                deleted(T, os[oi], m, m / 2, k, p);
                check(T, kind, p, m, os[oi], bs[bi], "indel", false);
                inserted(T, os[oi], m, m / 2, k, rng, p);
                check(T, kind, p, m, os[oi], bs[bi], "indel", false);
              }
          }
      }
    }
  return cases - before;
}

long leave(Rng& rng)
{
  const long before = cases;
  Text T;
  uint8_t p[MAXM + 4];
  const int ns[3] = { 300, 303, 320 };
  for (int kind = 0; kind < 6; ++kind)
    for (int ni = 0; ni < 3; ++ni) {
      make_text(T, kind, ns[ni], rng);
      for (int mi = 0; mi < 4; ++mi) {
        const int m = PIN_M[mi], last = T.n - m;
        for (int w = 1; w <= 15; ++w) {
          const int k = w + 1, a3 = m / 3, b3 = 2 * m / 3;
          if (!fits(m, k)) continue;
          int bs[3], nb;
          bands_of(w, bs, nb);
          const int os[3] = { 0, last - 16, last / 2 };   /* n >= m + 44: the k bases past the window are text */
          for (int oi = 0; oi < 3; ++oi) {
            const int a = os[oi];
            memcpy(p, T.c + a, (size_t) a3);
            memcpy(p + a3, T.c + a + a3 + k, (size_t) (b3 - a3));
            for (int i = 0; i < k; ++i) p[b3 + i] = other(T.c[a + b3 + k], i ? p[b3 + i - 1] : T.c[a + b3 + k - 1], rng);
            memcpy(p + b3 + k, T.c + a + b3 + k, (size_t) (m - b3 - k));
            for (int bi = 0; bi < nb; ++bi) check(T, kind, p, m, os[oi], bs[bi], "leave", false);
          }
        }
      }
    }
  return cases - before;
}

long comeback(Rng& rng)
{
  const long before = cases;
  Text T;
  uint8_t p[MAXM + 4];
  const int ns[3] = { 300, 303, 320 };
  for (int kind = 0; kind < 6; ++kind)
    for (int ni = 0; ni < 3; ++ni) {
      make_text(T, kind, ns[ni], rng);
      for (int mi = 0; mi < 4; ++mi) {
        const int m = PIN_M[mi], last = T.n - m;
        for (int w = 1; w <= 15; ++w) {
          const int k = w + 1, a3 = m / 3, b3 = 2 * m / 3;
          if (!fits(m, k)) continue;
          int bs[3], nb;
          bands_of(w, bs, nb);
          const int os[3] = { 0, last - 16, last / 2 };   /* n >= m + 44: the k bases past the window are text */
          for (int oi = 0; oi < 3; ++oi) {
            const int a = os[oi];
            memcpy(p, T.c + a, (size_t) a3);
            for (int i = 0; i < k; ++i) p[a3 + i] = other(T.c[a + a3], i ? p[a3 + i - 1] : T.c[a + a3 - 1], rng);
            memcpy(p + a3 + k, T.c + a + a3, (size_t) (b3 - a3 - k));
            memcpy(p + b3, T.c + a + b3, (size_t) (m - b3));
            for (int bi = 0; bi < nb; ++bi) check(T, kind, p, m, os[oi], bs[bi], "comeback", false);
          }
        }
      }
    }
  return cases - before;
}

}  // namespace

int main()
{
  Rng rng = { 20260421u };
  printf("sweep %ld\n", sweep(rng));
  printf("ends %ld\n", ends(rng));
  printf("edge %ld\n", edge(rng));
  printf("indel %ld\n", indel(rng));
  printf("leave %ld\n", leave(rng));
  printf("comeback %ld\n", comeback(rng));
  if (bad_lim) { printf("FAILED: %d candidates take more words than the kernel holds\n", bad_lim); return 1; }
  if (failures) { printf("FAILED %ld of %ld\n", failures, cases); return 1; }
  printf("OK %ld\n", cases);
  return 0;
}
