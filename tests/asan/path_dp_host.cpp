/*
 * path_dp_host.cpp -- TEST HARNESS: csrc/hip/kfmi_path_dp.h compiled for the
 * host (g++, AddressSanitizer + UBSan) and compared with a plain full-table
 * dynamic programme and walk written from the definition of kstep_fmi.h
 * ("align paths").
 *
 * The code words and the window words are built the way paths_kernel builds
 * them: the read's last base in the low bits of cw[0]; the text's word stream
 * with bit 2g = text base n - 1 - g, addressed through a stream with one word
 * in front (off = n - c - m for the band's centre c = min(B, n - m), g = off +
 * 16 - w, w0 = g >> 4, sh = g & 15, lim words, zero where the stream holds no
 * text).  band_rows_keep keeps its rows in a plain array of m x 3 words,
 * band_value gives D from the last row and band_walk reads the rows back;
 * <16> runs at every length, <8> as well up to 128 bases.  Compared: whether
 * the task has a path at all, D, the end position and every run.
 *
 * Cases: four text kinds (all-A, period 2, period 3, random) x n in 5, 12, 20,
 * 40, 257, 300, 303, 320 (the first three shorter than the widest band) x every
 * m of 1, 15, 16, 17, 100, 128, 129, 255, 256 that fits x every band 0..15 x 32
 * begin positions: min(i, n) and max(n - i, 0) for i = 0..15, so B > n - m (c <
 * B), B - c > w (no path) and B = n are among them.  The read is the window at
 * B moved by up to +-w, with 0-3 random edits.
 *
 * Prints "cases <count>" and "paths <count with a path>", then "OK <cases>";
 * exits 0 when every case agrees.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../k-step_fm-index_amd/csrc/hip/kfmi_path_dp.h"

namespace {

enum { MAXN = 320, MAXM = 256, INF = 1 << 28, MAXRUNS = 2 * (MAXM + 31) + 1 };

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

const char* const KINDS[4] = { "all-A", "period-2", "period-3", "random" };

void make_text(Text& T, int kind, int n, Rng& rng)
{
  T.n = n;
  for (int i = 0; i < n; ++i) switch (kind) {
      case 0: T.c[i] = 0; break;
      case 1: T.c[i] = (uint8_t) (1 + (i & 1)); break;          /* CGCG.. */
      case 2: T.c[i] = (uint8_t) ("\0\1\3"[i % 3]); break;       /* ACTACT.. */
      default: T.c[i] = (uint8_t) rng.below(4);
    }
  memset(T.stream, 0, sizeof T.stream);
  for (int g = 0; g < n; ++g) T.stream[g >> 4] |= (uint32_t) T.c[n - 1 - g] << (2 * (g & 15));
}

struct Path {
  bool has;
  long D, end;
  int nruns;
  uint32_t runs[MAXRUNS];
};

void push(Path& P, uint32_t& op, uint32_t& len, uint32_t o)
{
  if (o == op) { ++len; return; }
  if (len) P.runs[P.nruns++] = len << 4 | op;
  op = o;
  len = 1;
}

/* the definition: the table A(i, d) around c and the walk from (0, B - c) */
void plain_path(const Text& T, const uint8_t* p, int m, long B, int w, Path& P)
{
  static int A[MAXM + 1][31];
  const long n = T.n;
  P.has = false;
  P.D = P.end = -1;
  P.nruns = 0;
  if (n < m || B > n) return;
  const long c = B < n - m ? B : n - m;
  if (B - c > w) return;
  for (int i = m; i >= 0; --i)
    for (int d = w; d >= -w; --d) {          /* d + 1 of the same row first */
      const long j = c + i + d;
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
  int i = 0, d = (int) (B - c), v = A[0][d + w];
  if (v >= INF) return;
  P.has = true;
  P.D = v;
  uint32_t op = 0, len = 0;
  while (i < m) {
    const long j = c + i + d;
    if (d + 1 <= w && j < n && A[i][d + 1 + w] + 1 == v) { push(P, op, len, 2u); ++d; --v; }
    else if (d - 1 >= -w && A[i + 1][d - 1 + w] + 1 == v) { push(P, op, len, 1u); ++i; --d; --v; }
    else {
      if (!(j < n) || A[i + 1][d + w] + (p[i] != T.c[j]) != v) { fprintf(stderr, "the plain walk is stuck\n"); exit(2); }
      const int x = p[i] != T.c[j];
      push(P, op, len, x ? 8u : 7u);
      ++i;
      v -= x;
    }
  }
  if (len) P.runs[P.nruns++] = len << 4 | op;
  P.end = c + m + d;
}

int bad_lim = 0;

struct Kept {
  uint32_t w[MAXM][3];
  void operator()(uint32_t r, uint32_t vp, uint32_t hp, uint32_t eq) { w[r][0] = vp; w[r][1] = hp; w[r][2] = eq; }
};
struct Back {
  const Kept* k;
  void operator()(uint32_t r, uint32_t& vp, uint32_t& hp, uint32_t& eq) { vp = k->w[r][0]; hp = k->w[r][1]; eq = k->w[r][2]; }
};
struct Runs {
  Path* P;
  void operator()(uint32_t op, uint32_t len) { P->runs[P->nruns++] = len << 4 | op; }
};

/* the same task through the header, the words staged as paths_kernel stages them */
template <int MAXW>
void header_path(const Text& T, const uint8_t* p, int m, uint32_t B, uint32_t w, Path& P)
{
  static Kept kept;
  const uint32_t n = (uint32_t) T.n;
  P.has = false;
  P.D = P.end = -1;
  P.nruns = 0;
  const bool in = n >= (uint32_t) m && B <= n;
  const uint32_t c = in ? (B < n - (uint32_t) m ? B : n - (uint32_t) m) : 0u;
  if (!in || B - c > w) return;
  uint32_t cw[MAXW], tx[MAXW + 3];
  for (int j = 0; j < MAXW; ++j) cw[j] = 0u;
  for (int i = 0; i < m; ++i) {
    const int r = m - 1 - i;
    cw[r >> 4] |= (uint32_t) p[i] << (2 * (r & 15));
  }
  const uint32_t off = n - c - (uint32_t) m, g = off + 16u - w, w0 = g >> 4, sh = g & 15u;
  const uint32_t lim = ((sh + (uint32_t) m - 1u + 2u * w) >> 4) + 1u, wtext = (n - 1u) >> 4;
  if (lim > (uint32_t) MAXW + 3u) ++bad_lim;
  for (int j = 0; j < MAXW + 3; ++j) {
    const uint32_t x = w0 + (uint32_t) j;
    tx[j] = ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) ? T.stream[x - 1u] : 0u;
  }
  memset(&kept, 0xEE, sizeof kept);   /* rows the pass does not write must not matter */
  uint32_t vp, vn, s0;
  kfmi::band_rows_keep<MAXW>(cw, tx, (uint32_t) m, w, sh, w > off ? w - off : 0u, kept, vp, vn, s0);
  const uint32_t k0 = w - (B - c);
  P.has = true;
  P.D = kfmi::band_value(vp, vn, s0, k0);
  Back back = { &kept };
  Runs runs = { &P };
  P.end = kfmi::band_walk((uint32_t) m, w, B, n, k0, back, runs);
}

long cases = 0, with_path = 0, failures = 0;

bool same(const Path& a, const Path& b)
{
  if (a.has != b.has) return false;
  if (!a.has) return true;
  return a.D == b.D && a.end == b.end && a.nruns == b.nruns && !memcmp(a.runs, b.runs, sizeof(uint32_t) * (size_t) a.nruns);
}

void check(const Text& T, int kind, const uint8_t* p, int m, int B, int w)
{
  static Path want, got;
  ++cases;
  plain_path(T, p, m, B, w, want);
  with_path += want.has;
  header_path<16>(T, p, m, (uint32_t) B, (uint32_t) w, got);
  bool ok = same(got, want);
  if (ok && m <= 128) {
    header_path<8>(T, p, m, (uint32_t) B, (uint32_t) w, got);
    ok = same(got, want);
  }
  if (!ok && ++failures <= 20)
    fprintf(stderr, "FAIL %s n %d m %d B %d band %d: header (%d %ld %ld, %d runs), want (%d %ld %ld, %d runs)\n", KINDS[kind],
            T.n, m, B, w, (int) got.has, got.D, got.end, got.nruns, (int) want.has, want.D, want.end, want.nruns);
}

uint8_t other(uint8_t a, Rng& rng)
{
  for (;;) {
    const uint8_t x = (uint8_t) rng.below(4);
    if (x != a) return x;
  }
}

int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

const int NS[8] = { 5, 12, 20, 40, 257, 300, 303, 320 };
const int MS[9] = { 1, 15, 16, 17, 100, 128, 129, 255, 256 };

}  // namespace

int main()
{
  Rng rng = { 20261021u };
  Text T;
  uint8_t p[MAXM + 4];
  for (int kind = 0; kind < 4; ++kind)
    for (int ni = 0; ni < 8; ++ni) {
      make_text(T, kind, NS[ni], rng);
      const int n = T.n;
      for (int mi = 0; mi < 9; ++mi) {
        const int m = MS[mi];
        if (m > n) continue;
        for (int w = 0; w <= 15; ++w)
          for (int bi = 0; bi < 32; ++bi) {
            const int B = bi < 16 ? (bi < n ? bi : n) : (n - (bi - 16) > 0 ? n - (bi - 16) : 0);
            const int a = clampi(B + (int) rng.below(2u * (uint32_t) w + 1u) - w, 0, n - m);
            memcpy(p, T.c + a, (size_t) m);
            for (int e = (int) (cases & 3); e > 0; --e) {
              const int at = (int) rng.below((uint32_t) m), what = m >= 2 ? (int) rng.below(3) : 0;
              if (what == 0) p[at] = other(p[at], rng);
              else if (what == 1) { memmove(p + at + 1, p + at, (size_t) (m - 1 - at)); p[at] = (uint8_t) rng.below(4); }
              else { memmove(p + at, p + at + 1, (size_t) (m - 1 - at)); p[m - 1] = (uint8_t) rng.below(4); }
            }
            check(T, kind, p, m, B, w);
          }
      }
    }
  printf("cases %ld\n", cases);
  printf("paths %ld\n", with_path);
  if (bad_lim) { printf("FAILED: %d tasks take more words than the kernel holds\n", bad_lim); return 1; }
  if (failures) { printf("FAILED %ld of %ld\n", failures, cases); return 1; }
  printf("OK %ld\n", cases);
  return 0;
}
