/*
 * window_dp_host.cpp -- TEST HARNESS: csrc/hip/kfmi_window_dp.h compiled for
 * the host (g++, AddressSanitizer + UBSan) and compared with a plain full
 * table written from the definition of kstep_fmi.h ("place windows / pairs").
 *
 * The words are staged the way window_kernel stages them: the read's last base
 * in the low bits of cw[0]; the text's word stream with bit 2g = text base
 * n - 1 - g in a heap array of exactly n / 16 + 2 words, so a word index past
 * the stream is a sanitizer report; the scan from g = n - T up to n - 1 - lo
 * with the next word fetched one ahead.  The plain table runs out to the text's
 * end n -- it knows no scan bound -- so the bound is under test.  Each case runs
 * through every instantiated word count NW of 1, 2, 4, 8 with 32 NW >= m and
 * compares x, y of the record and, for a hit, B_max.
 *
 * Families (four text kinds each: all-A, period 2, period 3, random):
 *   sweep  n = 700; m in 1, 2, 31, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256;
 *          window lengths 1, 2, 31, 32, 33, 100, 400; the window at the text's
 *          start, over its end and in the middle; 0 .. 8 planted unit edits in
 *          a read taken from inside the window; max_edits by turns the number
 *          planted, one less, and m;
 *   long   m in 63 .. 256 of the list; one deletion and one insertion of 16,
 *          17, 18, 19, 20 bases at m / 2; window 33; max_edits the indel;
 *   short  texts of 1, 5 and 30 bases, every m of the list above n; the windows
 *          (0, 33) and (n, 1); max_edits m;
 *   tight  every m >= 33 of the list; K = 1, 3, 8 text bases skipped at m / 2,
 *          the window's last position the read's origin, max_edits = K: the
 *          placement ends on the scan end exactly.
 *
 * Prints one line "<family> <cases>" per family, "hits <n>" and "OK <cases>";
 * exits 0 when every case agrees.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../k-step_fm-index_amd/csrc/hip/kfmi_window_dp.h"

namespace {

const int MS[13] = { 1, 2, 31, 32, 33, 63, 64, 65, 100, 128, 129, 255, 256 };
const int LENS[7] = { 1, 2, 31, 32, 33, 100, 400 };

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); }
  uint32_t below(uint32_t k) { return next() % k; }
};

struct Text {
  int n;
  std::vector<uint8_t> c;
  std::vector<uint32_t> stream;   /* bit 2g: text base n - 1 - g; n / 16 + 2 words */
};

void make_text(Text& T, int kind, int n, Rng& rng)
{
  T.n = n;
  T.c.assign((size_t) n, 0);
  for (int i = 0; i < n; ++i) switch (kind) {
      case 0: T.c[i] = 0; break;
      case 1: T.c[i] = (uint8_t) (1 + (i & 1)); break;
      case 2: T.c[i] = (uint8_t) ("\0\1\3"[i % 3]); break;
      default: T.c[i] = (uint8_t) rng.below(4);
    }
  T.stream.assign((size_t) n / 16 + 2, 0u);
  for (int g = 0; g < n; ++g) T.stream[(size_t) g >> 4] |= (uint32_t) T.c[n - 1 - g] << (2 * (g & 15));
}

struct Rec { uint32_t x, y, bmax; };

/* the definition out to n: A(i, j) in two rows, then the record */
Rec plain(const Text& T, const uint8_t* p, int m, uint32_t lo, uint32_t len, uint32_t max_edits)
{
  const long n = T.n;
  std::vector<int> nxt((size_t) n + 1, 0), cur((size_t) n + 1, 0);
  for (int i = m - 1; i >= 0; --i) {
    cur[(size_t) n] = nxt[(size_t) n] + 1;
    for (long j = n - 1; j >= 0; --j) {
      int v = nxt[(size_t) j + 1] + (p[i] != T.c[(size_t) j]);
      if (nxt[(size_t) j] + 1 < v) v = nxt[(size_t) j] + 1;
      if (cur[(size_t) j + 1] + 1 < v) v = cur[(size_t) j + 1] + 1;
      cur[(size_t) j] = v;
    }
    nxt.swap(cur);
  }
  long E = -1, bmin = 0, bmax = 0;
  for (long b = lo; b < (long) lo + (long) len && b <= n; ++b) {
    const int v = nxt[(size_t) b];
    if (E < 0 || v < E) { E = v; bmin = bmax = b; }
    else if (v == E) bmax = b;
  }
  Rec r = { 0xFFFFFFFFu, 0u, 0u };
  if (E >= 0 && (uint64_t) E <= max_edits) {
    r.x = (uint32_t) bmin;
    r.y = (uint32_t) E | (bmax > bmin ? 0x00010000u : 0u);
    r.bmax = (uint32_t) bmax;
  }
  return r;
}

/* the header, staged and scanned as window_kernel does */
template <int NW>
Rec header(const Text& T, const uint8_t* p, int m, uint32_t lo, uint32_t len, uint32_t max_edits)
{
  constexpr int MAXW = NW <= 4 ? 8 : 16;
  uint32_t cw[MAXW];
  for (int j = 0; j < MAXW; ++j) cw[j] = 0u;
  for (int i = 0; i < m; ++i) {
    const int r = m - 1 - i;
    cw[r >> 4] |= (uint32_t) p[i] << (2 * (r & 15));
  }
  const uint32_t n = (uint32_t) T.n, um = (uint32_t) m;
  uint32_t hi_b = 0u, Tend = 0u, E = 0xFFFFFFFFu, bmin = 0u, bmax = 0u;
  const int any = kfmi::window_scan(n, lo, len, um, max_edits, &hi_b, &Tend);
  if (any) {
    uint32_t peq[4][NW], pv[NW], mv[NW];
    kfmi::window_match_words<NW, MAXW>(cw, um, peq);
    kfmi::window_first_column<NW>(pv, mv);
    uint32_t score = um;
    if (hi_b == n) kfmi::window_fold(score, n, E, bmin, bmax);
    uint32_t g = n - Tend;
    const uint32_t gend = n - lo;
    if (g < gend) {
      const uint32_t xl = (gend - 1u) >> 4;
      uint32_t word = T.stream.at(g >> 4);
      uint32_t next = (g >> 4) < xl ? T.stream.at((g >> 4) + 1u) : 0u;
      while (g < gend) {
        const uint32_t c = (word >> (2u * (g & 15u))) & 3u;
        score += (uint32_t) kfmi::window_step<NW>(peq, pv, mv, um, c);
        const uint32_t j = n - 1u - g;
        if (j <= hi_b) kfmi::window_fold(score, j, E, bmin, bmax);
        ++g;
        if ((g & 15u) == 0u && g < gend) {
          word = next;
          if ((g >> 4) < xl) next = T.stream.at((g >> 4) + 1u);
        }
      }
    }
  }
  Rec r = { 0u, 0u, 0u };
  kfmi::window_record(any, E, bmin, bmax, max_edits, &r.x, &r.y);
  r.bmax = r.x != 0xFFFFFFFFu ? bmax : 0u;
  return r;
}

long cases = 0, hits = 0, bad = 0;

void compare(const char* fam, const Text& T, int kind, const uint8_t* p, int m, uint32_t lo, uint32_t len, uint32_t me)
{
  const Rec want = plain(T, p, m, lo, len, me);
  for (int nw = 1; nw <= 8; nw *= 2) {
    if (32 * nw < m) continue;
    const Rec got = nw == 1 ? header<1>(T, p, m, lo, len, me) : nw == 2 ? header<2>(T, p, m, lo, len, me)
                  : nw == 4 ? header<4>(T, p, m, lo, len, me) : header<8>(T, p, m, lo, len, me);
    ++cases;
    if (want.x != 0xFFFFFFFFu) ++hits;
    if (got.x != want.x || got.y != want.y || got.bmax != want.bmax) {
      if (bad++ < 10)
        fprintf(stderr, "%s kind %d n %d m %d lo %u len %u me %u NW %d: got %u %x %u want %u %x %u\n", fam, kind, T.n, m,
                lo, len, me, nw, got.x, got.y, got.bmax, want.x, want.y, want.bmax);
    }
  }
}

/* m bases read off the text from o on with `edits` unit edits planted; bases past the text are random */
void planted(const Text& T, int o, int m, int edits, Rng& rng, uint8_t* p)
{
  std::vector<uint8_t> r;
  for (int i = 0; i < m + 16; ++i) r.push_back(o + i < T.n ? T.c[(size_t) (o + i)] : (uint8_t) rng.below(4));
  for (int e = 0; e < edits; ++e) {
    const size_t at = rng.below((uint32_t) m);
    switch (rng.below(3)) {
      case 0: r[at] = (uint8_t) ((r[at] + 1 + rng.below(3)) & 3); break;
      case 1: r.erase(r.begin() + (long) at); break;
      default: r.insert(r.begin() + (long) at, (uint8_t) rng.below(4));
    }
  }
  for (int i = 0; i < m; ++i) p[i] = r[(size_t) i];
}

}  // namespace

int main()
{
  Rng rng{20240623};
  uint8_t p[256];
  long before;
  Text T;
  /* sweep */
  before = cases;
  for (int kind = 0; kind < 4; ++kind) {
    make_text(T, kind, 700, rng);
    for (int m : MS)
      for (int len : LENS)
        for (int e = 0; e <= 8; ++e)
          for (int pos = 0; pos < 3; ++pos) {
            const int n = T.n;
            const uint32_t lo = pos == 0 ? 0u : pos == 1 ? (uint32_t) (n - len / 2) : 20u + rng.below((uint32_t) (n - len - m - 40));
            const int o = (int) lo + (int) rng.below((uint32_t) len);   /* may lie past n - m, or past n */
            planted(T, o < n ? o : n - 1, m, e, rng, p);
            const uint32_t me = e % 3 == 0 ? (uint32_t) e : e % 3 == 1 ? (uint32_t) (e - 1) : (uint32_t) m;
            compare("sweep", T, kind, p, m, lo, (uint32_t) len, me);
          }
  }
  printf("sweep %ld\n", cases - before);
  /* long */
  before = cases;
  for (int kind = 0; kind < 4; ++kind) {
    make_text(T, kind, 700, rng);
    for (int m : MS) {
      if (m < 63) continue;
      for (int k = 16; k <= 20; ++k)
        for (int ins = 0; ins < 2; ++ins) {
          const int o = 100 + (int) rng.below(200), h = m / 2;
          int q = 0;
          for (int i = 0; i < h; ++i) p[q++] = T.c[(size_t) (o + i)];
          if (ins) {
            for (int i = 0; i < k; ++i) p[q++] = (uint8_t) rng.below(4);
            for (int i = h; q < m; ++i) p[q++] = T.c[(size_t) (o + i)];
          } else {
            for (int i = h + k; q < m; ++i) p[q++] = T.c[(size_t) (o + i)];
          }
          compare("long", T, kind, p, m, (uint32_t) (o - 16), 33u, (uint32_t) k);
        }
    }
  }
  printf("long %ld\n", cases - before);
  /* short */
  before = cases;
  for (int kind = 0; kind < 4; ++kind)
    for (int n : { 1, 5, 30 }) {
      make_text(T, kind, n, rng);
      for (int m : MS) {
        if (m <= n) continue;
        planted(T, 0, m, 0, rng, p);
        compare("short", T, kind, p, m, 0u, 33u, (uint32_t) m);
        compare("short", T, kind, p, m, (uint32_t) n, 1u, (uint32_t) m);
      }
    }
  printf("short %ld\n", cases - before);
  /* tight */
  before = cases;
  for (int kind = 0; kind < 4; ++kind) {
    make_text(T, kind, 700, rng);
    for (int m : MS) {
      if (m < 33) continue;
      for (int K : { 1, 3, 8 }) {
        const int o = 100 + (int) rng.below(200), h = m / 2;
        int q = 0;
        for (int i = 0; i < h; ++i) p[q++] = T.c[(size_t) (o + i)];
        for (int i = h + K; q < m; ++i) p[q++] = T.c[(size_t) (o + i)];
        compare("tight", T, kind, p, m, (uint32_t) (o - 32), 33u, (uint32_t) K);
      }
    }
  }
  printf("tight %ld\n", cases - before);
  printf("hits %ld\n", hits);
  if (bad) {
    fprintf(stderr, "%ld of %ld cases differ\n", bad, cases);
    return 1;
  }
  printf("OK %ld\n", cases);
  return 0;
}
