/*
 * kfmi_sam.h -- the per-task arithmetic of kfmi_sam_lines (kstep_fmi.h, "SAM
 * lines"): a task's status, the exact length of its line from the records
 * alone, and the bytes of the line.  Plain C on u32 record words, so the host
 * form (csrc/host/sam.c) and the kernels (csrc/hip/kfmi_sam.hip) compile the
 * same text; tests/sam_ref.py states it again as Python string formatting.
 *
 * Two things differ between the two sides and are left to the includer: where
 * a text base comes from (KFMI_SAM_TEXT(src, p), the 2-bit code of text
 * position p: the ASCII text on the host, the lane's BandWindow on the device)
 * and how SEQ is written (from ASCII, from code words in registers).  A line is
 * therefore written in three steps: the front up to the tab before SEQ, SEQ by
 * the includer, the back from the tab after SEQ.
 *
 * Bound of a line.  QNAME <= 20 digits, FLAG <= 2, RNAME <= 254, POS <= 10,
 * MAPQ <= 3; CIGAR: at most 2 * KFMI_PATH_MAX_ENTRIES = 64 runs of at most 3
 * digits and a letter (a run is at most m + band <= 271 bases), 256; SEQ <= 256;
 * NM:i: and at most 5 digits; MD:Z: and at most one count per X base, D run
 * and line end (<= 272, each one digit, plus at most m / 10 + m / 100 = 27
 * further digits, since a count of k digits follows 10^(k-1) matched bases),
 * one letter per text base under X or D (<= 271) and one ^ per D run (<= 32),
 * 602; the constant fields "*", "0", "0", "*", 12 tabs and the newline, 17.
 * Together at most 20 + 2 + 254 + 10 + 3 + 256 + 256 + 10 + 5 + 602 + 17 =
 * 1435 <= KFMI_SAM_LINE_MAX.  kfmi_sam_status makes SPAN of every record whose
 * runs do not add up to m read bases and end - B text bases, so the bound holds
 * of whatever the handles contain.
 */
#ifndef KFMI_SAM_H_
#define KFMI_SAM_H_

#include <stdint.h>

#include "kfmi_internal.h"

#if defined(__HIPCC__)
#define KFMI_SAM_FN __host__ __device__ __forceinline__
#define KFMI_SAM_SRC_FN template <class Src> __device__ __forceinline__
#define KFMI_SAM_SRC_ARG const Src&
/* A lane's loops stay scalar loops: vectorised, the byte loops cost the write kernel 100 registers and more. */
#define KFMI_SAM_ROLLED _Pragma("clang loop vectorize(disable) unroll(disable)")
#define KFMI_SAM_DST uint8_t *
#else
#define KFMI_SAM_FN static inline
#define KFMI_SAM_SRC_FN static inline
#define KFMI_SAM_SRC_ARG const kfmi_sam_src
#define KFMI_SAM_ROLLED
#define KFMI_SAM_DST uint8_t *
#endif

/* a task's status, in the order of the unmapped line's YU code; OK is not a code of a line */
enum { KFMI_SAM_NONE = 0, KFMI_SAM_OVERFLOW = 1, KFMI_SAM_SPAN = 2, KFMI_SAM_OK = 3 };

#define KFMI_SAM_LINE_MAX 1536u
#define KFMI_SAM_NO_CONTIG 0xFFFFFFFFu
/* what the length pass leaves per task: the line's bytes (0: the task writes none), which line, the YU code */
#define KFMI_SAM_LEN_MASK   0x0000FFFFu
#define KFMI_SAM_MAPPED     0x00010000u
#define KFMI_SAM_UNMAPPED   0x00020000u
#define KFMI_SAM_CODE_SHIFT 18

/* the table as both sides read it: name i is names[name_off[i] .. name_off[i + 1]) */
typedef struct {
  const uint32_t *begins, *lengths, *name_off;
  const uint8_t *names;
  uint32_t count;
} kfmi_sam_table;

/* what the walk over a task's runs finds: read and text bases used, bytes of CIGAR and of the MD string */
typedef struct {
  uint32_t read, text, cigar, md, valid;
} kfmi_sam_runs;

KFMI_SAM_FN uint32_t kfmi_sam_digits(uint64_t v)
{
  uint32_t d = 1u;
  KFMI_SAM_ROLLED
  while (v >= 10u) {
    v /= 10u;
    ++d;
  }
  return d;
}

/* v in decimal at dst[pos ..]; returns the position after it */
KFMI_SAM_FN uint32_t kfmi_sam_put_dec(KFMI_SAM_DST dst, uint32_t pos, uint64_t v)
{
  const uint32_t d = kfmi_sam_digits(v);
  uint32_t k;
  KFMI_SAM_ROLLED
  for (k = d; k-- > 0u;) {
    dst[pos + k] = (uint8_t) ('0' + (uint32_t) (v % 10u));
    v /= 10u;
  }
  return pos + d;
}

KFMI_SAM_FN uint32_t kfmi_sam_put_str(KFMI_SAM_DST dst, uint32_t pos, const char *s, uint32_t len)
{
  uint32_t k;
  KFMI_SAM_ROLLED
  for (k = 0; k < len; ++k) dst[pos + k] = (uint8_t) s[k];
  return pos + len;
}

/* "ACGT"[code] without a table */
KFMI_SAM_FN uint8_t kfmi_sam_letter(uint32_t code) { return (uint8_t) (0x54474341u >> (8u * (code & 3u))); }
/* "MIDNSHP=X"[op] for the ops a path holds and M */
KFMI_SAM_FN uint8_t kfmi_sam_op(uint32_t op)
{
  return (uint8_t) (op == 7u ? '=' : op == 8u ? 'X' : op == 1u ? 'I' : op == 2u ? 'D' : 'M');
}

/* the contig that holds [B, end): the last one that begins at or before B, by binary search, if it ends at or after
 * `end`; contigs ascend and do not overlap, so no other one can */
KFMI_SAM_FN uint32_t kfmi_sam_contig(const kfmi_sam_table *tab, uint32_t B, uint32_t end)
{
  uint32_t lo = 0u, hi = tab->count;   /* begins[lo - 1] <= B < begins[hi] */
  KFMI_SAM_ROLLED
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (tab->begins[mid] <= B) lo = mid + 1u;
    else hi = mid;
  }
  if (lo == 0u) return KFMI_SAM_NO_CONTIG;
  --lo;
  return (uint64_t) end <= (uint64_t) tab->begins[lo] + tab->lengths[lo] ? lo : KFMI_SAM_NO_CONTIG;
}

/* One walk over a task's `runs` words: what they use and what they cost.  valid: every run is I, D, = or X of at
 * least one base.  Under KFMI_SAM_CIGAR_M adjacent = and X runs are one M run. */
KFMI_SAM_FN kfmi_sam_runs kfmi_sam_walk(const uint32_t *cig, uint32_t runs, uint32_t options)
{
  kfmi_sam_runs o = {0u, 0u, 0u, 0u, 1u};
  uint32_t c = 0u, macc = 0u, r;
  KFMI_SAM_ROLLED
  for (r = 0; r < runs; ++r) {
    const uint32_t op = cig[r] & 15u, len = cig[r] >> 4;
    const int diag = op == 7u || op == 8u;
    if (len == 0u || !(diag || op == 1u || op == 2u)) o.valid = 0u;
    if (op != 2u) o.read += len;
    if (op != 1u) o.text += len;
    if (diag && (options & KFMI_SAM_CIGAR_M)) macc += len;
    else {
      if (macc) o.cigar += kfmi_sam_digits(macc) + 1u;
      macc = 0u;
      o.cigar += kfmi_sam_digits(len) + 1u;
    }
    if (op == 7u) c += len;
    else if (op == 8u) {   /* per base the count and a letter; the count is 0 after the first */
      o.md += kfmi_sam_digits(c) + 1u + 2u * (len - 1u);
      c = 0u;
    } else if (op == 2u) {
      o.md += kfmi_sam_digits(c) + 1u + len;
      c = 0u;
    }
  }
  if (macc) o.cigar += kfmi_sam_digits(macc) + 1u;
  o.md += kfmi_sam_digits(c);
  return o;
}

/* The status of one task: B word x of its hit, (px, py) its path record, cig its 2C words; *contig and *walk are
 * set where the status is KFMI_SAM_OK. */
KFMI_SAM_FN uint32_t kfmi_sam_status(const kfmi_sam_table *tab, uint32_t n, uint32_t m, uint32_t band, uint32_t C,
                                     uint32_t options, uint32_t B, uint32_t px, uint32_t py, const uint32_t *cig,
                                     uint32_t *contig, kfmi_sam_runs *walk)
{
  const uint32_t runs = (py >> KFMI_PATH_RUNS_SHIFT) & KFMI_PATH_RUNS_MASK;
  uint32_t c, i;
  if (px == KFMI_HIT_NONE) return KFMI_SAM_NONE;
  if (py & KFMI_PATH_OVERFLOW) return KFMI_SAM_OVERFLOW;
  if (n < m || B > n || px <= B) return KFMI_SAM_SPAN;   /* px == B: a path of insertions only uses no text base */
  c = B < n - m ? B : n - m;
  if (B - c > band || (uint64_t) px > (uint64_t) c + m + band) return KFMI_SAM_SPAN;   /* outside the band's window */
  if (runs == 0u || runs > 2u * C) return KFMI_SAM_SPAN;
  i = kfmi_sam_contig(tab, B, px);
  if (i == KFMI_SAM_NO_CONTIG) return KFMI_SAM_SPAN;
  *walk = kfmi_sam_walk(cig, runs, options);
  if (!walk->valid || walk->read != m || walk->text != px - B) return KFMI_SAM_SPAN;
  *contig = i;
  return KFMI_SAM_OK;
}

/* Which of a read's tasks writes its line, from the two statuses and edits of BOTH mode (one strand: pass the task
 * as `own` with both = 0).  Returns 0 (this task writes nothing), KFMI_SAM_MAPPED, or KFMI_SAM_UNMAPPED | code <<
 * KFMI_SAM_CODE_SHIFT: the unmapped line is the FWD task's. */
KFMI_SAM_FN uint32_t kfmi_sam_choice(int both, int rev, uint32_t own, uint32_t own_d, uint32_t mate, uint32_t mate_d)
{
  if (!both) return own == KFMI_SAM_OK ? KFMI_SAM_MAPPED : KFMI_SAM_UNMAPPED | own << KFMI_SAM_CODE_SHIFT;
  if (own == KFMI_SAM_OK)
    return mate != KFMI_SAM_OK || own_d < mate_d || (own_d == mate_d && !rev) ? KFMI_SAM_MAPPED : 0u;
  if (mate == KFMI_SAM_OK || rev) return 0u;
  return KFMI_SAM_UNMAPPED | (own > mate ? own : mate) << KFMI_SAM_CODE_SHIFT;
}

/* MAPQ from word x of the task's quality record, where there is one */
KFMI_SAM_FN uint32_t kfmi_sam_mapq(int have, uint32_t x) { return !have ? 255u : x < 254u ? x : 254u; }

/* bytes of a mapped line: 12 tabs, the newline, "*", "0", "0", "*", "NM:i:", "MD:Z:" are 27 */
KFMI_SAM_FN uint32_t kfmi_sam_mapped_len(const kfmi_sam_table *tab, uint32_t contig, uint64_t qname, int rev,
                                         uint32_t B, uint32_t mapq, uint32_t m, uint32_t d, const kfmi_sam_runs *walk)
{
  return kfmi_sam_digits(qname) + (rev ? 2u : 1u) + (tab->name_off[contig + 1u] - tab->name_off[contig]) +
         kfmi_sam_digits(B - tab->begins[contig] + 1u) + kfmi_sam_digits(mapq) + walk->cigar + m +
         kfmi_sam_digits(d) + walk->md + 27u;
}

/* bytes of an unmapped line: "\t4\t*\t0\t0\t*\t*\t0\t0\t" 17, "\t*\tYU:i:" 8, the code, the newline */
KFMI_SAM_FN uint32_t kfmi_sam_unmapped_len(uint64_t qname, uint32_t m) { return kfmi_sam_digits(qname) + m + 27u; }

/* a mapped line up to the tab before SEQ */
KFMI_SAM_FN uint32_t kfmi_sam_put_front(KFMI_SAM_DST dst, uint32_t pos, const kfmi_sam_table *tab, uint32_t contig,
                                        uint64_t qname, int rev, uint32_t B, uint32_t mapq, const uint32_t *cig,
                                        uint32_t runs, uint32_t options)
{
  const uint32_t n0 = tab->name_off[contig], n1 = tab->name_off[contig + 1u];
  uint32_t macc = 0u, r, k;
  pos = kfmi_sam_put_dec(dst, pos, qname);
  dst[pos++] = '\t';
  pos = kfmi_sam_put_dec(dst, pos, rev ? 16u : 0u);
  dst[pos++] = '\t';
  KFMI_SAM_ROLLED
  for (k = n0; k < n1; ++k) dst[pos++] = tab->names[k];
  dst[pos++] = '\t';
  pos = kfmi_sam_put_dec(dst, pos, B - tab->begins[contig] + 1u);
  dst[pos++] = '\t';
  pos = kfmi_sam_put_dec(dst, pos, mapq);
  dst[pos++] = '\t';
  KFMI_SAM_ROLLED
  for (r = 0; r < runs; ++r) {
    const uint32_t op = cig[r] & 15u, len = cig[r] >> 4;
    if ((op == 7u || op == 8u) && (options & KFMI_SAM_CIGAR_M)) macc += len;
    else {
      if (macc) {
        pos = kfmi_sam_put_dec(dst, pos, macc);
        dst[pos++] = 'M';
        macc = 0u;
      }
      pos = kfmi_sam_put_dec(dst, pos, len);
      dst[pos++] = kfmi_sam_op(op);
    }
  }
  if (macc) {
    pos = kfmi_sam_put_dec(dst, pos, macc);
    dst[pos++] = 'M';
  }
  return kfmi_sam_put_str(dst, pos, "\t*\t0\t0\t", 7u);
}

/* an unmapped line up to the tab before SEQ, and from the tab after it */
KFMI_SAM_FN uint32_t kfmi_sam_put_unmapped_front(KFMI_SAM_DST dst, uint32_t pos, uint64_t qname)
{
  pos = kfmi_sam_put_dec(dst, pos, qname);
  return kfmi_sam_put_str(dst, pos, "\t4\t*\t0\t0\t*\t*\t0\t0\t", 17u);
}

KFMI_SAM_FN uint32_t kfmi_sam_put_unmapped_back(KFMI_SAM_DST dst, uint32_t pos, uint32_t code)
{
  pos = kfmi_sam_put_str(dst, pos, "\t*\tYU:i:", 8u);
  dst[pos++] = (uint8_t) ('0' + code);
  dst[pos++] = '\n';
  return pos;
}

/* The back of a mapped line, from the tab after SEQ: NM and the MD walk over the text from B on.  KFMI_SAM_TEXT(src, p)
 * -- and on the host the type kfmi_sam_src -- are the includer's, defined before it includes this file. */
KFMI_SAM_SRC_FN uint32_t kfmi_sam_put_back(KFMI_SAM_DST dst, uint32_t pos, uint32_t d, const uint32_t *cig, uint32_t runs,
                                           uint32_t B, KFMI_SAM_SRC_ARG src)
{
  uint32_t c = 0u, p = B, r, k;
  pos = kfmi_sam_put_str(dst, pos, "\t*\tNM:i:", 8u);
  pos = kfmi_sam_put_dec(dst, pos, d);
  pos = kfmi_sam_put_str(dst, pos, "\tMD:Z:", 6u);
  KFMI_SAM_ROLLED
  for (r = 0; r < runs; ++r) {
    const uint32_t op = cig[r] & 15u, len = cig[r] >> 4;
    if (op == 7u) {
      c += len;
      p += len;
    } else if (op == 8u) {
      KFMI_SAM_ROLLED
      for (k = 0; k < len; ++k) {
        pos = kfmi_sam_put_dec(dst, pos, c);
        dst[pos++] = kfmi_sam_letter(KFMI_SAM_TEXT(src, p));
        c = 0u;
        ++p;
      }
    } else if (op == 2u) {
      pos = kfmi_sam_put_dec(dst, pos, c);
      dst[pos++] = '^';
      KFMI_SAM_ROLLED
      for (k = 0; k < len; ++k) dst[pos++] = kfmi_sam_letter(KFMI_SAM_TEXT(src, p++));
      c = 0u;
    }
  }
  pos = kfmi_sam_put_dec(dst, pos, c);
  dst[pos++] = '\n';
  return pos;
}
#endif /* KFMI_SAM_H_ */
