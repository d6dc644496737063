/*
 * kfmi_align.hip -- seed alignment: the best banded edit-distance placement of
 * every task among the text positions its seeds imply (kstep_fmi.h section 2,
 * "align seeds"; not in the reference, which stops at
 * intervals).
 *
 * The frame is verify_kernel's (kfmi_verify.hip): one lane per task, the read
 * packed into registers by the search's own stagers with rem = 0, the same
 * slot / row generator, wave-uniform rounds in which every lane issues the
 * text-window loads of the candidate it holds together with the sa load of its
 * next row and waits once, and the 16-lane group mask where the tables are past
 * the translation reach.  The host side of a call is kfmi_verify.hip's
 * seed_score_call.
 *
 * What differs is the window and the score.  The window of origin o under band
 * w is the text at [o - w, o + m + w) clipped to the text: in the word stream,
 * whose bit 2g is text base n - 1 - g, the bases from off - w on with off =
 * n - o - m.  The lane addresses it through a stream with one word in front
 * (base off + 16 - w >= 1), so that the 15 cells that can lie past the text's
 * end need no signed arithmetic: word 0 of that stream and every word past the
 * text's last are not loaded and read as zero, and the cells they would serve
 * are invalid (kfmi_align_dp.h).  A candidate takes ((sh + m - 1 + 2w) >> 4) + 1
 * <= ceil((m + 2w) / 16) + 1 words.  The score is the bit-parallel banded
 * dynamic programme of kfmi_align_dp.h: m rows per candidate in every lane,
 * whatever the text holds, so only the candidate counts diverge, as in the
 * verify.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_runtime.h"
#include "kfmi_verify.h"
#include "kfmi_align_dp.h"

namespace kfmi {

/* STR: the strand staging (a.strands 2 = REV, 3 = BOTH: task 2q + strand), else forward reads. */
template <int MAXW, bool STR>
__global__ __launch_bounds__(256) void align_kernel(VerifyArgs a, uint32_t band)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  if constexpr (STR) {
    stage_strand_codes<MAXW>(a.ascii, a.num, a.m, stage, cw, a.strands);   /* whole block, before any exit */
  } else {
    uint32_t rc = 0;
    stage_query_codes<MAXW>(a.ascii, a.num, a.m, stage, cw, 0u, rc);       /* whole block, before any exit */
  }
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= (STR && a.strands == 3u ? 2u : 1u) * a.num) return;
  const uint32_t m = a.m, n = a.rows - 1u, w = band;
  const uint32_t* __restrict__ text = a.jsa + 2ull * a.rows;
  const uint2* __restrict__ ivt = a.iv + t * a.S;
  const uint2* __restrict__ spt = a.sp + t * a.S;
  const int grp = (int) (threadIdx.x & 63u) / 16;
  uint32_t s = 0, r = 0, rend = 0, start = 0;   /* the next slot, and the rows left of the current one */
  uint32_t p = 0, pstart = 0;                   /* the candidate in hand: its sa value and its slot's start */
  bool have = false;
  uint32_t E = 0xFFFFFFFFu, bmin = 0xFFFFFFFFu, bmax = 0u, scored = 0u;
  for (;;) {
    /* lanes out of rows take their next slot; an ignored slot leaves them out of rows */
    while (__ballot(r >= rend && s < a.S)) {
      if (r >= rend && s < a.S) {
        const uint2 lr = ivt[s], sl = spt[s];
        ++s;
        if (lr.y > lr.x && lr.x < a.rows && sl.y != 0u && (uint64_t) sl.x + sl.y <= m) {
          const uint64_t cap = (uint64_t) lr.x + a.max_occ;
          const uint32_t e = lr.y < a.rows ? lr.y : a.rows;
          r = lr.x;
          rend = cap < e ? (uint32_t) cap : e;
          start = sl.x;
        }
      }
    }
    const bool more = r < rend;   /* r < rows */
    if (!__ballot(more || have)) break;
    const bool sc = have && p < a.rows && p >= pstart && (uint64_t) (p - pstart) + m <= n;
    const uint32_t o = sc ? p - pstart : 0u;
    const uint32_t off = sc ? n - o - m : 0u;        /* the read's last base is base `off` of the stream */
    const uint32_t g = off + 16u - w;                /* the window's first base in the stream with a word in front */
    const uint32_t w0 = g >> 4, sh = g & 15u;
    const uint32_t lim = sc ? ((sh + m - 1u + 2u * w) >> 4) + 1u : 0u;   /* <= MAXW + 3 */
    const uint32_t wtext = sc ? (n - 1u) >> 4 : 0u;  /* sc: n >= m >= 1; the last word that holds text */
    uint32_t tx[MAXW + 3];
#pragma unroll
    for (int j = 0; j < MAXW + 3; ++j) tx[j] = 0u;
    uint32_t np = SKIP_NONE;
    if (a.split4) {   /* wave-uniform: all of a lane's loads under its group's mask */
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (grp == q) {
#pragma unroll
          for (int j = 0; j < MAXW + 3; ++j) {
            const uint32_t x = w0 + (uint32_t) j;   /* word x - 1 of the text's stream */
            if ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) tx[j] = text[x - 1u];
          }
          if (more) np = a.jsa[r];
        }
    } else {
#pragma unroll
      for (int j = 0; j < MAXW + 3; ++j) {
        const uint32_t x = w0 + (uint32_t) j;
        if ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) tx[j] = text[x - 1u];
      }
      if (more) np = a.jsa[r];
    }
    if (sc) {
      uint32_t vp, vn, s0;
      band_rows<MAXW>(cw, tx, m, w, sh, w > off ? w - off : 0u, vp, vn, s0);
      band_fold(vp, vn, s0, w, o, n, E, bmin, bmax);
      ++scored;
    }
    have = more;
    if (more) {
      p = np;
      pstart = start;
      ++r;
    }
  }
  const bool hit = scored != 0u && E <= a.max_mism;
  a.hits[t] = hit ? make_uint2(bmin, E | (bmax - bmin > 2u * w ? KFMI_HIT_MULTI : 0u) | (scored << KFMI_HIT_SCORED_SHIFT))
                  : make_uint2(KFMI_HIT_NONE, scored << KFMI_HIT_SCORED_SHIFT);
}

static hipError_t launch_align(const VerifyArgs& a, uint32_t band, hipStream_t st)
{
  const bool str = a.strands != KFMI_STRAND_FWD;
  const uint64_t tasks = (a.strands == KFMI_STRAND_BOTH ? 2u : 1u) * a.num;
  const dim3 grid((uint32_t) ((tasks + 255) / 256));
  const size_t lds = 4 * (size_t) stage_slot_bytes(a.m);
  if (a.m <= 128) {
    if (str) hipLaunchKernelGGL((align_kernel<8, true>), grid, dim3(256), lds, st, a, band);
    else hipLaunchKernelGGL((align_kernel<8, false>), grid, dim3(256), lds, st, a, band);
  } else {
    if (str) hipLaunchKernelGGL((align_kernel<16, true>), grid, dim3(256), lds, st, a, band);
    else hipLaunchKernelGGL((align_kernel<16, false>), grid, dim3(256), lds, st, a, band);
  }
  return hipGetLastError();
}

extern "C" int32_t kfmi_align_seeds(void* index, void* queries, void* intervals, void* spans, void* hits,
                                    uint32_t max_seeds, uint32_t strands, uint32_t max_occ, uint32_t band,
                                    uint32_t max_edits)
{
  if (band > KFMI_ALIGN_MAX_BAND) return KFMI_E_BAD_ARGUMENT;
  return seed_score_call(index, queries, intervals, spans, hits, max_seeds, strands, max_occ, band, max_edits,
                         launch_align);
}

}  // namespace kfmi
