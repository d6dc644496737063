/*
 * kfmi_align.hip -- seed alignment: the best banded edit-distance placement of
 * every task among the text positions its seeds imply (kstep_fmi.h section 2,
 * "align seeds"; not in the reference, which stops at
 * intervals).
 *
 * The frame is kfmi_text.h's: one lane per task, the read in registers, the
 * slot and row generator of a seed walk (SeedRows), wave-uniform rounds in
 * which every lane issues the window loads of the candidate it holds
 * (BandWindow: the text at [o - w, o + m + w) clipped to the text) together
 * with the sa load of its next row and waits once.  The host side of a call is
 * seed_score_call.
 *
 * What is this file's is the score and the record.  The score is the
 * bit-parallel banded dynamic programme of kfmi_align_dp.h: m rows per
 * candidate in every lane, whatever the text holds, so only the candidate
 * counts diverge, as in the verify.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kfmi_text.h"
#include "kfmi_align_dp.h"

namespace kfmi {

template <int MAXW, bool STR>
__global__ __launch_bounds__(256) void align_kernel(VerifyArgs a, uint32_t band)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  uint64_t t;
  if (!text_task<MAXW, STR>(a.ascii, a.num, a.m, a.strands, stage, cw, t)) return;
  const uint32_t m = a.m, n = a.n, w = band;
  const uint2* __restrict__ ivt = a.iv + t * a.S;
  const uint2* __restrict__ spt = a.sp + t * a.S;
  const int grp = lane_group();
  SeedRows k;
  uint32_t E = 0xFFFFFFFFu, bmin = 0xFFFFFFFFu, bmax = 0u, scored = 0u;
  for (;;) {
    k.refill(a, ivt, spt);
    const bool more = k.more();
    if (!__ballot(more || k.have)) break;
    uint32_t o;
    const bool sc = k.candidate(a, m, n, o);
    BandWindow<MAXW> win(sc, sc ? n - o - m : 0u, m, w, n);   /* the read's last base: base n - o - m of the stream */
    uint32_t np = SKIP_NONE;
    under_group_mask(a.split4, grp, [&] {
      win.load(a.text);
      if (more) np = a.jsa[k.r];
    });
    if (sc) {
      uint32_t vp, vn, s0;
      band_rows<MAXW>(cw, win.tx, m, w, win.sh, win.low, vp, vn, s0);
      band_fold(vp, vn, s0, w, o, n, E, bmin, bmax);
      ++scored;
    }
    k.advance(np);
  }
  const bool hit = scored != 0u && E <= a.bound;
  a.hits[t] = hit ? make_uint2(bmin, E | (bmax - bmin > 2u * w ? KFMI_HIT_MULTI : 0u) | (scored << KFMI_HIT_SCORED_SHIFT))
                  : make_uint2(KFMI_HIT_NONE, scored << KFMI_HIT_SCORED_SHIFT);
}

static hipError_t launch_align(const VerifyArgs& a, uint32_t band, hipStream_t st)
{
  const uint64_t tasks = (a.strands == KFMI_STRAND_BOTH ? 2u : 1u) * a.num;
  return launch_text(a.m, a.strands, tasks, st, [&](auto W, auto S, dim3 grid, size_t lds) {
    hipLaunchKernelGGL((align_kernel<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, st, a, band);
  });
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
