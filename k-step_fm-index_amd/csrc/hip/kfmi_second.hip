/*
 * kfmi_second.hip -- second placement and mapping quality: for every task the
 * best banded placement outside the neighbourhood of the begin position that
 * kfmi_align_seeds reported, and the quality the gap between the two gives
 * (kstep_fmi.h section 2, "second placement / mapping quality"; DESIGN.md 5n;
 * not in the reference, which stops at intervals).
 *
 * second_kernel is align_kernel (kfmi_align.hip) over the same candidates, on
 * kfmi_text.h's frame: one lane per task, the read in registers, SeedRows,
 * wave-uniform rounds with one wait.  Three things differ.  X, word x of the
 * task's hit, is loaded once per lane.  The per-lane predicate is far = sc &&
 * |o - X| > w, which takes the place of sc for the window and for the dynamic
 * programme: a candidate whose whole band lies within 2w of X can own no far
 * cell, so it issues no text loads and runs no rows -- for a uniquely mapping
 * read that is every candidate, and a round costs the sa load of the next row
 * alone.  And the fold over row 0 (band_fold_far, kfmi_align_dp.h) leaves out
 * the cells with |b - X| <= 2w.  TRUNC comes from a short prologue over the
 * task's S slots.  A task with X = KFMI_HIT_NONE takes no slot at all.
 *
 * quality_kernel is a streaming kernel over the records, one lane per task, on
 * the arithmetic of kfmi_quality.h.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kfmi_quality.h"
#include "kfmi_text.h"
#include "kfmi_align_dp.h"

namespace kfmi {

/* a.hits: the `second` records written; first: the hits read; a.bound: max_second */
template <int MAXW, bool STR>
__global__ __launch_bounds__(256) void second_kernel(VerifyArgs a, const uint2* __restrict__ first, uint32_t band)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  uint64_t t;
  if (!text_task<MAXW, STR>(a.ascii, a.num, a.m, a.strands, stage, cw, t)) return;
  const uint32_t m = a.m, n = a.n, w = band;
  const uint2* __restrict__ ivt = a.iv + t * a.S;
  const uint2* __restrict__ spt = a.sp + t * a.S;
  const int grp = lane_group();
  const uint32_t X = first[t].x;
  const bool placed = X != KFMI_HIT_NONE;
  /* TRUNC: a slot that is not ignored holds more rows than max_occ looks at (refill's tests, once more) */
  uint32_t trunc = 0u;
  for (uint32_t s = 0; s < a.S; ++s) {
    const uint2 lr = ivt[s], sl = spt[s];
    if (lr.y > lr.x && lr.x < a.rows && sl.y != 0u && (uint64_t) sl.x + sl.y <= a.m &&
        (lr.y < a.rows ? lr.y : a.rows) - lr.x > a.max_occ)
      trunc = KFMI_SECOND_TRUNCATED;
  }
  SeedRows k;
  if (!placed) k.s = a.S;   /* no slot is taken: the lane only keeps the wave's rounds company */
  uint32_t E = 0xFFFFFFFFu, bmin = 0xFFFFFFFFu, bmax = 0u, counted = 0u;
  for (;;) {
    k.refill(a, ivt, spt);
    const bool more = k.more();
    if (!__ballot(more || k.have)) break;
    uint32_t o;
    const bool sc = k.candidate(a, m, n, o);
    const int64_t dx = (int64_t) o - (int64_t) X;
    const bool far = sc && (dx > (int64_t) w || dx < -(int64_t) w);   /* the candidates that can own a far cell */
    BandWindow<MAXW> win(far, far ? n - o - m : 0u, m, w, n);
    uint32_t np = SKIP_NONE;
    under_group_mask(a.split4, grp, [&] {
      win.load(a.text);
      if (more) np = a.jsa[k.r];
    });
    if (far) {
      uint32_t vp, vn, s0;
      band_rows<MAXW>(cw, win.tx, m, w, win.sh, win.low, vp, vn, s0);
      band_fold_far(vp, vn, s0, w, o, n, X, E, bmin, bmax);
      ++counted;
    }
    k.advance(np);
  }
  const uint32_t tail = trunc | (counted << KFMI_HIT_SCORED_SHIFT);
  const bool got = E != 0xFFFFFFFFu && E <= a.bound;   /* E is set iff a far pair exists */
  a.hits[t] = !placed ? make_uint2(KFMI_HIT_NONE, 0u)
              : got   ? make_uint2(bmin, E | (bmax - bmin > 2u * w ? KFMI_HIT_MULTI : 0u) | tail)
                      : make_uint2(KFMI_HIT_NONE, tail);
}

static hipError_t launch_second(const VerifyArgs& a, const uint2* first, uint32_t band, hipStream_t st)
{
  const uint64_t tasks = (a.strands == KFMI_STRAND_BOTH ? 2u : 1u) * a.num;
  return launch_text(a.m, a.strands, tasks, st, [&](auto W, auto S, dim3 grid, size_t lds) {
    hipLaunchKernelGGL((second_kernel<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, st, a, first,
                       band);
  });
}

/* seed_score_call's checks in its order, with the two record handles in place of its one */
extern "C" int32_t kfmi_align_second(void* index, void* queries, void* intervals, void* spans, void* hits, void* second,
                                     uint32_t max_seeds, uint32_t strands, uint32_t max_occ, uint32_t band,
                                     uint32_t max_second)
{
  if (band > KFMI_ALIGN_MAX_BAND) return KFMI_E_BAD_ARGUMENT;
  if (max_seeds < 1 || max_seeds > 8) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (max_occ < 1 || max_occ > KFMI_VERIFY_MAX_OCC) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* ri = (kfmi_res_t*) intervals;
  kfmi_res_t* rs = (kfmi_res_t*) spans;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  kfmi_res_t* r2 = (kfmi_res_t*) second;
  if (!f || !q || !ri || !rs || !rh || !r2 || ri == rs || rh == ri || rh == rs || r2 == ri || r2 == rs || r2 == rh)
    return KFMI_E_BAD_ARGUMENT;
  const uint64_t tasks = (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num;
  if (ri->num != max_seeds * tasks || rs->num != max_seeds * tasks || rh->num != tasks || r2->num != tasks)
    return KFMI_E_BAD_ARGUMENT;
  if (q->size < 1 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  TextCall c;
  int32_t err = c.open(f, q, {ri, rs, rh, r2});
  if (err) return err;
  VerifyArgs a{c.args(strands)};
  a.iv = reinterpret_cast<const uint2*>(ri->d_results);
  a.sp = reinterpret_cast<const uint2*>(rs->d_results);
  a.hits = reinterpret_cast<uint2*>(r2->d_results);
  a.jsa = c.jsa;
  a.S = max_seeds;
  a.rows = c.di->bwtsize;
  a.max_occ = max_occ;
  a.bound = max_second;
  err = c.begin();
  if (err) return err;
  if (c.dq->num) HIP_OK(launch_second(a, reinterpret_cast<const uint2*>(rh->d_results), band, c.l.st));
  return c.finish();
}

__global__ __launch_bounds__(256) void quality_kernel(const uint2* __restrict__ hits, const uint2* __restrict__ second,
                                                       uint2* __restrict__ quals, uint64_t tasks, uint32_t both,
                                                       uint32_t max_second)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= tasks) return;   /* both: tasks is even, t ^ 1 is a task too */
  const uint64_t u = both ? t ^ 1u : t;
  const uint2 h = hits[t], s = second[t], hm = hits[u], sm = second[u];
  const uint32_t own[2] = {h.x, h.y}, sec[2] = {s.x, s.y}, mate[2] = {hm.x, hm.y}, msec[2] = {sm.x, sm.y};
  uint32_t out[2];
  kfmi_quality(own, sec, mate, msec, (int) both, (int) (both && (t & 1u)), max_second, out);
  quals[t] = make_uint2(out[0], out[1]);
}

extern "C" int32_t kfmi_map_quality(void* index, void* hits, void* second, void* quals, uint32_t strands,
                                    uint32_t max_second)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  kfmi_res_t* r2 = (kfmi_res_t*) second;
  kfmi_res_t* rq = (kfmi_res_t*) quals;
  if (!f || !rh || !r2 || !rq || rq == rh || rq == r2 || rh == r2 || rh->num != r2->num || rh->num != rq->num)
    return KFMI_E_BAD_ARGUMENT;
  int32_t err = kfmi_quality_args(rh->num, strands);
  if (err) return err;
  RecordCall c;
  err = c.open(f, {rh, r2, rq});
  if (err) return err;
  err = c.begin();
  if (err) return err;
  if (rh->num) {
    hipLaunchKernelGGL(quality_kernel, dim3((uint32_t) ((rh->num + 255) / 256)), dim3(256), 0, c.l.st,
                       reinterpret_cast<const uint2*>(rh->d_results), reinterpret_cast<const uint2*>(r2->d_results),
                       reinterpret_cast<uint2*>(rq->d_results), rh->num, strands == KFMI_STRAND_BOTH ? 1u : 0u,
                       max_second);
    HIP_OK(hipGetLastError());
  }
  return c.finish();
}

}  // namespace kfmi
