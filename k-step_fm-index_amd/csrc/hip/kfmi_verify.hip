/*
 * kfmi_verify.hip -- seed verification: the best Hamming placement of every
 * task among the text positions its seeds imply (kstep_fmi.h section 2,
 * "verify seeds"; not in the reference, which stops at
 * intervals).
 *
 * Input: the reads on the device, the two handles a seed search leaves there
 * (slot t * S + s: {L, R} in `intervals`, {start, len} in `spans`) and the flat
 * tables [sa | isa | text] of the text jump (kfmi_jump.hip).  The FM index is
 * never touched, so the kernel knows no geometry: it is templated on the code
 * words per read (8 | 16) and on the staging (forward reads, or the strand
 * staging for REV and BOTH) alone.
 *
 * The frame is kfmi_text.h's: one lane per task, the read in registers, the
 * slot and row generator of a seed walk.  Each row r is a candidate p = sa[r],
 * origin o = p - start.  The read's code words and the text's word
 * stream share their bit order (the base at reversed index r at bits 2r), so the
 * window of origin o starts at bit 2 * (n - o - m) of the stream, takes
 * ceil(m / 16) + 1 dwords, and the Hamming distance is an XOR, a mask on the
 * last word and popc((x | x >> 1) & 0x55555555).
 *
 * A round is wave-uniform.  Every lane issues the window loads of the candidate
 * it holds together with the sa load of its next row, then everything waits
 * once: a candidate costs about one round trip.  Every address is in range
 * before its load: rows below `rows`, window words clamped to the stream's last
 * word -- a window with no word in front, clamped and not zero-filled, so it is
 * this file's and not kfmi_text.h's BandWindow.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kfmi_text.h"

namespace kfmi {

template <int MAXW, bool STR>
__global__ __launch_bounds__(256) void verify_kernel(VerifyArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  uint64_t t;
  if (!text_task<MAXW, STR>(a.ascii, a.num, a.m, a.strands, stage, cw, t)) return;
  const uint32_t m = a.m, n = a.n, nw = (m + 15u) >> 4;
  const uint32_t wlast = (uint32_t) jump_text_words(n) - 1u;   /* the stream's last word */
  const uint2* __restrict__ ivt = a.iv + t * a.S;
  const uint2* __restrict__ spt = a.sp + t * a.S;
  const int grp = lane_group();
  SeedRows k;
  uint32_t best_m = 0xFFFFFFFFu, best_o = 0xFFFFFFFFu, multi = 0u, scored = 0u;
  for (;;) {
    k.refill(a, ivt, spt);
    const bool more = k.more();
    if (!__ballot(more || k.have)) break;
    uint32_t o;
    const bool sc = k.candidate(a, m, n, o);
    const uint32_t off = sc ? n - o - m : 0u;   /* the window starts at bit 2 * off of the stream */
    /* sc: n >= m, so wlast >= nw; a scored window ends inside the stream, the clamp never moves it */
    const uint32_t w0 = sc ? ((off >> 4) + nw <= wlast ? off >> 4 : wlast - nw) : 0u;
    const uint32_t sh = (off & 15u) * 2u;
    const uint32_t lim = sc ? nw + 1u : 0u;
    const uint32_t* tp = a.text + w0;
    uint32_t tx[MAXW + 1];
#pragma unroll
    for (int j = 0; j <= MAXW; ++j) tx[j] = 0u;
    uint32_t np = SKIP_NONE;
    under_group_mask(a.split4, grp, [&] {
#pragma unroll
      for (int j = 0; j <= MAXW; ++j)
        if ((uint32_t) j < lim) tx[j] = tp[j];
      if (more) np = a.jsa[k.r];
    });
    if (sc) {
      uint32_t mm = 0u;
#pragma unroll
      for (int j = 0; j < MAXW; ++j)
        if ((uint32_t) j < nw) {
          const uint32_t left = 2u * m - 32u * (uint32_t) j;   /* bits of the read from this word on */
          const uint32_t x = (cw[j] ^ __builtin_amdgcn_alignbit(tx[j + 1], tx[j], sh)) &
                             (left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u);
          mm += (uint32_t) __popc((x | (x >> 1)) & 0x55555555u);
        }
      ++scored;
      if (mm < best_m) {
        best_m = mm;
        best_o = o;
        multi = 0u;
      } else if (mm == best_m && o != best_o) {   /* another origin with the same count */
        multi = KFMI_HIT_MULTI;
        best_o = o < best_o ? o : best_o;
      }
    }
    k.advance(np);
  }
  const bool hit = scored != 0u && best_m <= a.bound;
  a.hits[t] = hit ? make_uint2(best_o, best_m | multi | (scored << KFMI_HIT_SCORED_SHIFT))
                  : make_uint2(KFMI_HIT_NONE, scored << KFMI_HIT_SCORED_SHIFT);
}

static hipError_t launch_verify(const VerifyArgs& a, uint32_t band, hipStream_t st)
{
  const uint64_t tasks = (a.strands == KFMI_STRAND_BOTH ? 2u : 1u) * a.num;
  return launch_text(a.m, a.strands, tasks, st, [&](auto W, auto S, dim3 grid, size_t lds) {
    hipLaunchKernelGGL((verify_kernel<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, st, a);
  });
}

/* The host array of a transferred results handle copied to its device array:
 * caller-filled slots for kfmi_verify_seeds (transferCPUtoGPU zeroes the device
 * array it allocates and copies nothing up). */
extern "C" int32_t kfmi_results_to_device(void* results)
{
  kfmi_res_t* r = (kfmi_res_t*) results;
  if (!r) return KFMI_E_BAD_ARGUMENT;
  if (r->grp) return KFMI_E_NOT_IMPLEMENTED;
  if (!r->d_results) return KFMI_E_NOT_ON_DEVICE;
  DeviceGuard dg;
  DevCtx* ctx = nullptr;
  const int32_t err = ctx_for(r->d_device, &ctx);
  if (err) return err;
  HIP_OK(hipMemcpyAsync(r->d_results, r->h_results, 8ull * r->num, hipMemcpyHostToDevice, ctx->st));
  HIP_OK(hipStreamSynchronize(ctx->st));
  return KFMI_SUCCESS;
}

int32_t RecordCall::open(kfmi_fmi_t* f, std::initializer_list<const kfmi_res_t*> rs)
{
  lk = std::shared_lock<RwLock>(index_lock(f));
  /* resident_single's refusals in its order, without reads */
  if (f->grp) return KFMI_E_NOT_IMPLEMENTED;
  for (const kfmi_res_t* r : rs)
    if (r->grp) return KFMI_E_NOT_IMPLEMENTED;
  if (!f->dev) return KFMI_E_NOT_ON_DEVICE;
  for (const kfmi_res_t* r : rs)
    if (!r->d_results) return KFMI_E_NOT_ON_DEVICE;
  if (!lane_kernels(f->dev)) return KFMI_E_NOT_IMPLEMENTED;
  di = f->dev;
  for (const kfmi_res_t* r : rs)
    if (r->d_device != di->device) return KFMI_E_BAD_ARGUMENT;
  return search_lane(di->device, &l);
}

int32_t TextCall::open(kfmi_fmi_t* f, kfmi_qrys_t* q, std::initializer_list<const kfmi_res_t*> rs)
{
  lk = std::shared_lock<RwLock>(index_lock(f));
  /* the copies the seed search covers, which the text jump builds its tables for, and the ASCII rows */
  int32_t err = resident_single(f, q, rs, NEED_LANE_KERNELS | NEED_ASCII);
  if (err) return err;
  di = f->dev;
  dq = q->dev;
  if (dq->device != di->device || dq->num != q->num || dq->size != q->size) return KFMI_E_BAD_ARGUMENT;
  err = search_lane(di->device, &l);
  if (err) return err;
  /* the text jump's tables, built here where the copy has none -- the path
   * kfmi_set_jump(1) takes at a first search, whatever this thread's setting */
  IdxArgs ix = idx_args(di);
  err = use_jump(di, l.st, ix, 1u);
  if (err) return err;
  if (!ix.jsa) return KFMI_E_NOT_IMPLEMENTED;   /* the index failed the tables' exactness check */
  jsa = ix.jsa;
  split4 = split_for(8ull * di->bwtsize, LAY_INTER) == 4u ? 1u : 0u;
  return KFMI_SUCCESS;
}

int32_t RecordCall::begin()
{
  HIP_OK(hipEventRecord(l.ev[0], l.st));
  HIP_OK(hipEventRecord(l.ev[1], l.st));
  return KFMI_SUCCESS;
}

int32_t RecordCall::finish()
{
  HIP_OK(hipEventRecord(l.ev[2], l.st));
  const int32_t err = search_finish(l.st, l.ev, t_ms);
  t_ms[0] = t_ms[2];   /* total, 0, the kernel: nothing is packed beforehand */
  t_ms[1] = 0.0;
  return err;
}

int32_t seed_score_call(void* index, void* queries, void* intervals, void* spans, void* hits, uint32_t max_seeds,
                        uint32_t strands, uint32_t max_occ, uint32_t band, uint32_t bound, SeedScoreLaunch launch)
{
  if (max_seeds < 1 || max_seeds > 8) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (max_occ < 1 || max_occ > KFMI_VERIFY_MAX_OCC) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* ri = (kfmi_res_t*) intervals;
  kfmi_res_t* rs = (kfmi_res_t*) spans;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  if (!f || !q || !ri || !rs || !rh || ri == rs || rh == ri || rh == rs) return KFMI_E_BAD_ARGUMENT;
  const uint64_t tasks = (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num;
  if (ri->num != max_seeds * tasks || rs->num != max_seeds * tasks || rh->num != tasks) return KFMI_E_BAD_ARGUMENT;
  if (q->size < 1 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  TextCall c;
  int32_t err = c.open(f, q, {ri, rs, rh});
  if (err) return err;
  VerifyArgs a{c.args(strands)};
  a.iv = reinterpret_cast<const uint2*>(ri->d_results);
  a.sp = reinterpret_cast<const uint2*>(rs->d_results);
  a.hits = reinterpret_cast<uint2*>(rh->d_results);
  a.jsa = c.jsa;
  a.S = max_seeds;
  a.rows = c.di->bwtsize;
  a.max_occ = max_occ;
  a.bound = bound;
  err = c.begin();
  if (err) return err;
  if (c.dq->num) HIP_OK(launch(a, band, c.l.st));
  return c.finish();
}

extern "C" int32_t kfmi_verify_seeds(void* index, void* queries, void* intervals, void* spans, void* hits,
                                     uint32_t max_seeds, uint32_t strands, uint32_t max_occ, uint32_t max_mism)
{
  return seed_score_call(index, queries, intervals, spans, hits, max_seeds, strands, max_occ, 0u, max_mism,
                         launch_verify);
}

}  // namespace kfmi
