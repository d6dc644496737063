/*
 * kfmi_seeds.hip -- seed search: the greedy right-to-left factorisation of
 * every read into maximal exact segments (kstep_fmi.h section 2, DESIGN.md 5g;
 * not in the reference, which returns the interval of the whole read).
 *
 * A search of ns strands with S = max_seeds runs ns * num tasks and fills S
 * slots per task in two results handles: slot t * S + s of `intervals` holds
 * [L, R) of record s of task t, the same slot of `spans` its {start, len}.
 * The walk is seed_walk (kfmi_kernels.h) behind one of three stagings: the
 * fused forward packer, the fused strand packer (m % K == 0), or code words in
 * memory -- the forward pack launch, the strand pack launch or a host-packed
 * upload.  Plain-counter task backends at K = 1, 2, reads of up to 256 bases,
 * one device; everything else is refused before anything is queued.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <shared_mutex>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_runtime.h"

namespace kfmi {

KFMI_FOR_NB(KFMI_SEEDS_EXTERN, 1, LAY_INTER)
KFMI_FOR_NB(KFMI_SEEDS_EXTERN, 2, LAY_INTER)
KFMI_FOR_NB(KFMI_SEEDS_EXTERN, 1, LAY_MID)
KFMI_FOR_NB(KFMI_SEEDS_EXTERN, 2, LAY_MID)
/* seeds_trace_one<K, NB, LAY> is compiled in kfmi_inst_trace_seeds_*.hip */
KFMI_FOR_NB(KFMI_SEEDS_TRACE_EXTERN, 1, LAY_INTER)
KFMI_FOR_NB(KFMI_SEEDS_TRACE_EXTERN, 2, LAY_INTER)
KFMI_FOR_NB(KFMI_SEEDS_TRACE_EXTERN, 1, LAY_MID)
KFMI_FOR_NB(KFMI_SEEDS_TRACE_EXTERN, 2, LAY_MID)

/* a.trace set: the traced kernels (kfmi_search_seeds_trace) */
static hipError_t dispatch_seeds(uint32_t K, uint32_t nb, int lay, const SearchLaunch& a)
{
#define KFMI_CASE(KK, NBV, LAYV)                \
  if (K == KK && nb == NBV && lay == LAYV)      \
    return a.trace ? seeds_trace_one<KK, NBV, LAYV>(a) : seeds_one<KK, NBV, LAYV>(a);
  KFMI_FOR_NB(KFMI_CASE, 1, LAY_INTER)
  KFMI_FOR_NB(KFMI_CASE, 2, LAY_INTER)
  KFMI_FOR_NB(KFMI_CASE, 1, LAY_MID)
  KFMI_FOR_NB(KFMI_CASE, 2, LAY_MID)
#undef KFMI_CASE
  return hipErrorInvalidValue;
}

/* The device copies that have seed kernels: the per-lane kernels on the two
 * plain-counter layouts at K <= 2 (the backends "task" and "task-mid"). */
static bool seeds_supported(const kfmi_dev_index* di)
{
  return !is_coop(di->backend) && (di->layout == LAY_INTER || di->layout == LAY_MID) && di->K >= 1 && di->K <= 2;
}

/* Queues one seed search on st, bracketed by ev[0..2] like search_enqueue.
 * Forward tasks pack in the kernel where the forward search would (ASCII on
 * the device, fused packing on), else walk dq->packed -- written by the pack
 * launch here, or by the host on upload.  Reverse and both-strand tasks pack
 * in the kernel where a strand search would (strand_fused_maxw), else walk
 * the strand pack's task columns.  trace: null, or one record per task for the
 * traced kernels (kfmi_search_seeds_trace); nothing else differs. */
static int32_t seeds_enqueue(kfmi_dev_index* di, kfmi_dev_queries* dq, uint32_t* d_iv, uint32_t* d_sp, hipStream_t st,
                             hipEvent_t* ev, const TableWants& want, uint32_t max_seeds, uint32_t strands,
                             DevCtx* ctx, uint4* trace = nullptr)
{
  if (dq->device != di->device || dq->K != di->K) return KFMI_E_BAD_ARGUMENT;
  const bool fwd = strands == KFMI_STRAND_FWD;
  const uint64_t ns = strands == KFMI_STRAND_BOTH ? 2 : 1;
  SearchLaunch a{};
  a.st = st;
  a.ix = idx_args(di);
  int32_t err = use_tables(di, st, a.ix, want, dq->rem);
  if (err) return err;
  if (fwd) a.maxw = dq->ascii ? fused_maxw(di->backend, dq->K * dq->steps) : 0;
  else a.maxw = strand_fused_maxw(di, dq->ascii != nullptr, dq->K, dq->steps, dq->rem);
  if (!a.maxw) {
    a.words_maxw = strand_words_maxw(dq->nwords);
    if (!a.words_maxw) return KFMI_E_BAD_ARGUMENT;
    if (!fwd) {
      err = strand_reserve(dq, dq->num, ctx);
      if (err) return err;
    }
  }
  a.strands = a.maxw && !fwd ? strands : 0u;
  a.qp = fwd ? dq->packed : dq->strand_words;
  a.ascii = dq->ascii;
  a.m = dq->size;
  a.num = a.maxw ? dq->num : ns * dq->num;
  a.steps = dq->steps;
  a.nwords = dq->nwords;
  a.res = d_iv;
  a.spans = d_sp;
  a.max_seeds = max_seeds;
  a.trace = trace;
  HIP_OK(hipEventRecord(ev[0], st));
  if (!a.maxw) HIP_OK(fwd ? launch_pack(dq, st) : launch_strand_pack(dq, dq->strand_words, strands, false, st));
  HIP_OK(hipEventRecord(ev[1], st));
  if (dq->num) HIP_OK(dispatch_seeds(di->K, di->nb, di->layout, a));
  HIP_OK(hipEventRecord(ev[2], st));
  return KFMI_SUCCESS;
}

/* kfmi_search_seeds, and kfmi_search_seeds_trace when `trace` is given: the
 * same checks in the same order, the same enqueue; the traced call adds the
 * device records and their copy to the host. */
static int32_t search_seeds(void* index, void* queries, void* intervals, void* spans, uint32_t max_seeds,
                            uint32_t strands, uint32_t* trace)
{
  if (max_seeds < 1 || max_seeds > 8) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* ri = (kfmi_res_t*) intervals;
  kfmi_res_t* rs = (kfmi_res_t*) spans;
  if (!f || !q || !ri || !rs || ri == rs) return KFMI_E_BAD_ARGUMENT;
  const uint64_t slots = (uint64_t) max_seeds * (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num;
  if (ri->num != slots || rs->num != slots) return KFMI_E_BAD_ARGUMENT;
  if (q->size > 256) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  /* group_transfer cuts results by their own count, which is not the read slices' */
  if (f->grp || q->grp || ri->grp || rs->grp) return KFMI_E_NOT_IMPLEMENTED;
  if (!f->dev || !q->dev || !ri->d_results || !rs->d_results) return KFMI_E_NOT_ON_DEVICE;
  kfmi_dev_index* di = f->dev;
  if (!seeds_supported(di)) return KFMI_E_NOT_IMPLEMENTED;
  if (ri->d_device != di->device || rs->d_device != di->device) return KFMI_E_BAD_ARGUMENT;
  SearchLane l;
  int32_t err = search_lane(di->device, &l);
  if (err) return err;
  const uint64_t tasks = (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num;
  uint4* d_trace = nullptr;
  if (trace && hipMalloc((void**) &d_trace, 16ull * (tasks ? tasks : 1)) != hipSuccess) {
    (void) hipGetLastError();
    return KFMI_E_DEVICE_ALLOC;
  }
  /* a seed search never takes the text jump */
  err = seeds_enqueue(di, q->dev, ri->d_results, rs->d_results, l.st, l.ev, tables_wanted().no_jump(), max_seeds, strands,
                      l.ctx, d_trace);
  if (!err) err = search_finish(l.st, l.ev, t_ms);
  if (trace) {
    if (!err && tasks && hipMemcpy(trace, d_trace, 16ull * tasks, hipMemcpyDeviceToHost) != hipSuccess) err = KFMI_E_KERNEL;
    (void) hipFree(d_trace);
  }
  return err;
}

extern "C" int32_t kfmi_search_seeds(void* index, void* queries, void* intervals, void* spans, uint32_t max_seeds,
                                     uint32_t strands)
{
  return search_seeds(index, queries, intervals, spans, max_seeds, strands, nullptr);
}

/* kstep_fmi.h: kfmi_search_seeds with the traced kernels and one record per
 * task copied out. */
extern "C" int32_t kfmi_search_seeds_trace(void* index, void* queries, void* intervals, void* spans, uint32_t max_seeds,
                                           uint32_t strands, uint32_t* trace)
{
  if (!trace) return KFMI_E_BAD_ARGUMENT;
  return search_seeds(index, queries, intervals, spans, max_seeds, strands, trace);
}

}  // namespace kfmi
