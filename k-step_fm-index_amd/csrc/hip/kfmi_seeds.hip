/*
 * kfmi_seeds.hip -- seed search: the greedy right-to-left factorisation of
 * every read into maximal exact segments (kstep_fmi.h section 2, DESIGN.md 5g;
 * not in the reference, which returns the interval of the whole read).
 *
 * A search of ns strands with S = max_seeds runs ns * num tasks and fills S
 * slots per task in two results handles: slot t * S + s of `intervals` holds
 * [L, R) of record s of task t, the same slot of `spans` its {start, len}.
 * The walk is seed_walk (kfmi_kernels.h) behind one of three stagings -- the
 * fused forward packer, the fused strand packer, or code words in memory --
 * and which one is the launch plan's answer (kfmi_plan.h), queued by
 * search_enqueue like every other search.  Plain-counter task backends at K = 1, 2, reads of up to 256 bases,
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

KFMI_FOR_LANE_GEOMETRIES(KFMI_SEEDS_EXTERN)
/* seeds_trace_one<K, NB, LAY> is compiled in kfmi_inst_trace_seeds_*.hip */
KFMI_FOR_LANE_GEOMETRIES(KFMI_SEEDS_TRACE_EXTERN)

/* a.trace set: the traced kernels (kfmi_search_seeds_trace) */
hipError_t dispatch_seeds(uint32_t K, uint32_t nb, int lay, const SearchLaunch& a)
{
#define KFMI_CASE(KK, NBV, LAYV)                \
  if (K == KK && nb == NBV && lay == LAYV)      \
    return a.trace ? seeds_trace_one<KK, NBV, LAYV>(a) : seeds_one<KK, NBV, LAYV>(a);
  KFMI_FOR_LANE_GEOMETRIES(KFMI_CASE)
#undef KFMI_CASE
  return hipErrorInvalidValue;
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
  const int32_t err = resident_single(f, q, {ri, rs}, NEED_LANE_KERNELS);
  if (err) return err;
  /* a seed search never takes the text jump */
  return search_run(f, q, ri->d_results, tables_wanted().no_jump(), SearchWhat{strands, rs->d_results, max_seeds}, trace,
                    (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num);
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
