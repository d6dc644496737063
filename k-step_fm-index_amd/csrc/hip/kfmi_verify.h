/*
 * kfmi_verify.h -- what kfmi_verify_seeds (kfmi_verify.hip) and
 * kfmi_align_seeds (kfmi_align.hip) share: the kernels' arguments and the host
 * side of a call -- argument checks, residency, the text jump's tables built on
 * demand, the launch between the lane's events and the timing.  TextCall is
 * that host side without the seed handles; kfmi_align_paths (kfmi_paths.hip)
 * takes it too.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <shared_mutex>

#include "../kfmi_internal.h"
#include "kfmi_devguard.h"
#include "kfmi_runtime.h"

namespace kfmi {

struct VerifyArgs {
  const uint8_t* __restrict__ ascii;   /* num reads of m bases */
  const uint2* __restrict__ iv;        /* S slots per task: {L, R} */
  const uint2* __restrict__ sp;        /* S slots per task: {start, len} */
  uint2* __restrict__ hits;            /* one record per task */
  const uint32_t* __restrict__ jsa;    /* [sa | isa | text] */
  uint64_t num;
  uint32_t m, strands, S, rows, max_occ, max_mism, split4;   /* max_mism: the record's bound (align: max_edits) */
};

/* launches the kernel of one call on the lane's stream; band is 0 for the verify */
typedef hipError_t (*SeedScoreLaunch)(const VerifyArgs& a, uint32_t band, hipStream_t st);

/* One call of kfmi_verify_seeds / kfmi_align_seeds: every check, then `launch`. */
int32_t seed_score_call(void* index, void* queries, void* intervals, void* spans, void* hits, uint32_t max_seeds,
                        uint32_t strands, uint32_t max_occ, uint32_t band, uint32_t bound, SeedScoreLaunch launch);

/* What such a call does around its launches, for kfmi_align_paths
 * (kfmi_paths.hip) as well: a call checks its own arguments, then open() keeps
 * the caller's device and the index's lock for the object's life, requires the
 * single-device copies the seed search covers with the reads' ASCII rows, takes
 * the calling thread's lane and builds the text jump's tables where the copy
 * has none; begin() and finish() bracket the launches with the lane's events,
 * wait, and leave kfmi_last_timing at total, 0, the launches. */
struct TextCall {
  DeviceGuard dg;
  std::shared_lock<RwLock> lk;
  kfmi_dev_index* di = nullptr;
  kfmi_dev_queries* dq = nullptr;
  SearchLane l;
  const uint32_t* jsa = nullptr;   /* [sa | isa | text] */
  uint32_t split4 = 0;             /* the tables are past the translation reach: loads under the 16-lane group mask */
  int32_t open(kfmi_fmi_t* f, kfmi_qrys_t* q, std::initializer_list<const kfmi_res_t*> rs);
  int32_t begin();
  int32_t finish();
};

}  // namespace kfmi
