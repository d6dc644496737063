/*
 * kfmi_verify.h -- what kfmi_verify_seeds (kfmi_verify.hip) and
 * kfmi_align_seeds (kfmi_align.hip) share: the kernels' arguments and the host
 * side of a call -- argument checks, residency, the text jump's tables built on
 * demand, the launch between the lane's events and the timing.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace kfmi
