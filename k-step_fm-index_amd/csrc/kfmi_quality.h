/*
 * kfmi_quality.h -- the per-task arithmetic of kfmi_map_quality (kstep_fmi.h,
 * "second placement / mapping quality"): the gap between a task's placement
 * and the next-best one, and the quality that gap gives.  Plain C on u32 record
 * words, so the host form (csrc/host/second.c) and the kernel
 * (csrc/hip/kfmi_second.hip) compile the same text; tests/second_ref.py states
 * it again in numpy.
 */
#ifndef KFMI_QUALITY_H_
#define KFMI_QUALITY_H_

#include <stdint.h>

#include "kfmi_internal.h"   /* KFMI_HIT_*, KFMI_SECOND_TRUNCATED, KFMI_MAPQ_* */

#if defined(__HIPCC__)
#define KFMI_QUAL_FN __host__ __device__ __forceinline__
#else
#define KFMI_QUAL_FN static inline
#endif

/* What kfmi_map_quality requires of its arguments; entries is the handles' size. */
static inline int32_t kfmi_quality_args(uint64_t entries, uint32_t strands)
{
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (strands == KFMI_STRAND_BOTH && (entries & 1u)) return KFMI_E_BAD_ARGUMENT;   /* two tasks per read */
  return KFMI_SUCCESS;
}

/* The record of task t: own = hits[t], sec = second[t]; both: BOTH mode, where mate = hits[t ^ 1] and msec =
 * second[t ^ 1] are the read's other strand (not read otherwise) and rev says that t is the REV task. */
KFMI_QUAL_FN void kfmi_quality(const uint32_t* own, const uint32_t* sec, const uint32_t* mate, const uint32_t* msec,
                               int both, int rev, uint32_t max_second, uint32_t* out)
{
  const uint64_t E = own[1] & KFMI_HIT_MISM_MASK;
  uint64_t C = (uint64_t) max_second + 1u, gap;
  uint32_t q, trunc = sec[1] & KFMI_SECOND_TRUNCATED;
  out[0] = 0u;
  out[1] = 0u;
  if (own[0] == KFMI_HIT_NONE) return;
  if (sec[0] != KFMI_HIT_NONE && (sec[1] & KFMI_HIT_MISM_MASK) < C) C = sec[1] & KFMI_HIT_MISM_MASK;
  if (both) {
    const uint64_t Em = mate[1] & KFMI_HIT_MISM_MASK;
    trunc |= msec[1] & KFMI_SECOND_TRUNCATED;
    if (mate[0] != KFMI_HIT_NONE) {
      if (Em < C) C = Em;
      if (Em == E && rev) C = E;   /* equal edits on both strands: gap 0 on either, said outright for the REV task */
    }
  }
  gap = C > E ? C - E : 0u;
  if (gap > 0xFFFFFFFFull) gap = 0xFFFFFFFFull;   /* max_second = 2^32 - 1 and E = 0: the word saturates */
  q = gap >= KFMI_MAPQ_MAX / KFMI_MAPQ_PER_EDIT ? KFMI_MAPQ_MAX : KFMI_MAPQ_PER_EDIT * (uint32_t) gap;
  if (trunc && q > KFMI_MAPQ_TRUNCATED) q = KFMI_MAPQ_TRUNCATED;
  out[0] = q;
  out[1] = (uint32_t) gap;
}

#endif
