/*
 * kfmi_plan.h -- the launch plan: where a search's code words come from, as a
 * pure function of values (no handle, no device).  Every search form asks here
 * -- search_enqueue for the forward, strand and seed searches and their traced
 * twins, a chunk of stream_on, count_on -- and plan_launch (kfmi_runtime.h) turns the answer into the
 * SearchLaunch; the kernel's fetch form is fetch_form<G> (kfmi_kernels.h).
 * DESIGN.md "launch plan" has the rules as a table; kfmi_launch_plan
 * (kstep_fmi.h) shows both to a CPU test.
 */
#ifndef KFMI_PLAN_H_
#define KFMI_PLAN_H_

#include <stdint.h>

#include "../kfmi_internal.h"
#include "kfmi_device.h"

namespace kfmi {

struct PlanIn {
  bool coop = false;       /* a cooperative backend */
  int layout = LAY_INTER;
  uint32_t K = 1;
  bool seeds = false;      /* a seed search of `strands`, else the search of `strands` */
  uint32_t strands = KFMI_STRAND_FWD;
  bool ascii = false;      /* the ASCII rows of this batch or chunk are on the device (not host-packed) */
  uint32_t steps = 0, nwords = 0, rem = 0;   /* query_geometry: m = rem + K * steps, in nwords code words */
  bool fused = true;       /* the fused knob (KFMI_FUSED, kfmi_set_fused) */
  bool skip = false;       /* the skip table is in effect (ix.skip != nullptr) */
  bool traced = false;     /* the traced twin: refused where no traced kernel exists */
};

enum PlanPack : int { PACK_NONE = 0, PACK_FORWARD = 1, PACK_STRANDS_ASCII = 2, PACK_STRANDS_WORDS = 3 };

struct LaunchPlan {
  int32_t refusal = KFMI_SUCCESS;
  int maxw = 0;                /* SearchLaunch::maxw: 8 / 16 = the kernel packs the ASCII rows itself */
  int words_maxw = 0;          /* SearchLaunch::words_maxw */
  uint32_t strands = 0;        /* SearchLaunch::strands, as the kernel receives it */
  bool strand_words = false;   /* qp: dq->strand_words, else dq->packed */
  uint32_t columns = 1;        /* task columns per read: SearchLaunch::num = columns * reads */
  int pack = PACK_NONE;        /* the launch between ev[0] and ev[1] */
  bool reserve = false;        /* strand_reserve before anything is queued */
};

/* Code registers the kernel needs to pack a query itself: 16 bases per word, 8
 * words up to 128 K-step bases, 16 up to 256; 0 = the pack launch (longer reads,
 * or the knob is off).  Task and coop kernels alike. */
inline int fused_maxw(bool fused, uint32_t bases) { return !fused ? 0 : (bases <= 128 ? 8 : (bases <= 256 ? 16 : 0)); }

/* Code registers per task for the walks that keep packed words in registers
 * (task_words_skip_kernel, seed_words_kernel): 8 or 16, 0 = longer reads. */
inline int strand_words_maxw(uint32_t nwords) { return nwords <= 8 ? 8 : (nwords <= 16 ? 16 : 0); }

inline LaunchPlan launch_plan(const PlanIn& in)
{
  LaunchPlan p;
  const bool fwd = in.strands == KFMI_STRAND_FWD;
  if (!fwd && !in.seeds && !in.ascii && in.K == 3) {   /* no 15-base words from the host packer */
    p.refusal = KFMI_E_BAD_ARGUMENT;
    return p;
  }
  /* the fused strand kernels: task backends at K <= 2, whole K-steps, not the grouped layout */
  const bool in_kernel = in.ascii && (fwd || !(in.rem || in.K > 2 || in.coop || in.layout == LAY_GRP));
  p.maxw = in_kernel ? fused_maxw(in.fused, in.K * in.steps) : 0;
  /* a forward search of packed words takes the plain walk, even with the skip table in effect */
  if (!p.maxw && (in.seeds || !fwd)) p.words_maxw = strand_words_maxw(in.nwords);
  if (in.seeds && !p.maxw && !p.words_maxw) p.refusal = KFMI_E_BAD_ARGUMENT;
  else if (in.traced && !in.seeds && (fwd ? !p.maxw || in.coop : !p.maxw && !(in.skip && p.words_maxw)))
    p.refusal = KFMI_E_NOT_IMPLEMENTED;   /* the plain walk of words and the cooperative kernels have no traced form */
  if (p.refusal) return p;
  p.strands = p.maxw && !fwd ? in.strands : 0u;
  p.strand_words = !fwd;
  p.columns = !p.maxw && in.strands == KFMI_STRAND_BOTH ? 2u : 1u;
  if (!p.maxw) p.pack = fwd ? (in.ascii ? PACK_FORWARD : PACK_NONE) : (in.ascii ? PACK_STRANDS_ASCII : PACK_STRANDS_WORDS);
  p.reserve = !p.maxw && !fwd;
  return p;
}

}  // namespace kfmi

#endif  // KFMI_PLAN_H_
