/*
 * kfmi_text.h -- the frame of the text kernels: verify_kernel
 * (kfmi_verify.hip), align_kernel (kfmi_align.hip), paths_kernel
 * (kfmi_paths.hip) and window_kernel (kfmi_window.hip) each run one lane per
 * task over the 2-bit text of the text jump's flat tables [sa | isa | text]
 * (kfmi_jump.hip), whose word stream holds text base n - 1 - g at bits 2g.
 * What they share is written here once:
 *
 *   on the device  text_task         the block's reads staged, the lane's code words and task
 *                  under_group_mask  a round's loads under the 16-lane group mask (verify, align, paths)
 *                  SeedRows          the slot and row generator of a seed walk (verify, align)
 *                  BandWindow        the text window of one band (align, paths)
 *   for a launch   TextArgs          the arguments every text kernel takes
 *                  launch_text       grid, staging LDS, the kernel of (code words, staging)
 *   for a call     RecordCall        lock, residency, lane, the launches between the lane's events
 *                  TextCall          ... with the reads and the text jump's tables built on demand
 *                  DeviceScratch, launch_result, seed_score_call
 *
 * The .hip files keep what is theirs: the score and the record (verify, align),
 * the kept rows and the walk (paths), the scan and the column step (window).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include <shared_mutex>
#include <type_traits>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_devguard.h"
#include "kfmi_runtime.h"

namespace kfmi {

/* What every text kernel takes.  The FM index is never touched, so the kernels know no geometry: they are templated
 * on the code words per read (8 | 16) and on the staging alone. */
struct TextArgs {
  const uint8_t* __restrict__ ascii;   /* num reads of m bases */
  const uint32_t* __restrict__ text;   /* the text's word stream, jsa + 2 * rows */
  uint64_t num;
  uint32_t m, strands, n, split4;      /* n = rows - 1 text bases; split4: loads under the 16-lane group mask */
};

struct VerifyArgs : TextArgs {
  const uint2* __restrict__ iv;        /* S slots per task: {L, R} */
  const uint2* __restrict__ sp;        /* S slots per task: {start, len} */
  uint2* __restrict__ hits;            /* one record per task */
  const uint32_t* __restrict__ jsa;    /* [sa | isa | text] */
  uint32_t S, rows, max_occ, bound;    /* bound: the record's (verify: max_mism, align: max_edits) */
};

/* The block's reads staged and packed by the search's own stagers with rem = 0 -- STR: the strand staging (strands
 * 2 = REV, 3 = BOTH: task 2q + strand), else forward reads -- into the lane's code words; t: the lane's task.
 * Returns whether the lane has one.  Every thread of the block must call it, before any exit. */
template <int MAXW, bool STR>
__device__ __forceinline__ bool text_task(const uint8_t* __restrict__ ascii, uint64_t num, uint32_t m, uint32_t strands,
                                          uint8_t* stage, uint32_t (&cw)[MAXW], uint64_t& t)
{
  if constexpr (STR) {
    stage_strand_codes<MAXW>(ascii, num, m, stage, cw, strands);
  } else {
    uint32_t rc = 0;
    stage_query_codes<MAXW>(ascii, num, m, stage, cw, 0u, rc);
  }
  t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  return t < (STR && strands == 3u ? 2u : 1u) * num;
}

/* the lane's 16-lane group of its wave */
__device__ __forceinline__ int lane_group() { return (int) (threadIdx.x & 63u) / 16; }

/* `f` -- a lane's loads of one round -- under each 16-lane group's mask in turn where the tables are past the
 * translation reach (split4, wave-uniform: split_for(8 * rows, LAY_INTER) == 4, as for the jump's gathers), and
 * plainly otherwise: one turn for every lane.  The turns are a loop that stays rolled, so that `f` has one body and
 * one set of destination registers and of load predicates: the loads of all four turns go out with no wait between
 * them, and the round waits once after the loop.  (Unrolled, the compiler zeroes the destinations again in every turn
 * and waits for the turn before -- four round trips; with a second, plain copy of `f` the predicates of both copies
 * cost align_kernel a wave per SIMD.) */
template <class F>
__device__ __forceinline__ void under_group_mask(uint32_t split4, int grp, F&& f)
{
  const int turns = split4 ? 4 : 1;
#pragma unroll 1
  for (int q = 0; q < turns; ++q)
    if (!split4 || grp == q) f();
}

/* The slot and row generator of a seed walk.  A lane walks its S slots: rows L, L + 1, .. below min(R, rows,
 * L + max_occ), each row r a candidate p = sa[r] of origin o = p - start.  A round is wave-uniform:
 *   for (;;) { k.refill(..); if (!__ballot(k.more() || k.have)) break; sc = k.candidate(..);
 *              [the window loads of the candidate in hand with np = jsa[k.r] where k.more(), one wait]
 *              [the score where sc] k.advance(np); } */
struct SeedRows {
  uint32_t s = 0, r = 0, rend = 0, start = 0;   /* the next slot, and the rows left of the current one */
  uint32_t p = 0, pstart = 0;                   /* the candidate in hand: its sa value and its slot's start */
  bool have = false;
  /* lanes out of rows take their next slot; an ignored slot leaves them out of rows */
  __device__ __forceinline__ void refill(const VerifyArgs& a, const uint2* __restrict__ ivt,
                                         const uint2* __restrict__ spt)
  {
    while (__ballot(r >= rend && s < a.S)) {
      if (r >= rend && s < a.S) {
        const uint2 lr = ivt[s], sl = spt[s];
        ++s;
        if (lr.y > lr.x && lr.x < a.rows && sl.y != 0u && (uint64_t) sl.x + sl.y <= a.m) {
          const uint64_t cap = (uint64_t) lr.x + a.max_occ;
          const uint32_t e = lr.y < a.rows ? lr.y : a.rows;
          r = lr.x;
          rend = cap < e ? (uint32_t) cap : e;
          start = sl.x;
        }
      }
    }
  }
  __device__ __forceinline__ bool more() const { return r < rend; }   /* r < rows: jsa[r] may be loaded */
  /* whether the candidate in hand places the read inside the text, and its origin */
  __device__ __forceinline__ bool candidate(const VerifyArgs& a, uint32_t m, uint32_t n, uint32_t& o) const
  {
    const bool sc = have && p < a.rows && p >= pstart && (uint64_t) (p - pstart) + m <= n;
    o = sc ? p - pstart : 0u;
    return sc;
  }
  __device__ __forceinline__ void advance(uint32_t np)
  {
    have = more();
    if (have) {
      p = np;
      pstart = start;
      ++r;
    }
  }
};

/* The window of one band: the text at [o - w, o + m + w) clipped to the text, which in the word stream is the bases
 * from off - w on with off = n - o - m (0 where !sc).  It is addressed through a stream with one word in front (base
 * off + 16 - w >= 1), so that the 15 cells that can lie past the text's end need no signed arithmetic: word 0 of that
 * stream and every word past the text's last are not loaded and read as zero, and the cells they would serve are
 * invalid (kfmi_align_dp.h).  A window takes ((sh + m - 1 + 2w) >> 4) + 1 <= ceil((m + 2w) / 16) + 1 words; tx, sh
 * and low are band_rows' arguments. */
template <int MAXW>
struct BandWindow {
  uint32_t w0, sh, lim, wtext, low;
  uint32_t tx[MAXW + 3];
  __device__ __forceinline__ BandWindow(bool sc, uint32_t off, uint32_t m, uint32_t w, uint32_t n)
  {
    const uint32_t g = off + 16u - w;                  /* the window's first base in the stream with a word in front */
    w0 = g >> 4;
    sh = g & 15u;
    lim = sc ? ((sh + m - 1u + 2u * w) >> 4) + 1u : 0u;   /* <= MAXW + 3 */
    wtext = sc ? (n - 1u) >> 4 : 0u;                   /* sc: n >= m >= 1; the last word that holds text */
    low = w > off ? w - off : 0u;
#pragma unroll
    for (int j = 0; j < MAXW + 3; ++j) tx[j] = 0u;
  }
  __device__ __forceinline__ void load(const uint32_t* __restrict__ text)
  {
#pragma unroll
    for (int j = 0; j < MAXW + 3; ++j) {
      const uint32_t x = w0 + (uint32_t) j;   /* word x - 1 of the text's stream */
      if ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) tx[j] = text[x - 1u];
    }
  }
};

/* One launch of a text kernel over `tasks` tasks of m bases: `pick(W, S, grid, lds)` starts the kernel of
 * W::value code words (8 up to 128 bases, else 16) and staging S::value on 256-thread blocks. */
template <class Pick>
hipError_t launch_text(uint32_t m, uint32_t strands, uint64_t tasks, hipStream_t st, Pick&& pick)
{
  const dim3 grid((uint32_t) ((tasks + 255) / 256));
  const size_t lds = 4 * (size_t) stage_slot_bytes(m);
  auto staged = [&](auto W) {
    if (strands != KFMI_STRAND_FWD) pick(W, std::true_type{}, grid, lds);
    else pick(W, std::false_type{}, grid, lds);
  };
  if (m <= 128) staged(std::integral_constant<int, 8>{});
  else staged(std::integral_constant<int, 16>{});
  return hipGetLastError();
}

/* The host side of a call on records alone (kfmi_mate_windows, kfmi_pair_hits): open() keeps the caller's device and
 * the index's lock for the object's life, requires every handle on the index's device -- the coverage is
 * kfmi_align_seeds' so that a chain of calls is refused as one -- and takes the calling thread's lane; begin() and
 * finish() bracket the launches with the lane's events, wait, and leave kfmi_last_timing at total, 0, the launches. */
struct RecordCall {
  DeviceGuard dg;
  std::shared_lock<RwLock> lk;
  kfmi_dev_index* di = nullptr;
  SearchLane l;
  int32_t open(kfmi_fmi_t* f, std::initializer_list<const kfmi_res_t*> rs);
  int32_t begin();
  int32_t finish();
};

/* ... and of a call of a text kernel: a call checks its own arguments, then open() requires the single-device copies
 * the seed search covers with the reads' ASCII rows as well and builds the text jump's tables where the copy has none;
 * args() is what the kernels take of them. */
struct TextCall : RecordCall {
  kfmi_dev_queries* dq = nullptr;
  const uint32_t* jsa = nullptr;   /* [sa | isa | text] */
  uint32_t split4 = 0;             /* the tables are past the translation reach */
  int32_t open(kfmi_fmi_t* f, kfmi_qrys_t* q, std::initializer_list<const kfmi_res_t*> rs);
  TextArgs args(uint32_t strands) const
  {
    return TextArgs{dq->ascii, jsa + 2ull * di->bwtsize, dq->num, dq->size, strands, di->bwtsize - 1u, split4};
  }
};

/* device memory for the life of a call: alloc() clears the HIP error it fails with */
struct DeviceScratch {
  uint32_t* p = nullptr;
  int32_t alloc(uint64_t bytes)
  {
    if (hipMalloc((void**) &p, bytes) == hipSuccess) return KFMI_SUCCESS;
    (void) hipGetLastError();
    p = nullptr;
    return KFMI_E_DEVICE_ALLOC;
  }
  ~DeviceScratch()
  {
    if (p) (void) hipFree(p);
  }
};

/* what a call returns after its launches: `err`, or KFMI_E_KERNEL with a line on stderr where a launch failed */
inline int32_t launch_result(int32_t err, hipError_t he, const char* kernel)
{
  if (he == hipSuccess) return err;
  fprintf(stderr, "kstepfmi: %s launch failed: %s\n", kernel, hipGetErrorString(he));
  return KFMI_E_KERNEL;
}

/* launches the kernel of one call on the lane's stream; band is 0 for the verify */
typedef hipError_t (*SeedScoreLaunch)(const VerifyArgs& a, uint32_t band, hipStream_t st);

/* One call of kfmi_verify_seeds / kfmi_align_seeds (kfmi_verify.hip): every check, then `launch`. */
int32_t seed_score_call(void* index, void* queries, void* intervals, void* spans, void* hits, uint32_t max_seeds,
                        uint32_t strands, uint32_t max_occ, uint32_t band, uint32_t bound, SeedScoreLaunch launch);

}  // namespace kfmi
