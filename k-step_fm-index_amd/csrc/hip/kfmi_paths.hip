/*
 * kfmi_paths.hip -- alignment paths: the CIGAR and the end position of every
 * task's placement at the begin position its hit holds (kstep_fmi.h section 2,
 * "align paths"; not in the reference, which stops at
 * intervals).
 *
 * The frame is align_kernel's (kfmi_align.hip): one lane per task, the read
 * packed into registers by the search's own stagers with rem = 0, the window
 * [c - w, c + m + w) of the band's centre c loaded as align_kernel loads the
 * window of an origin -- the stream with one word in front, lim, wtext, the
 * 16-lane group mask where the tables are past the translation reach.  A lane
 * has one candidate, so there is one load round and no sa load.
 *
 * The forward pass is band_rows' row step with each row kept
 * (kfmi_path_dp.h): three words per row -- vp, hp, eq -- go to a workspace in
 * global memory laid out [row][word][task of the launch], so a wave's row is
 * three contiguous 256-byte writes.  The walk reads the rows back from the last
 * one down, a wave in step (every transition but a skipped text base takes one
 * row), with the next row's loads in flight while a row is walked, and writes a
 * run into the task's words each time the operation changes.  A lane reads
 * only what it wrote itself, so no fence stands between the passes.
 *
 * The host side launches chunks of tasks so that the workspace keeps under a
 * cap: a chunk is a launch of its own on offset pointers, and the kernel knows
 * nothing of chunks.  Chunks are multiples of 64 tasks, which keeps the first
 * read of every staging round on a 16-byte boundary for every m.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_runtime.h"
#include "kfmi_verify.h"
#include "kfmi_path_dp.h"

namespace kfmi {

struct PathArgs {
  const uint8_t* __restrict__ ascii;   /* the launch's reads, num of m bases */
  const uint2* __restrict__ hits;      /* one record per task; x is read */
  uint2* __restrict__ paths;           /* one record per task */
  uint32_t* __restrict__ cigars;       /* 2C words per task */
  const uint32_t* __restrict__ text;   /* the text's word stream */
  uint32_t* rows;                      /* the kept rows: word p of row r of task t at (3 r + p) * stride + t */
  uint64_t num, stride;
  uint32_t m, strands, n, band, max_edits, C, split4;
};

/* a lane's column of the workspace: rows out in the forward pass ... */
struct KeepRows {
  uint32_t* at;   /* word 0 of row 0 of this lane */
  uint64_t stride;
  __device__ __forceinline__ void operator()(uint32_t r, uint32_t vp, uint32_t hp, uint32_t eq) const
  {
    uint32_t* p = at + 3ull * r * stride;
    p[0] = vp;
    p[stride] = hp;
    p[2 * stride] = eq;
  }
};

/* ... and back in the walk, one row ahead: row r is handed out from registers while row r - 1 is on its way */
struct ReadRows {
  const uint32_t* at;
  uint64_t stride;
  uint32_t vp, hp, eq;
  __device__ __forceinline__ void fetch(uint32_t r)
  {
    const uint32_t* p = at + 3ull * r * stride;
    vp = p[0];
    hp = p[stride];
    eq = p[2 * stride];
  }
  __device__ __forceinline__ void operator()(uint32_t r, uint32_t& vp_o, uint32_t& hp_o, uint32_t& eq_o)
  {
    vp_o = vp;
    hp_o = hp;
    eq_o = eq;
    if (r) fetch(r - 1u);
  }
};

/* the task's words: runs past the 2C-th are counted and not written */
struct RunWords {
  uint32_t* cig;
  uint32_t cap, runs;
  __device__ __forceinline__ void operator()(uint32_t op, uint32_t len)
  {
    if (runs < cap) cig[runs] = len << 4 | op;
    ++runs;
  }
};

/* STR: the strand staging (a.strands 2 = REV, 3 = BOTH: task 2q + strand), else forward reads. */
template <int MAXW, bool STR>
__global__ __launch_bounds__(256) void paths_kernel(PathArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  if constexpr (STR) {
    stage_strand_codes<MAXW>(a.ascii, a.num, a.m, stage, cw, a.strands);   /* whole block, before any exit */
  } else {
    uint32_t rc = 0;
    stage_query_codes<MAXW>(a.ascii, a.num, a.m, stage, cw, 0u, rc);       /* whole block, before any exit */
  }
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= (STR && a.strands == 3u ? 2u : 1u) * a.num) return;
  const uint32_t m = a.m, n = a.n, w = a.band, cap = 2u * a.C;
  const uint32_t* __restrict__ text = a.text;
  const int grp = (int) (threadIdx.x & 63u) / 16;
  const uint32_t B = a.hits[t].x;
  const bool in = B != KFMI_HIT_NONE && n >= m && B <= n;
  const uint32_t c = in ? (B < n - m ? B : n - m) : 0u;   /* the band's centre: c + m <= n */
  const bool sc = in && B - c <= w;
  const uint32_t off = sc ? n - c - m : 0u;          /* the read's last base is base `off` of the stream */
  const uint32_t g = off + 16u - w;                  /* the window's first base in the stream with a word in front */
  const uint32_t w0 = g >> 4, sh = g & 15u;
  const uint32_t lim = sc ? ((sh + m - 1u + 2u * w) >> 4) + 1u : 0u;   /* <= MAXW + 3 */
  const uint32_t wtext = sc ? (n - 1u) >> 4 : 0u;    /* sc: n >= m >= 1; the last word that holds text */
  uint32_t tx[MAXW + 3];
#pragma unroll
  for (int j = 0; j < MAXW + 3; ++j) tx[j] = 0u;
  if (a.split4) {   /* wave-uniform: all of a lane's loads under its group's mask */
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (grp == q) {
#pragma unroll
        for (int j = 0; j < MAXW + 3; ++j) {
          const uint32_t x = w0 + (uint32_t) j;   /* word x - 1 of the text's stream */
          if ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) tx[j] = text[x - 1u];
        }
      }
  } else {
#pragma unroll
    for (int j = 0; j < MAXW + 3; ++j) {
      const uint32_t x = w0 + (uint32_t) j;
      if ((uint32_t) j < lim && x >= 1u && x - 1u <= wtext) tx[j] = text[x - 1u];
    }
  }
  uint32_t* cig = a.cigars + t * cap;
  uint2 rec = make_uint2(KFMI_HIT_NONE, 0u);
  uint32_t used = 0u;
  if (sc) {
    KeepRows keep{a.rows + t, a.stride};
    uint32_t vp, vn, s0;
    band_rows_keep<MAXW>(cw, tx, m, w, sh, w > off ? w - off : 0u, keep, vp, vn, s0);
    const uint32_t k0 = w - (B - c);
    const uint32_t D = band_value(vp, vn, s0, k0);
    if (D <= a.max_edits) {
      ReadRows back{a.rows + t, a.stride, 0u, 0u, 0u};
      back.fetch(m - 1u);
      RunWords out{cig, cap, 0u};
      const uint32_t end = band_walk(m, w, B, n, k0, back, out);
      const bool over = out.runs > cap;
      used = over ? 0u : out.runs;
      rec = make_uint2(end, D | out.runs << KFMI_PATH_RUNS_SHIFT | (over ? KFMI_PATH_OVERFLOW : 0u));
    }
  }
#pragma unroll 1
  for (uint32_t r = used; r < cap; ++r) cig[r] = 0u;
  a.paths[t] = rec;
}

static hipError_t launch_paths(const PathArgs& a, uint64_t tasks, hipStream_t st)
{
  const bool str = a.strands != KFMI_STRAND_FWD;
  const dim3 grid((uint32_t) ((tasks + 255) / 256));
  const size_t lds = 4 * (size_t) stage_slot_bytes(a.m);
  if (a.m <= 128) {
    if (str) hipLaunchKernelGGL((paths_kernel<8, true>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((paths_kernel<8, false>), grid, dim3(256), lds, st, a);
  } else {
    if (str) hipLaunchKernelGGL((paths_kernel<16, true>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((paths_kernel<16, false>), grid, dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

static const uint64_t PATH_ROWS_CAP = 1ull << 30;   /* bytes of kept rows per launch */
static std::atomic<uint64_t> g_path_chunk{0};       /* kfmi_set_path_chunk: tasks per launch, 0 = by the cap */

extern "C" int32_t kfmi_set_path_chunk(uint64_t tasks)
{
  g_path_chunk.store(tasks ? (tasks + 63u) & ~63ull : 0u, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

extern "C" int32_t kfmi_align_paths(void* index, void* queries, void* hits, void* paths, void* cigars, uint32_t strands,
                                    uint32_t band, uint32_t max_edits, uint32_t cigar_entries)
{
  const uint32_t C = cigar_entries;
  if (band > KFMI_ALIGN_MAX_BAND || C < 1 || C > KFMI_PATH_MAX_ENTRIES) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  kfmi_res_t* rp = (kfmi_res_t*) paths;
  kfmi_res_t* rc = (kfmi_res_t*) cigars;
  if (!f || !q || !rh || !rp || !rc || rp == rh || rc == rh || rc == rp) return KFMI_E_BAD_ARGUMENT;
  const uint32_t ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  const uint64_t tasks = ns * q->num;
  if (rh->num != tasks || rp->num != tasks || rc->num != tasks * C) return KFMI_E_BAD_ARGUMENT;
  if (q->size < 1 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  TextCall c;
  int32_t err = c.open(f, q, {rh, rp, rc});
  if (err) return err;
  const uint32_t m = c.dq->size;
  /* tasks per launch: a multiple of 64 (of 256 by the cap), no more than the batch needs */
  const uint64_t knob = g_path_chunk.load(std::memory_order_relaxed);
  const uint64_t by_cap = (PATH_ROWS_CAP / (12ull * m)) & ~255ull;   /* >= 349,440 at m = 256 */
  uint64_t chunk = knob ? knob : by_cap;
  if (chunk > ((tasks + 63u) & ~63ull)) chunk = (tasks + 63u) & ~63ull;
  uint32_t* rows = nullptr;
  if (tasks && hipMalloc((void**) &rows, 12ull * m * chunk) != hipSuccess) {
    (void) hipGetLastError();
    return KFMI_E_DEVICE_ALLOC;
  }
  PathArgs a{};
  a.text = c.jsa + 2ull * c.di->bwtsize;
  a.rows = rows;
  a.stride = chunk;
  a.m = m;
  a.strands = strands;
  a.n = c.di->bwtsize - 1u;
  a.band = band;
  a.max_edits = max_edits;
  a.C = C;
  a.split4 = c.split4;
  err = c.begin();
  hipError_t he = hipSuccess;
  for (uint64_t base = 0; !err && he == hipSuccess && base < tasks; base += chunk) {
    const uint64_t cnt = tasks - base < chunk ? tasks - base : chunk;   /* even under BOTH: tasks and chunk are */
    a.ascii = c.dq->ascii + (base / ns) * m;
    a.num = cnt / ns;
    a.hits = reinterpret_cast<const uint2*>(rh->d_results) + base;
    a.paths = reinterpret_cast<uint2*>(rp->d_results) + base;
    a.cigars = rc->d_results + 2ull * C * base;
    he = launch_paths(a, cnt, c.l.st);
  }
  if (!err) err = c.finish();   /* waits for the launches that were queued, whatever `he` says */
  if (rows) (void) hipFree(rows);
  if (he != hipSuccess) {
    fprintf(stderr, "kstepfmi: paths_kernel launch failed: %s\n", hipGetErrorString(he));
    return KFMI_E_KERNEL;
  }
  return err;
}

}  // namespace kfmi
