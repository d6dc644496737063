/*
 * kfmi_paths.hip -- alignment paths: the CIGAR and the end position of every
 * task's placement at the begin position its hit holds (kstep_fmi.h section 2,
 * "align paths"; not in the reference, which stops at
 * intervals).
 *
 * The frame is kfmi_text.h's: one lane per task, the read in registers, the
 * window [c - w, c + m + w) of the band's centre c a BandWindow.  A lane has
 * one candidate, so there is one load round and no sa load.
 *
 * The forward pass is the banded row step with each row kept (band_rows_keep,
 * kfmi_align_dp.h): three words per row -- vp, hp, eq -- go to a workspace in
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

#include "kfmi_text.h"
#include "kfmi_path_dp.h"

namespace kfmi {

struct PathArgs : TextArgs {            /* ascii, num: the launch's reads */
  const uint2* __restrict__ hits;      /* one record per task; x is read */
  uint2* __restrict__ paths;           /* one record per task */
  uint32_t* __restrict__ cigars;       /* 2C words per task */
  uint32_t* rows;                      /* the kept rows: word p of row r of task t at (3 r + p) * stride + t */
  uint64_t stride;
  uint32_t band, max_edits, C;
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

template <int MAXW, bool STR>
__global__ __launch_bounds__(256) void paths_kernel(PathArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  uint64_t t;
  if (!text_task<MAXW, STR>(a.ascii, a.num, a.m, a.strands, stage, cw, t)) return;
  const uint32_t m = a.m, n = a.n, w = a.band, cap = 2u * a.C;
  const uint32_t B = a.hits[t].x;
  const bool in = B != KFMI_HIT_NONE && n >= m && B <= n;
  const uint32_t c = in ? (B < n - m ? B : n - m) : 0u;   /* the band's centre: c + m <= n */
  const bool sc = in && B - c <= w;
  BandWindow<MAXW> win(sc, sc ? n - c - m : 0u, m, w, n);   /* the read's last base: base n - c - m of the stream */
  under_group_mask(a.split4, lane_group(), [&] { win.load(a.text); });
  uint32_t* cig = a.cigars + t * cap;
  uint2 rec = make_uint2(KFMI_HIT_NONE, 0u);
  uint32_t used = 0u;
  if (sc) {
    KeepRows keep{a.rows + t, a.stride};
    uint32_t vp, vn, s0;
    band_rows_keep<MAXW>(cw, win.tx, m, w, win.sh, win.low, keep, vp, vn, s0);
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
  return launch_text(a.m, a.strands, tasks, st, [&](auto W, auto S, dim3 grid, size_t lds) {
    hipLaunchKernelGGL((paths_kernel<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, st, a);
  });
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
  DeviceScratch rows;
  if (tasks && (err = rows.alloc(12ull * m * chunk))) return err;
  PathArgs a{c.args(strands)};
  a.rows = rows.p;
  a.stride = chunk;
  a.band = band;
  a.max_edits = max_edits;
  a.C = C;
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
  return launch_result(err, he, "paths_kernel");
}

}  // namespace kfmi
