/*
 * kfmi_jump.hip -- the text jump's tables (DESIGN.md 5a'', kstep_fmi.h): per
 * device copy the full suffix array sa[row], its inverse isa[pos] and the
 * text's 2-bit codes laid out as the walk's code stream, built from the
 * uploaded index alone; the auto rule, jump_min and the accessors (the setting
 * is with the other tables' in kfmi_tables.hip).  The kernel side is
 * skip_walk<.., JUMP = true> (kfmi_kernels.h).
 *
 * Build.  lf_next_kernel gives next[i] = LF_K(i), a '$' row D_s its own
 * successor.  Every chain of a text's index ends at a row D_s, the row of
 * suffix s, so SA[i] = s + K * (steps from i to D_s).  The steps are counted by
 * pointer jumping with a distance beside each pointer:
 *   next'[i] = next[next[i]],  dist'[i] = dist[i] + dist[next[i]]
 * (dist = 1 on ordinary rows, 0 on '$' rows), ceil(log2 rows) rounds between
 * two pairs of 4-byte arrays.  Then sa is written over the last pointers,
 * isa[sa[i]] = i over their spent twin, and the code stream is filled through
 * isa (jump_text_kernel).  The distances live where the line table (DESIGN.md
 * 5a''') goes: its 128-byte lines are 8 B x rows and a little, and they are
 * filled last, from isa and the code stream (jump_lines_kernel), when the
 * distances are spent -- so the build allocates nothing that goes.
 *
 * Exactness is checked, not assumed: the tables are kept only when every
 * chain ends at a '$' row, every sa value is a text position (<= n) and every
 * position 0 .. n got a row -- rows and positions are n + 1 each, so sa is then
 * a bijection with isa its inverse.  A 'ref'-mode index whose LF_K is not the
 * text's permutation fails one of the three and gets no tables, which is not
 * an error: the search walks on the skip table or the K-steps.
 *
 * Gathers and scatters into the 4 B x rows arrays (24 GB in two at 3 Gbase, past the
 * translation reach) go out as four exec-masked 16-lane groups when split_for
 * says so for their size; every load is 4 bytes at 4-byte alignment.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <shared_mutex>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_runtime.h"

namespace kfmi {

static std::atomic<uint32_t> g_jump_min{KFMI_JUMP_MIN_DEFAULT};
static std::atomic<int> g_jump_lines{-1};   /* -1: KFMI_JUMP_LINES, else 1; kfmi_set_jump_lines */

extern "C" int32_t kfmi_set_jump_min(uint32_t bases)
{
  if (bases < 1) return KFMI_E_BAD_ARGUMENT;
  g_jump_min.store(bases, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

extern "C" uint32_t kfmi_jump_min(void) { return g_jump_min.load(std::memory_order_relaxed); }

/* The line table's use by the search (the tables are built either way): 0 =
 * every lane takes the flat tables, 1 = windows of at most JUMP_LINE_W bases
 * take their line (default), with all the loads of that round trip issued
 * per 16-lane group where the tables are past the translation reach
 * (split_for, as for the other gathers), 2 = the lines with the window's loads
 * never split (the measured alternative, slower at 3 Gbase: DESIGN.md 5a''').
 * Process-wide, read where jump_min is read. */
extern "C" int32_t kfmi_set_jump_lines(uint32_t mode)
{
  if (mode > 2) return KFMI_E_BAD_ARGUMENT;
  g_jump_lines.store((int) mode, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

extern "C" uint32_t kfmi_jump_lines(void)
{
  const int v = g_jump_lines.load(std::memory_order_relaxed);
  if (v >= 0) return (uint32_t) v;
  static const uint32_t env = [] {   /* KFMI_JUMP_LINES, read once per process */
    const char* e = getenv("KFMI_JUMP_LINES");
    if (!e || !*e) return 1u;
    const int x = atoi(e);
    return x < 0 || x > 2 ? 1u : (uint32_t) x;
  }();
  return env;
}

static uint64_t text_words(uint64_t n) { return jump_text_words(n); }

/* The host's view of jump_line_at (kfmi_device.h), for the tests: out[0 .. 5] =
 * the lines' first dword in the allocation, the line count, and the ISA dword,
 * first window dword (both from the lines' start), bit shift and dword count
 * of a jump with nb bases left at text position p of an n-base text. */
extern "C" int32_t kfmi_jump_line_geometry(uint64_t n, uint64_t p, uint32_t nb, uint64_t* out)
{
  if (!out || n < 1 || n >= 0xFFFFFFFFull || p > n || nb < 1 || nb > JUMP_LINE_W || nb > p) return KFMI_E_BAD_ARGUMENT;
  const JumpLineAt at = jump_line_at((uint32_t) n, (uint32_t) p, nb);
  out[0] = jump_lines_off(n + 1);
  out[1] = jump_line_count(n);
  out[2] = at.isa_dw;
  out[3] = at.text_dw;
  out[4] = at.shift;
  out[5] = at.ndw;
  return KFMI_SUCCESS;
}

/* The auto rule (kstep_fmi.h): host arithmetic only. */
extern "C" uint32_t kfmi_jump_auto(uint64_t rows, uint32_t K, uint64_t budget_bytes)
{
  if (K < 1 || K > 2 || rows < 2 || rows > 0xFFFFFFFFull) return 0;
  return 16 * rows + 4 * text_words(rows - 1) <= budget_bytes ? 1u : 0u;
}

/* Plain-semantics per-lane layouts at K <= 2: the AltCounters layouts answer
 * with the reference's sentinel quirk, not the true interval. */
static bool jump_applies(const kfmi_dev_index* di)
{
  return di->K >= 1 && di->K <= 2 && !is_coop(di->backend) && (di->layout == LAY_INTER || di->layout == LAY_MID) &&
         di->bwtsize >= 2;
}

constexpr uint32_t JUMP_BAD_CHAIN = 1u, JUMP_BAD_POS = 2u, JUMP_BAD_ISA = 4u;

__device__ __forceinline__ int dollar_of(uint32_t row, const DollarArgs& dl, uint32_t K)
{
  int s = -1;
  for (int t = (int) K - 1; t >= 0; --t)
    if (dl.dpos[t] == row) s = t;
  return s;
}

__global__ __launch_bounds__(256) void jump_dist0_kernel(const uint32_t* __restrict__ next, uint64_t rows,
                                                         uint32_t* __restrict__ dist)
{
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256)
    dist[i] = next[i] == (uint32_t) i ? 0u : 1u;
}

/* One round: twice as far, and how far.  next[i] < rows (lf_next_kernel). */
__global__ __launch_bounds__(256) void jump_round_kernel(const uint32_t* __restrict__ next, const uint32_t* __restrict__ dist,
                                                         uint64_t rows, uint32_t split, uint32_t* __restrict__ next2,
                                                         uint32_t* __restrict__ dist2)
{
  const int grp = (int) (threadIdx.x & 63) / 16;
  for (uint64_t i0 = (uint64_t) blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < rows; i0 += (uint64_t) gridDim.x * 256) {
    const uint64_t i = i0 + (threadIdx.x & 63u);
    const bool on = i < rows;
    const uint32_t j = on ? next[i] : 0u;
    const uint32_t d = on ? dist[i] : 0u;
    const bool ok = on && (uint64_t) j < rows;
    uint32_t nj = j, dj = 0u;
    if (split) {   /* wave-uniform */
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (ok && grp == g) {
          nj = next[j];
          dj = dist[j];
        }
    } else if (ok) {
      nj = next[j];
      dj = dist[j];
    }
    if (on) {
      next2[i] = nj;
      dist2[i] = d + dj;
    }
  }
}

/* sa[i] = s + K * dist[i] with D_s = the end of i's chain, written over next. */
__global__ __launch_bounds__(256) void jump_sa_kernel(uint32_t* __restrict__ next_sa, const uint32_t* __restrict__ dist,
                                                      uint64_t rows, DollarArgs dl, uint32_t K, uint32_t* __restrict__ bad)
{
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256) {
    const int s = dollar_of(next_sa[i], dl, K);
    const uint64_t p = (uint64_t) (s < 0 ? 0 : s) + (uint64_t) K * dist[i];
    uint32_t v = (uint32_t) p;
    if (s < 0) {
      atomicOr(bad, JUMP_BAD_CHAIN);
      v = SKIP_NONE;
    } else if (p >= rows) {   /* positions are 0 .. n = rows - 1 */
      atomicOr(bad, JUMP_BAD_POS);
      v = SKIP_NONE;
    }
    next_sa[i] = v;
  }
}

/* isa[sa[i]] = i; isa was filled with SKIP_NONE. */
__global__ __launch_bounds__(256) void jump_isa_kernel(const uint32_t* __restrict__ sa, uint64_t rows, uint32_t split,
                                                       uint32_t* __restrict__ isa)
{
  const int grp = (int) (threadIdx.x & 63) / 16;
  for (uint64_t i0 = (uint64_t) blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < rows; i0 += (uint64_t) gridDim.x * 256) {
    const uint64_t i = i0 + (threadIdx.x & 63u);
    const uint32_t p = i < rows ? sa[i] : SKIP_NONE;
    const bool ok = (uint64_t) p < rows;
    if (split) {   /* wave-uniform */
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (ok && grp == g) isa[p] = (uint32_t) i;
    } else if (ok) {
      isa[p] = (uint32_t) i;
    }
  }
}

__global__ __launch_bounds__(256) void jump_isa_check_kernel(const uint32_t* __restrict__ isa, uint64_t rows,
                                                             uint32_t* __restrict__ bad)
{
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256)
    if ((uint64_t) isa[i] >= rows) atomicOr(bad, JUMP_BAD_ISA);
}

void free_jump(kfmi_dev_index* di)
{
  if (di->jump_sa) (void) hipFree(di->jump_sa);
  di->jump_sa = nullptr;
  di->jump_auto = -1;
}

/* The tables of a device copy built into di->jump_sa (caller holds ftab_mu):
 * one allocation [sa | isa | text | lines] that stays, so the kernel carries
 * one pointer.  The pointers ping-pong between the sa and isa parts, the
 * distances between two halves of the lines' part (32 dwords for every 16
 * rows and two lines more: at least 2 x rows dwords); the round count is
 * known, so the walk starts in the part that leaves the last pointers in
 * `sa`.  KFMI_E_DEVICE_ALLOC when it does not fit;
 * KFMI_SUCCESS with no tables (di->jump_none = 1) when the index fails the
 * exactness check. */
static int32_t build_jump(kfmi_dev_index* di, hipStream_t st)
{
  const uint64_t rows = di->bwtsize, n = rows - 1, words = text_words(n);
  const uint64_t loff = jump_lines_off(rows), lines = jump_line_count(n);
  uint32_t *keep = nullptr, *bad = nullptr;
  auto done = [&](int32_t code) {
    if (keep) (void) hipFree(keep);
    if (bad) (void) hipFree(bad);
    (void) hipGetLastError();
    return code;
  };
  /* the lines hold the 2 x rows distances: DW * (n / S + 2) >= (DW / S) * (n + 1) */
  static_assert(JUMP_LINE_DW >= 2 * JUMP_LINE_S, "two distance dwords per row fit the lines' part");
  if (hipMalloc((void**) &keep, 4 * (loff + lines * JUMP_LINE_DW)) != hipSuccess || hipMalloc((void**) &bad, 8) != hipSuccess)
    return done(KFMI_E_DEVICE_ALLOC);
  uint32_t* tmp = keep + loff;
  uint32_t* a[4] = {keep, tmp, keep + rows, tmp + rows};   /* next, dist and their twins */
  const uint32_t split = split_for(8 * rows, LAY_INTER) == 4u ? 1u : 0u;
  const dim3 grid(grid_blocks((rows + 255) / 256, 1u << 20));
  uint32_t rounds = 0;
  for (uint64_t span = 1; span < rows; span <<= 1) ++rounds;   /* after round r every row looks 2^r steps ahead */
  int cur = (rounds & 1u) ? 2 : 0;   /* next = a[cur], dist = a[cur + 1]; ends at 0 */
  SearchLaunch l{};
  l.st = st;
  l.ix = idx_args(di);
  l.num = rows;
  l.perm_next = a[cur];
  l.perm_bad = bad;
  uint32_t h_bad[2] = {0, 0};
  auto flags = [&] {   /* bad[0]: lf_next_kernel's image flag, bad[1]: ours */
    return hipGetLastError() == hipSuccess && hipMemcpyAsync(h_bad, bad, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipStreamSynchronize(st) == hipSuccess;
  };
  if (hipMemsetAsync(bad, 0, 8, st) != hipSuccess || dispatch(Op::PermCheck, di->K, di->nb, di->layout, l) != hipSuccess)
    return done(KFMI_E_KERNEL);
  hipLaunchKernelGGL(jump_dist0_kernel, grid, dim3(256), 0, st, a[cur], rows, a[cur + 1]);
  for (uint32_t r = 0; r < rounds; ++r, cur ^= 2)
    hipLaunchKernelGGL(jump_round_kernel, grid, dim3(256), 0, st, a[cur], a[cur + 1], rows, split, a[cur ^ 2],
                       a[(cur ^ 2) + 1]);
  uint32_t *sa = a[0], *dist = a[1], *isa = a[2], *text = keep + 2 * rows;   /* cur == 0 */
  hipLaunchKernelGGL(jump_sa_kernel, grid, dim3(256), 0, st, sa, dist, rows, di->dl, di->K, bad + 1);
  if (hipMemsetAsync(isa, 0xFF, 4 * rows, st) != hipSuccess) return done(KFMI_E_KERNEL);
  hipLaunchKernelGGL(jump_isa_kernel, grid, dim3(256), 0, st, sa, rows, split, isa);
  hipLaunchKernelGGL(jump_isa_check_kernel, grid, dim3(256), 0, st, isa, rows, bad + 1);
  if (!flags()) return done(KFMI_E_KERNEL);
  if (h_bad[0] | h_bad[1]) {   /* not the text's permutation: no tables, no error */
    di->jump_none = 1;
    return done(KFMI_SUCCESS);
  }
  l.jump_isa = isa;
  l.jump_text = text;
  l.jump_words = words;
  l.jump_split = l.ix.split == 1u ? 0u : 1u;
  l.num = n;
  l.jump_lines = tmp;   /* the distances are spent */
  if (dispatch(Op::JumpText, di->K, di->nb, di->layout, l) != hipSuccess ||
      dispatch(Op::JumpLines, di->K, di->nb, di->layout, l) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return done(KFMI_E_KERNEL);
  di->jump_sa = keep;   /* published complete; never replaced */
  keep = nullptr;
  return done(KFMI_SUCCESS);
}

/* The auto tables of an index, decided once per device copy, at an upload
 * after its auto skip table (use_tables decides them before it): built when kfmi_jump_auto says their peak fits the budget -- a
 * quarter of the device memory free right now, or kfmi_set_ftab_budget's
 * bytes.  Never an allocation error. */
int32_t auto_jump(kfmi_dev_index* di, hipStream_t st)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  if (di->jump_auto >= 0 || di->jump_sa) return KFMI_SUCCESS;
  di->jump_auto = 0;
  if (!jump_applies(di) || di->jump_none) return KFMI_SUCCESS;
  if (!kfmi_jump_auto(di->bwtsize, di->K, table_budget_now())) return KFMI_SUCCESS;
  const int32_t e = build_jump(di, st);
  if (e && e != KFMI_E_DEVICE_ALLOC) return e;
  di->jump_auto = (!e && di->jump_sa) ? 1 : 0;
  return KFMI_SUCCESS;
}

/* Sets ix.jsa .. for a search under the caller's resolved setting
 * (TableWants::jump): 2 = the auto tables if this copy has them, 1 = built now if
 * they are not there (an index that fails the exactness check still has none). */
int32_t use_jump(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, uint32_t want)
{
  const uint32_t folded = ix.jump_split & JUMP_FTAB_FOLDED;   /* use_ftab's bit: the table's, not the jump's */
  ix.jsa = nullptr;
  ix.jump_min = 0xFFFFFFFFu;
  ix.jump_split = 1 | folded;
  if (!want || !jump_applies(di)) return KFMI_SUCCESS;
  if (want == 2) {
    const int32_t e = auto_jump(di, st);
    if (e) return e;
  }
  {
    std::lock_guard<std::mutex> lk(di->ftab_mu);
    if (!di->jump_sa) {
      if (want == 2 || di->jump_none) return KFMI_SUCCESS;
      const int32_t e = build_jump(di, st);
      if (e) return e;
      if (!di->jump_sa) return KFMI_SUCCESS;
    }
  }
  ix.jsa = di->jump_sa;
  ix.jump_min = g_jump_min.load(std::memory_order_relaxed);
  const uint32_t lines = kfmi_jump_lines();
  const bool split4 = split_for(8ull * di->bwtsize, LAY_INTER) == 4u;
  ix.jump_split = (split4 ? JUMP_SPLIT4 : 0u) | (lines ? JUMP_LINES : 0u) | (lines == 1u && split4 ? JUMP_LINES_GROUPED : 0u) |
                  folded;
  return KFMI_SUCCESS;
}

static uint64_t jump_bytes_of(kfmi_dev_index* di)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  return di->jump_sa ? 8ull * di->bwtsize + 4 * text_words(di->bwtsize - 1) : 0ull;
}

static uint64_t jump_line_bytes_of(kfmi_dev_index* di)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  return di->jump_sa ? 4ull * JUMP_LINE_DW * jump_line_count(di->bwtsize - 1) : 0ull;
}

extern "C" uint64_t kfmi_device_jump_bytes(void* index) { return sum_members(index, jump_bytes_of); }

/* the line table's bytes, which kfmi_device_jump_bytes does not count */
extern "C" uint64_t kfmi_device_jump_line_bytes(void* index) { return sum_members(index, jump_line_bytes_of); }

/* Test accessor: the tables of the single-device copy, or of member `member`
 * of a device group, copied to sa[rows], isa[rows] and text[text_words];
 * KFMI_E_NOT_ON_DEVICE without tables, KFMI_E_BAD_ARGUMENT when the counts are
 * not the tables' own. */
extern "C" int32_t kfmi_device_jump_tables(void* index, uint32_t member, uint32_t* sa, uint32_t* isa, uint64_t rows,
                                           uint32_t* text, uint64_t words)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  if (!f || !sa || !isa || !text) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  kfmi_dev_index* di = nullptr;
  const int32_t e = member_index(f, member, &di);
  if (e) return e;
  std::lock_guard<std::mutex> tl(di->ftab_mu);
  if (!di->jump_sa) return KFMI_E_NOT_ON_DEVICE;
  if (rows != di->bwtsize || words != text_words(di->bwtsize - 1)) return KFMI_E_BAD_ARGUMENT;
  if (hipSetDevice(di->device) != hipSuccess) return KFMI_E_NO_DEVICE;
  HIP_OK(hipMemcpy(sa, di->jump_sa, 4ull * rows, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(isa, di->jump_sa + rows, 4ull * rows, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(text, di->jump_sa + 2 * rows, 4ull * words, hipMemcpyDeviceToHost));
  return KFMI_SUCCESS;
}

/* Test accessor: the raw line table of the same copy, `lines` lines of 32
 * dwords, the padding line included; the same codes. */
extern "C" int32_t kfmi_device_jump_lines(void* index, uint32_t member, uint32_t* out, uint64_t lines)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  if (!f || !out) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  kfmi_dev_index* di = nullptr;
  const int32_t e = member_index(f, member, &di);
  if (e) return e;
  std::lock_guard<std::mutex> tl(di->ftab_mu);
  if (!di->jump_sa) return KFMI_E_NOT_ON_DEVICE;
  if (lines != jump_line_count(di->bwtsize - 1)) return KFMI_E_BAD_ARGUMENT;
  if (hipSetDevice(di->device) != hipSuccess) return KFMI_E_NO_DEVICE;
  HIP_OK(hipMemcpy(out, di->jump_sa + jump_lines_off(di->bwtsize), 4ull * JUMP_LINE_DW * lines, hipMemcpyDeviceToHost));
  return KFMI_SUCCESS;
}

}  // namespace kfmi
