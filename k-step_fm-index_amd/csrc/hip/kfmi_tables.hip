/*
 * kfmi_tables.hip -- the tables derived from an uploaded index, per device
 * copy: the jump-start table (ftab), the skip table (5a'), the
 * remainder table (5e) and, built in kfmi_jump.hip, the text jump's tables
 * (5a'').  Their settings and how they resolve against each other, the auto
 * rules and the budget, the builds of the first three, a search's one call
 * (use_tables) and an upload's (auto_tables), the release, the byte accessors.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <shared_mutex>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_runtime.h"

namespace kfmi {

/* ---- settings, per calling thread: ftab -> skip -> jump ---- */
static thread_local int t_ftab = -1;   /* ftab bases; -1: KFMI_FTAB, else auto; -2: auto (kfmi_set_ftab) */
static thread_local int t_skip = -1;   /* skip table; -1: KFMI_SKIP, else auto; 0 off, 1 on, 2: auto (kfmi_set_skip) */
static thread_local int t_jump = -1;   /* text jump; -1: KFMI_JUMP, else auto; 0 off, 1 on, 2: auto (kfmi_set_jump) */

extern "C" int32_t kfmi_set_ftab(uint32_t bases)
{
  if (bases > 16 && bases != KFMI_FTAB_AUTO) return KFMI_E_BAD_ARGUMENT;
  t_ftab = bases == KFMI_FTAB_AUTO ? -2 : (int) bases;
  return KFMI_SUCCESS;
}

/* The calling thread's setting: a base count, 0 (off) or KFMI_FTAB_AUTO, which
 * use_ftab resolves per index. */
static uint32_t ftab_bases(void)
{
  if (t_ftab >= 0) return (uint32_t) t_ftab;
  if (t_ftab == -2) return KFMI_FTAB_AUTO;
  static const uint32_t env = [] {   /* KFMI_FTAB, read once per process */
    const char* e = getenv("KFMI_FTAB");
    if (!e || !*e || !strcmp(e, "auto")) return (uint32_t) KFMI_FTAB_AUTO;
    const int v = atoi(e);
    return v > 0 && v <= 16 ? (uint32_t) v : 0u;
  }();
  return env;
}

/* The auto rule (kstep_fmi.h): host arithmetic only, so a CPU test calls it. */
extern "C" uint32_t kfmi_ftab_auto_bases(uint64_t rows, uint32_t K, uint64_t budget_bytes)
{
  if (K < 1 || K > 4 || rows < 8) return 0;
  uint32_t n = 16 - 16 % K;
  while (n && (1ull << (2 * n)) > 2 * rows) n -= K;
  while (n && (8ull << (2 * n)) > budget_bytes) n -= K;
  return n;
}

/* KFMI_SKIP / KFMI_JUMP: 0, 1 or "auto" (2; the default) */
static int mode_from_env(const char* name)
{
  const char* e = getenv(name);
  if (!e || !*e || !strcmp(e, "auto")) return 2;
  return atoi(e) ? 1 : 0;
}

extern "C" int32_t kfmi_set_skip(uint32_t mode)
{
  if (mode > 1 && mode != KFMI_SKIP_AUTO) return KFMI_E_BAD_ARGUMENT;
  t_skip = mode == KFMI_SKIP_AUTO ? 2 : (int) mode;
  return KFMI_SUCCESS;
}

/* The calling thread's skip-table setting resolved against its ftab setting
 * (kstep_fmi.h): 0 = off, 1 = on (kfmi_set_skip(1) / KFMI_SKIP=1: built at the
 * first search, an allocation failure is an error), 2 = auto and in effect --
 * exactly when the ftab setting is auto as well, so an explicit kfmi_set_ftab
 * (0 or N) keeps naming the walk it always named. */
static uint32_t skip_wanted(void)
{
  int v = t_skip;
  if (v < 0) {
    static const int env = mode_from_env("KFMI_SKIP");   /* read once per process */
    v = env;
  }
  if (v == 2) return ftab_bases() == KFMI_FTAB_AUTO ? 2u : 0u;
  return (uint32_t) v;
}

extern "C" uint32_t kfmi_skip_in_effect(void) { return skip_wanted(); }

/* The auto rule (kstep_fmi.h): host arithmetic only, so a CPU test calls it. */
extern "C" uint32_t kfmi_skip_auto(uint64_t rows, uint32_t K, uint64_t budget_bytes)
{
  if (K < 1 || K > 2 || rows < 8 || rows > 0xFFFFFFFFull) return 0;
  return 16 * rows <= budget_bytes ? 1u : 0u;
}

extern "C" int32_t kfmi_set_jump(uint32_t mode)
{
  if (mode > 1 && mode != KFMI_JUMP_AUTO) return KFMI_E_BAD_ARGUMENT;
  t_jump = mode == KFMI_JUMP_AUTO ? 2 : (int) mode;
  return KFMI_SUCCESS;
}

/* 0 = off, 1 = on (explicit), 2 = auto and in effect: exactly when the skip
 * setting is auto and in effect, so kfmi_set_ftab(0), KFMI_SKIP=0 and an
 * explicit ftab count keep naming the walks they always named. */
static uint32_t jump_wanted(void)
{
  int v = t_jump;
  if (v < 0) {
    static const int env = mode_from_env("KFMI_JUMP");   /* read once per process */
    v = env;
  }
  if (v == 2) return skip_wanted() == 2u ? 2u : 0u;
  return (uint32_t) v;
}

extern "C" uint32_t kfmi_jump_in_effect(void) { return jump_wanted(); }

TableWants tables_wanted(void) { return TableWants{ftab_bases(), skip_wanted(), jump_wanted()}; }

static std::atomic<uint64_t> g_ftab_budget{KFMI_FTAB_BUDGET_FREE};

extern "C" int32_t kfmi_set_ftab_budget(uint64_t bytes)
{
  g_ftab_budget.store(bytes, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

uint64_t table_budget_now(void)
{
  const uint64_t budget = g_ftab_budget.load(std::memory_order_relaxed);
  if (budget != KFMI_FTAB_BUDGET_FREE) return budget;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void) hipGetLastError();
    return 0;
  }
  return (uint64_t) free_b / 4;
}

/* ---- remainder table ---- */
/* Reads with m % K = rem != 0 (the reference reads P[-1] there, defect B6):
 * their last rem bases are resolved by the remainder table, built once per
 * (index, rem) from the uploaded layout (rem_tab_kernel), and the K-steps
 * cover bases 0 .. m-rem-1.  The result is the reads' suffix-array interval,
 * which is what every plain-semantics backend returns for m % K = 0; the
 * AltCounters-semantics backends keep rejecting such reads (their intervals
 * differ from the true ones where the reference's sentinel counts, and the
 * reference defines no result here).  The ftab is not combined with it. */
bool rem_supported(int layout)
{
  return layout == LAY_INTER || layout == LAY_MID || layout == LAY_GRP;
}

static int32_t use_rtab(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, uint32_t rem)
{
  ix.rtab = nullptr;
  ix.rem = 0;
  if (!rem) return KFMI_SUCCESS;
  if (rem >= di->K || rem > 3 || !rem_supported(di->layout)) return KFMI_E_BAD_ARGUMENT;
  {
    std::lock_guard<std::mutex> lk(di->ftab_mu);
    if (!di->rtab[rem]) {
      uint2* t = nullptr;
      if (hipMalloc((void**) &t, 8ull << (2 * rem)) != hipSuccess) return KFMI_E_DEVICE_ALLOC;
      SearchLaunch a{};
      a.st = st;
      a.ix = idx_args(di);
      a.ftab_out = t;
      a.rem = rem;
      if (dispatch(Op::RemTab, di->K, di->nb, di->layout, a) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void) hipFree(t);
        return KFMI_E_KERNEL;
      }
      di->rtab[rem] = t;   /* published complete; never replaced */
    }
  }
  ix.rtab = di->rtab[rem];
  ix.rem = rem;
  ix.ftab = nullptr;
  ix.ftab_steps = 0;
  ix.ftab_mask = 0;
  ix.jump_split &= ~JUMP_FTAB_FOLDED;
  return KFMI_SUCCESS;
}

/* ---- jump-start table ---- */
/* The table of `bases` bases built into di->ftab[bases] (caller holds ftab_mu):
 * one launch per level on `st` (launch_ftab), waited for. */
static int32_t build_ftab(kfmi_dev_index* di, hipStream_t st, uint32_t bases)
{
  uint2* t = nullptr;
  if (hipMalloc((void**) &t, 8ull << (2 * bases)) != hipSuccess) {
    (void) hipGetLastError();
    return KFMI_E_DEVICE_ALLOC;
  }
  SearchLaunch a{};
  a.st = st;
  a.ix = idx_args(di);
  a.ftab_out = t;
  a.ftab_steps = bases / di->K;
  a.ftab_n = 1ull << (2 * bases);
  if (dispatch(Op::Ftab, di->K, di->nb, di->layout, a) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void) hipFree(t);
    return KFMI_E_KERNEL;
  }
  di->ftab[bases] = t;   /* published complete; never replaced */
  return KFMI_SUCCESS;
}

/* The auto table of an index (KFMI_FTAB_AUTO), decided once per device copy
 * (device `di->device` current): kfmi_ftab_auto_bases of its rows, K and the
 * budget (table_budget_now) and, when that table cannot be allocated, K bases
 * fewer until one can or none is left.  Never an allocation error: the search
 * then walks every step.  Called from the uploads (auto_tables) and, for an
 * index uploaded under another setting, from use_ftab.  *bases (may be null) =
 * its base count, 0 when it has none; *built (may be null) = this call built it. */
static int32_t auto_ftab(kfmi_dev_index* di, hipStream_t st, uint32_t* bases, bool* built = nullptr)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  if (built) *built = false;
  if (di->ftab_auto < 0) {
    uint32_t n = kfmi_ftab_auto_bases(di->bwtsize, di->K, table_budget_now());
    for (; n; n -= di->K) {
      if (di->ftab[n]) break;   /* an explicit setting built it already */
      const int32_t e = build_ftab(di, st, n);
      if (!e) {
        if (built) *built = true;
        break;
      }
      if (e != KFMI_E_DEVICE_ALLOC) return e;
    }
    di->ftab_auto = (int) n;
  }
  if (bases) *bases = (uint32_t) di->ftab_auto;
  return KFMI_SUCCESS;
}

/* The ftab of `bases` bases (KFMI_FTAB_AUTO: the index's auto table), built
 * on the device from the uploaded layout with the search's own LF steps when
 * it is not there yet; sets ix.ftab (null when off or when bases is not a
 * multiple of K). */
static int32_t use_ftab(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, uint32_t bases)
{
  ix.ftab = nullptr;
  ix.ftab_steps = 0;
  ix.ftab_mask = 0;
  ix.jump_split &= ~JUMP_FTAB_FOLDED;
  if (bases == KFMI_FTAB_AUTO) {
    const int32_t e = auto_ftab(di, st, &bases);
    if (e) return e;
  }
  if (!bases || bases % di->K || bases > 16) return KFMI_SUCCESS;
  {
    std::lock_guard<std::mutex> lk(di->ftab_mu);
    if (!di->ftab[bases]) {
      const int32_t e = build_ftab(di, st, bases);
      if (e) return e;
    }
    if ((di->ftab_folded >> bases) & 1u) ix.jump_split |= JUMP_FTAB_FOLDED;   /* the table's form goes with its pointer */
  }
  ix.ftab = di->ftab[bases];
  ix.ftab_steps = bases / di->K;
  ix.ftab_mask = bases >= 16 ? 0xFFFFFFFFu : (1u << (2 * bases)) - 1u;
  return KFMI_SUCCESS;
}

/* ---- skip table ---- */
/* Skip table, doubling (the exactness argument: skip_level0_kernel): entry i of
 * 2s steps = entry i of s steps, then the entry of the row it ends in, whose
 * codes go `shift` = 2K*s bits above the first half's; invalid when either
 * half is.  The second lookup is a gather into a table that can lie past the
 * translation reach (24 GB at 3 Gbase): with `split` it is issued as four
 * exec-masked 16-lane groups, like the task kernels' index gathers.  Entry
 * loads are 8 bytes at 8-byte alignment, never wider (load_words' rule). */
__global__ __launch_bounds__(256) void skip_double_kernel(const uint2* __restrict__ in, uint64_t rows, uint32_t shift,
                                                          uint32_t split, uint2* __restrict__ out)
{
  const int grp = (int) (threadIdx.x & 63) / 16;
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256) {
    const uint2 a = in[i];
    const bool ok = a.x != SKIP_NONE && (uint64_t) a.x < rows;
    uint2 b = make_uint2(SKIP_NONE, 0u);
    if (split) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (ok && grp == g) b = in[a.x];
    } else if (ok) {
      b = in[a.x];
    }
    out[i] = (ok && b.x != SKIP_NONE) ? make_uint2(b.x, a.y | (b.y << shift)) : make_uint2(SKIP_NONE, 0u);
  }
}

/* The skip table of a device copy built into di->skip (caller holds ftab_mu):
 * level 0 from the uploaded layout, then log2(16 / K) doublings between two
 * buffers; the second buffer is freed before returning.  KFMI_E_DEVICE_ALLOC
 * when the two buffers do not fit. */
static int32_t build_skip(kfmi_dev_index* di, hipStream_t st)
{
  const uint64_t rows = di->bwtsize;
  uint2* buf[2] = {nullptr, nullptr};
  for (uint2*& b : buf)
    if (hipMalloc((void**) &b, 8ull * rows) != hipSuccess) {
      (void) hipGetLastError();
      if (buf[0]) (void) hipFree(buf[0]);
      return KFMI_E_DEVICE_ALLOC;
    }
  SearchLaunch a{};
  a.st = st;
  a.ix = idx_args(di);
  a.num = rows;
  a.skip_out = buf[0];
  bool ok = dispatch(Op::Skip0, di->K, di->nb, di->layout, a) == hipSuccess;
  const uint32_t J = 16u / di->K;
  const uint32_t split = split_for(8ull * rows, LAY_INTER) == 4u ? 1u : 0u;
  int cur = 0;
  for (uint32_t s = 1; ok && s < J; s *= 2, cur ^= 1) {
    hipLaunchKernelGGL(skip_double_kernel, dim3(grid_blocks((rows + 255) / 256, 1u << 20)), dim3(256), 0, st, buf[cur],
                       rows, 2u * di->K * s, split, buf[cur ^ 1]);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  (void) hipFree(buf[cur ^ 1]);
  if (!ok) {
    (void) hipFree(buf[cur]);
    return KFMI_E_KERNEL;
  }
  di->skip = buf[cur];   /* published complete; never replaced */
  return KFMI_SUCCESS;
}

/* Whether a device copy takes the skip table at all: the per-lane (task)
 * kernels at K <= 2.  The coop kernels, K = 3 / 4 and every non-search kernel
 * ignore it (DESIGN.md 5a'), so no table is built for them. */
static bool skip_applies(const kfmi_dev_index* di)
{
  return di->K >= 1 && di->K <= 2 && !is_coop(di->backend) && di->layout != LAY_GRP;
}

/* The auto skip table of an index, decided once per device copy after its auto
 * ftab: built when kfmi_skip_auto says the table and its transient twin fit the
 * budget (table_budget_now).  Never an error when it does not fit: without the
 * table the search walks every K-step. */
static int32_t auto_skip(kfmi_dev_index* di, hipStream_t st)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  if (di->skip_auto >= 0 || di->skip) return KFMI_SUCCESS;
  di->skip_auto = 0;
  if (!skip_applies(di)) return KFMI_SUCCESS;
  if (!kfmi_skip_auto(di->bwtsize, di->K, table_budget_now())) return KFMI_SUCCESS;
  const int32_t e = build_skip(di, st);
  if (e && e != KFMI_E_DEVICE_ALLOC) return e;
  di->skip_auto = e ? 0 : 1;
  return KFMI_SUCCESS;
}

/* Sets ix.skip for a search under the caller's resolved setting (skip_wanted):
 * 2 = the auto table if this copy has one (decided here for a copy uploaded
 * under another setting), 1 = built now if it is not there. */
static int32_t use_skip(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, uint32_t want)
{
  ix.skip = nullptr;
  ix.skip_rows = 0;
  ix.skip_steps = 0;
  ix.skip_split = 1;
  if (!want || !skip_applies(di)) return KFMI_SUCCESS;
  if (want == 2) {
    const int32_t e = auto_skip(di, st);
    if (e) return e;
  }
  {
    std::lock_guard<std::mutex> lk(di->ftab_mu);
    if (!di->skip) {
      if (want == 2) return KFMI_SUCCESS;
      const int32_t e = build_skip(di, st);
      if (e) return e;
    }
  }
  ix.skip = di->skip;
  ix.skip_rows = di->bwtsize;
  ix.skip_steps = 16u / di->K;
  ix.skip_split = split_for(8ull * di->bwtsize, LAY_INTER);
  return KFMI_SUCCESS;
}

/* ---- folded jump-start table (DESIGN.md 5a'''', kfmi_device.h ftab_entry_at) ---- */
static std::atomic<int> g_ftab_fold{-1};          /* -1: KFMI_FTAB_FOLD, else 1; kfmi_set_ftab_fold */
static std::atomic<uint32_t> g_ftab_fold_bound{0};   /* test knob: lowers the fit rule's bound; 0 = the rule's own */

extern "C" int32_t kfmi_set_ftab_fold(uint32_t on)
{
  if (on > 1) return KFMI_E_BAD_ARGUMENT;
  g_ftab_fold.store((int) on, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

extern "C" uint32_t kfmi_ftab_fold(void)
{
  const int v = g_ftab_fold.load(std::memory_order_relaxed);
  if (v >= 0) return (uint32_t) v;
  static const uint32_t env = [] {   /* KFMI_FTAB_FOLD, read once per process */
    const char* e = getenv("KFMI_FTAB_FOLD");
    return !e || !*e || atoi(e) ? 1u : 0u;
  }();
  return env;
}

extern "C" int32_t kfmi_set_ftab_fold_bound(uint32_t bound)
{
  g_ftab_fold_bound.store(bound, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

/* The host's view of the folded form, for the tests (pure arithmetic). */
extern "C" uint32_t kfmi_ftab_fold_bound(uint64_t n) { return n >= 0xFFFFFFFFull ? 0u : ftab_fold_bound((uint32_t) n); }

extern "C" uint32_t kfmi_ftab_fold_fits(uint64_t n, uint64_t max_width)
{
  return n < 0xFFFFFFFFull && max_width <= 0xFFFFFFFFull && ftab_fold_fits((uint32_t) n, (uint32_t) max_width) ? 1u : 0u;
}

extern "C" int32_t kfmi_ftab_fold_encode(uint64_t n, uint32_t L, uint32_t R, uint32_t p, uint32_t* out)
{
  if (!out || n >= 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  if (R - L == 1u ? (uint64_t) p > n : !ftab_fold_fits((uint32_t) n, R - L)) return KFMI_E_BAD_ARGUMENT;
  const uint2 e = ftab_fold_entry(L, R, p);
  out[0] = e.x;
  out[1] = e.y;
  return KFMI_SUCCESS;
}

extern "C" int32_t kfmi_ftab_fold_decode(uint64_t n, uint32_t x, uint32_t y, uint32_t folded, uint32_t* out)
{
  if (!out || n >= 0xFFFFFFFFull) return KFMI_E_BAD_ARGUMENT;
  const FtabAt at = ftab_entry_at(make_uint2(x, y), folded != 0u, (uint32_t) n);
  out[0] = at.L;
  out[1] = at.R;
  out[2] = at.p;
  return KFMI_SUCCESS;
}

/* The fit rule's input: the largest width other than 1 of the table's entries,
 * 0xFFFFFFFF when a one-row entry names no row of the index (never on a valid
 * table; it refuses the fold).  Streaming; one atomic per wave. */
__global__ __launch_bounds__(256) void ftab_fold_check_kernel(const uint2* __restrict__ t, uint64_t entries, uint32_t rows,
                                                              uint32_t* __restrict__ maxw)
{
  uint32_t m = 0;
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < entries; i += (uint64_t) gridDim.x * 256) {
    const uint2 e = t[i];
    const uint32_t w = e.y - e.x;
    if (w != 1u) m = max(m, w);
    else if (e.x >= rows) m = 0xFFFFFFFFu;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) m = max(m, (uint32_t) __shfl_xor((int) m, o));
  if ((threadIdx.x & 63u) == 0u && m) atomicMax(maxw, m);
}

/* {L, R} -> the folded entry, in place, every thread its own entries.  The
 * sa[L] gather of the one-row entries goes out as four exec-masked 16-lane
 * groups where sa lies past the translation reach (`split`, split_for), as the
 * other gathers into the text jump's tables do.  L < rows (the check above). */
__global__ __launch_bounds__(256) void ftab_fold_kernel(uint2* __restrict__ t, uint64_t entries,
                                                        const uint32_t* __restrict__ sa, uint32_t split)
{
  const int grp = (int) (threadIdx.x & 63) / 16;
  for (uint64_t i0 = (uint64_t) blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < entries; i0 += (uint64_t) gridDim.x * 256) {
    const uint64_t i = i0 + (threadIdx.x & 63u);
    const bool on = i < entries;
    const uint2 e = on ? t[i] : make_uint2(0u, 0u);
    const bool one = on && e.y - e.x == 1u;
    uint32_t p = 0u;
    if (split) {   /* wave-uniform */
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (one && grp == g) p = sa[e.x];
    } else if (one) {
      p = sa[e.x];
    }
    if (on) t[i] = ftab_fold_entry(e.x, e.y, p);
  }
}

/* The fold pass of an upload (auto_tables; the handle is locked exclusively, so
 * nothing reads the copy): the auto table this upload built, rewritten into the
 * folded form when the fit rule holds for it -- decided on the device by a
 * reduction over the table -- and left {L, R} otherwise, which is no error.
 * The text jump's tables are this upload's own, so their exactness check passed
 * and every sa value is a position <= n. */
static int32_t fold_ftab(kfmi_dev_index* di, hipStream_t st)
{
  if (!kfmi_ftab_fold()) return KFMI_SUCCESS;
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  const int N = di->ftab_auto;
  if (N <= 0 || !di->ftab[N] || !di->jump_sa || ((di->ftab_folded >> N) & 1u)) return KFMI_SUCCESS;
  const uint64_t entries = 1ull << (2 * N);
  const uint32_t rows = di->bwtsize;
  uint32_t* d_max = nullptr;
  if (hipMalloc((void**) &d_max, 4) != hipSuccess) {
    (void) hipGetLastError();
    return KFMI_SUCCESS;
  }
  uint32_t h_max = 0xFFFFFFFFu;
  const dim3 grid(grid_blocks((entries + 255) / 256, 1u << 14));
  bool ok = hipMemsetAsync(d_max, 0, 4, st) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(ftab_fold_check_kernel, grid, dim3(256), 0, st, di->ftab[N], entries, rows, d_max);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&h_max, d_max, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
  }
  (void) hipFree(d_max);
  if (!ok) return KFMI_E_KERNEL;
  uint32_t bound = ftab_fold_bound(rows - 1u);
  const uint32_t lowered = g_ftab_fold_bound.load(std::memory_order_relaxed);
  if (lowered && lowered < bound) bound = lowered;
  if (h_max >= bound) return KFMI_SUCCESS;   /* does not fit: the table stays {L, R} */
  const uint32_t split = split_for(8ull * rows, LAY_INTER) == 4u ? 1u : 0u;
  hipLaunchKernelGGL(ftab_fold_kernel, grid, dim3(256), 0, st, di->ftab[N], entries, di->jump_sa, split);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return KFMI_E_KERNEL;
  di->ftab_folded |= 1u << N;
  return KFMI_SUCCESS;
}

/* ---- one call per search, one per upload ---- */
/* The tables of one search under the caller's settings `w`, set in ix, each
 * built first where `w` asks for it and the copy has none: the ftab, the
 * remainder table of the reads' `rem` (which clears the ftab), the text jump's
 * tables, the skip table.  On a copy uploaded under another setting this
 * decides the auto jump tables before the auto skip table, the other way round
 * from an upload (auto_tables); it always did, and stays so. */
int32_t use_tables(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, const TableWants& w, uint32_t rem)
{
  int32_t err = use_ftab(di, st, ix, w.ftab);
  if (!err) err = use_rtab(di, st, ix, rem);
  if (!err) err = use_jump(di, st, ix, w.jump);
  if (!err) err = use_skip(di, st, ix, w.skip);
  return err;
}

/* An upload's part, like the re-layout, so that no search pays for a build:
 * each table whose resolved setting is auto, decided and built once (device
 * `di->device` current): ftab, skip, jump.  Not fitting is never an error.
 * Last, the fold pass (fold_ftab) -- here only: a table built at a search, while
 * other searches may hold the shared lock, is never rewritten. */
int32_t auto_tables(kfmi_dev_index* di, hipStream_t st, const TableWants& w)
{
  int32_t err = KFMI_SUCCESS;
  bool ftab_built = false, jump_built = false;
  if (w.ftab == KFMI_FTAB_AUTO) err = auto_ftab(di, st, nullptr, &ftab_built);
  if (!err && w.skip == 2u) err = auto_skip(di, st);
  if (!err && w.jump == 2u) {
    const bool had = di->jump_sa != nullptr;
    err = auto_jump(di, st);
    jump_built = !err && !had && di->jump_sa != nullptr;
  }
  /* the fold: only a table and text-jump tables this upload built itself */
  if (!err && ftab_built && jump_built) err = fold_ftab(di, st);
  return err;
}

/* Frees the derived tables of a device copy that is about to be replaced
 * (caller holds the handle's exclusive lock: no search reads them).  They are
 * derived data, up to 34 GB each, and the replacing upload needs the memory:
 * a K = 4 copy re-laid for another backend holds two 96 GB layouts for a
 * moment.  Should that upload fail, the old copy stays searchable and builds
 * its tables again on demand -- except when it fails for lack of device
 * memory: then transferCPUtoGPU frees the old copy too and uploads again. */
void drop_ftabs(kfmi_dev_index* di)
{
  if (!di) return;
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  if (di->device >= 0) (void) hipSetDevice(di->device);
  for (uint2*& t : di->ftab)
    if (t) {
      (void) hipFree(t);
      t = nullptr;
    }
  di->ftab_auto = -1;
  di->ftab_folded = 0;
  if (di->skip) (void) hipFree(di->skip);   /* the skip table goes with them */
  di->skip = nullptr;
  di->skip_auto = -1;
  free_jump(di);   /* and the text jump's */
}

uint64_t sum_members(void* index, uint64_t (*of)(kfmi_dev_index*))
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  if (!f) return 0;
  std::shared_lock<RwLock> lk(index_lock(f));
  uint64_t b = 0;
  if (f->grp) {
    const GroupIndex* g = (const GroupIndex*) f->grp;
    for (int i = 0; i < g->n; ++i) b += of(g->di[i]);
  } else if (f->dev) {
    b = of(f->dev);
  }
  return b;
}

int32_t member_index(const kfmi_fmi_t* f, uint32_t member, kfmi_dev_index** di)
{
  *di = f->dev;
  if (f->grp) {
    const GroupIndex* g = (const GroupIndex*) f->grp;
    if ((int) member >= g->n) return KFMI_E_BAD_ARGUMENT;
    *di = g->di[member];
  } else if (member) {
    return KFMI_E_BAD_ARGUMENT;
  }
  return *di ? KFMI_SUCCESS : KFMI_E_NOT_ON_DEVICE;
}

static uint64_t ftab_bytes_of(kfmi_dev_index* di)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  uint64_t b = 0;
  for (uint32_t n = 1; n <= 16; ++n)
    if (di->ftab[n]) b += 8ull << (2 * n);
  return b;
}

static uint64_t skip_bytes_of(kfmi_dev_index* di)
{
  std::lock_guard<std::mutex> lk(di->ftab_mu);
  return di->skip ? 8ull * di->bwtsize : 0ull;
}

extern "C" uint64_t kfmi_device_ftab_bytes(void* index) { return sum_members(index, ftab_bytes_of); }

extern "C" uint64_t kfmi_device_skip_bytes(void* index) { return sum_members(index, skip_bytes_of); }

/* Test accessor: raw entries [first, first + count) of the auto jump-start table
 * of the single-device copy or of a group member, as stored (kstep_fmi.h). */
extern "C" int32_t kfmi_device_ftab_entries(void* index, uint32_t member, uint32_t* out, uint64_t first, uint64_t count,
                                            uint32_t* bases, uint32_t* folded)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  if (!f || !out) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  kfmi_dev_index* di = nullptr;
  const int32_t e = member_index(f, member, &di);
  if (e) return e;
  std::lock_guard<std::mutex> tl(di->ftab_mu);
  const int N = di->ftab_auto;
  if (N <= 0 || !di->ftab[N]) return KFMI_E_NOT_ON_DEVICE;
  const uint64_t entries = 1ull << (2 * N);
  if (first > entries || count > entries - first) return KFMI_E_BAD_ARGUMENT;
  if (hipSetDevice(di->device) != hipSuccess) return KFMI_E_NO_DEVICE;
  if (count) HIP_OK(hipMemcpy(out, di->ftab[N] + first, 8ull * count, hipMemcpyDeviceToHost));
  if (bases) *bases = (uint32_t) N;
  if (folded) *folded = (di->ftab_folded >> N) & 1u;
  return KFMI_SUCCESS;
}

/* Test accessor: the single-device copy's skip table copied to `out`
 * (`entries` uint2 {row, code}); KFMI_E_NOT_ON_DEVICE without a table or on a
 * device group, KFMI_E_BAD_ARGUMENT when `entries` is not its row count. */
extern "C" int32_t kfmi_device_skip_table(void* index, void* out, uint64_t entries, uint32_t* steps)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  if (!f || !out) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  kfmi_dev_index* di = nullptr;
  const int32_t e = f->grp ? KFMI_E_NOT_ON_DEVICE : member_index(f, 0, &di);
  if (e) return e;
  std::lock_guard<std::mutex> tl(di->ftab_mu);
  if (!di->skip) return KFMI_E_NOT_ON_DEVICE;
  if (entries != di->bwtsize) return KFMI_E_BAD_ARGUMENT;
  if (hipSetDevice(di->device) != hipSuccess) return KFMI_E_NO_DEVICE;
  HIP_OK(hipMemcpy(out, di->skip, 8ull * entries, hipMemcpyDeviceToHost));
  if (steps) *steps = 16u / di->K;
  return KFMI_SUCCESS;
}

}  // namespace kfmi
