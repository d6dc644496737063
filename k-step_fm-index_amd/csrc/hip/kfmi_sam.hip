/*
 * kfmi_sam.hip -- SAM lines: one record per read from the records of
 * kfmi_align_seeds, kfmi_align_paths and kfmi_map_quality, formatted on the
 * device (kstep_fmi.h section 2, "SAM lines"; not in the
 * reference, which stops at intervals).  The arithmetic of a line -- status,
 * length, bytes -- is csrc/kfmi_sam.h's, which csrc/host/sam.c compiles too.
 *
 * sam_length_kernel works on records alone, one lane per task: the task's
 * status, in BOTH mode the read's choice by one exchange with lane ^ 1, and the
 * exact length of the line, which needs no text base -- a base under X costs
 * digits(c) + 1 bytes whatever its letter.  It leaves one word per task: the
 * length (0 for the task that writes nothing), which line, the YU code.
 *
 * An exclusive scan (rocprim, u32 -> u64) turns the lengths into offsets; the
 * total comes back in one 8-byte copy and sizes the text's allocation.
 *
 * sam_write_kernel runs on kfmi_text.h's frame: one lane per task, the read in
 * registers (text_task), the text window paths_kernel loads (the same c,
 * BandWindow and under_group_mask; it covers [B, end) because status OK means
 * B - c <= w and end <= c + m + w), loaded only for mapped lines with D > 0 --
 * MD needs a text letter under X and D alone.  The lines of a wave's 64 tasks
 * are one contiguous byte range of the output, so the wave formats them into a
 * 16 KB tile of LDS and copies the tile out with 16-byte stores:
 *
 *   a round takes the longest prefix of the wave's remaining lines that ends
 *   at or below origin + 16 KB, origin = base & ~15 with base the first
 *   remaining line's offset -- one ballot; the tile is filled from base & 15
 *   on, so that LDS and global alignment agree; the ragged head and tail go out
 *   as bytes, everything between as uint4.
 *
 * A line is at most KFMI_SAM_LINE_MAX bytes (kfmi_sam.h derives it), so the
 * first remaining line always fits and a round makes progress.  The tiles lie
 * over the staging area, which text_task leaves behind a block barrier; from
 * there on only wave-level synchronisation is used, since the waves of a block
 * take different numbers of rounds.  kfmi_set_sam_form(1) keeps the plain form
 * for comparison: every lane writes its line straight to device memory.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "kfmi_text.h"

#define KFMI_SAM_TEXT(src, p) ((src).text_code(p))
#include "../kfmi_sam.h"

namespace kfmi {

static constexpr uint32_t SAM_TILE = 16384u;   /* bytes of LDS per wave */
static_assert(KFMI_SAM_LINE_MAX + 15u <= SAM_TILE, "the first remaining line of a round must fit the tile");

struct SamArgs {
  const uint2* __restrict__ hits;        /* one record per task; x is read */
  const uint2* __restrict__ paths;       /* one record per task */
  const uint2* __restrict__ quals;       /* one record per task, or nullptr */
  const uint32_t* __restrict__ cigars;   /* 2C words per task */
  kfmi_sam_table tab;
  uint32_t* info;                        /* tasks + 1 words: KFMI_SAM_LEN_MASK .. of kfmi_sam.h */
  const uint64_t* off;                   /* tasks + 1: where each task's line begins */
  uint8_t* out;
  uint64_t tasks, name_base;
  uint32_t n, m, band, C, options, strands;
};

__global__ __launch_bounds__(256) void sam_length_kernel(SamArgs a)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  const bool has = t < a.tasks;   /* BOTH: tasks is even, so lane ^ 1 has a task iff this one has */
  const int both = a.strands == KFMI_STRAND_BOTH;
  const int rev = a.strands == KFMI_STRAND_REV || (both && (t & 1u));
  uint32_t st = KFMI_SAM_NONE, d = 0u, contig = 0u, B = 0u;
  kfmi_sam_runs walk = {0u, 0u, 0u, 0u, 0u};
  if (has) {
    const uint2 p = a.paths[t];
    B = a.hits[t].x;
    d = p.y & KFMI_PATH_EDITS_MASK;
    st = kfmi_sam_status(&a.tab, a.n, a.m, a.band, a.C, a.options, B, p.x, p.y, a.cigars + 2ull * a.C * t, &contig,
                         &walk);
  }
  const uint32_t mst = (uint32_t) __shfl_xor((int) st, 1), md = (uint32_t) __shfl_xor((int) d, 1);
  uint32_t info = 0u;
  if (has) {
    const uint64_t qname = a.name_base + (both ? t >> 1 : t);
    const uint32_t choice = kfmi_sam_choice(both, rev, st, d, mst, md);
    if (choice & KFMI_SAM_MAPPED) {
      const uint32_t q0 = a.quals ? a.quals[t].x : 0u;
      info = choice | kfmi_sam_mapped_len(&a.tab, contig, qname, rev, B, kfmi_sam_mapq(a.quals != nullptr, q0), a.m, d,
                                          &walk);
    } else if (choice) {
      info = choice | kfmi_sam_unmapped_len(qname, a.m);
    }
  }
  if (t <= a.tasks) a.info[t] = info;   /* word `tasks` is 0: the scan's last element is the total */
}

/* the text's codes from the lane's window: tx[j] is word w0 + j - 1 of the text's stream, which holds text base
 * n - 1 - g at bits 2g; a select over the words, so that they stay in registers */
template <int MAXW>
struct WindowText {
  const uint32_t (&tx)[MAXW + 3];
  uint32_t w0, n;
  __device__ __forceinline__ uint32_t text_code(uint32_t p) const
  {
    const uint32_t g = n - 1u - p, j = (g >> 4) + 1u - w0;
    uint32_t word = 0u;
#pragma unroll
    for (int k = 0; k < MAXW + 3; ++k) word = j == (uint32_t) k ? tx[k] : word;
    return (word >> (2u * (g & 15u))) & 3u;
  }
};

/* SEQ from the lane's code words, which hold read base m - 1 - r at bits 2r: as aligned, or -- flip -- the reverse
 * complement, base for base from r = 0 up.  The words are indexed by unrolled loops alone. */
template <int MAXW>
__device__ __forceinline__ uint32_t put_seq(uint8_t* dst, uint32_t pos, const uint32_t (&cw)[MAXW], uint32_t m, bool flip)
{
  const uint32_t nw = (m + 15u) >> 4;
  if (!flip) {
#pragma unroll
    for (int j = MAXW - 1; j >= 0; --j)
      if ((uint32_t) j < nw) {
        const uint32_t c = cw[j], cnt = m - 16u * (uint32_t) j < 16u ? m - 16u * (uint32_t) j : 16u;
KFMI_SAM_ROLLED
        for (uint32_t r = cnt; r-- > 0u;) dst[pos++] = kfmi_sam_letter(c >> (2u * r));
      }
  } else {
#pragma unroll
    for (int j = 0; j < MAXW; ++j)
      if ((uint32_t) j < nw) {
        const uint32_t c = ~cw[j], cnt = m - 16u * (uint32_t) j < 16u ? m - 16u * (uint32_t) j : 16u;
KFMI_SAM_ROLLED
        for (uint32_t r = 0; r < cnt; ++r) dst[pos++] = kfmi_sam_letter(c >> (2u * r));
      }
  }
  return pos;
}

/* the lanes of a wave see each other's LDS bytes after it: every earlier access has completed, none moves across */
__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MAXW, bool STR, bool TILED>
__global__ __launch_bounds__(256) void sam_write_kernel(SamArgs a, TextArgs ta)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint32_t cw[MAXW];
  uint64_t t;
  const bool has = text_task<MAXW, STR>(ta.ascii, ta.num, ta.m, ta.strands, lds, cw, t);   /* ends in a block barrier */
  const uint32_t m = ta.m, n = ta.n, w = a.band;
  const int both = a.strands == KFMI_STRAND_BOTH;
  const int rev = a.strands == KFMI_STRAND_REV || (both && (t & 1u));
  const uint32_t info = has ? a.info[t] : 0u;
  const uint32_t len = info & KFMI_SAM_LEN_MASK;
  const uint64_t off = has ? a.off[t] : 0ull, end = off + len;
  const bool mapped = (info & KFMI_SAM_MAPPED) != 0u;
  const uint2 path = mapped ? a.paths[t] : make_uint2(0u, 0u);
  const uint32_t B = mapped ? a.hits[t].x : 0u;
  const uint32_t d = path.y & KFMI_PATH_EDITS_MASK;
  const bool sc = mapped && d != 0u;                       /* only X and D ask for a text letter */
  const uint32_t c = sc ? (B < n - m ? B : n - m) : 0u;   /* mapped: n >= m, B <= n, B - c <= w (kfmi_sam_status) */
  BandWindow<MAXW> win(sc, sc ? n - c - m : 0u, m, w, n);
  under_group_mask(ta.split4, lane_group(), [&] { win.load(ta.text); });
  const WindowText<MAXW> src{win.tx, win.w0, n};
  const uint64_t qname = a.name_base + (both ? t >> 1 : t);
  const uint32_t* cig = a.cigars + 2ull * a.C * t;

  auto format = [&](uint8_t* dst, uint32_t pos) {
    if (mapped) {
      const uint32_t runs = (path.y >> KFMI_PATH_RUNS_SHIFT) & KFMI_PATH_RUNS_MASK;
      const uint32_t q0 = a.quals ? a.quals[t].x : 0u;
      pos = kfmi_sam_put_front(dst, pos, &a.tab, kfmi_sam_contig(&a.tab, B, path.x), qname, rev, B,
                               kfmi_sam_mapq(a.quals != nullptr, q0), cig, runs, a.options);
      pos = put_seq<MAXW>(dst, pos, cw, m, false);
      (void) kfmi_sam_put_back(dst, pos, d, cig, runs, B, src);
    } else {   /* the read as given: a REV-only lane holds P' */
      pos = kfmi_sam_put_unmapped_front(dst, pos, qname);
      pos = put_seq<MAXW>(dst, pos, cw, m, a.strands == KFMI_STRAND_REV);
      (void) kfmi_sam_put_unmapped_back(dst, pos, info >> KFMI_SAM_CODE_SHIFT);
    }
  };

  if constexpr (!TILED) {
    if (len) format(a.out + off, 0u);
  } else {
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t* tile = lds + (threadIdx.x >> 6) * SAM_TILE;
    bool todo = len != 0u;
    for (;;) {
      const uint64_t live = __ballot(todo);
      if (!live) break;
      const uint64_t base = __shfl((unsigned long long) off, __ffsll((unsigned long long) live) - 1);
      const uint64_t origin = base & ~15ull;   /* tile byte k is output byte origin + k */
      const bool take = todo && end - origin <= SAM_TILE;   /* ends ascend with the lane: a prefix of the live lanes */
      const uint64_t took = __ballot(take);                 /* never empty: base - origin + KFMI_SAM_LINE_MAX fits */
      if (!took) break;
      const uint64_t rend = __shfl((unsigned long long) end, 63 - __clzll((long long) took));
      if (take) {
        format(tile, (uint32_t) (off - origin));
        todo = false;
      }
      wave_sync();
      const uint64_t a0 = ((base + 15u) & ~15ull) < rend ? (base + 15u) & ~15ull : rend;
      const uint64_t a1 = (rend & ~15ull) > a0 ? rend & ~15ull : a0;
KFMI_SAM_ROLLED
      for (uint64_t g = base + lane; g < a0; g += 64u) a.out[g] = tile[g - origin];
KFMI_SAM_ROLLED
      for (uint64_t g = a0 + 16u * lane; g < a1; g += 1024u)
        *reinterpret_cast<uint4*>(a.out + g) = *reinterpret_cast<const uint4*>(tile + (g - origin));
KFMI_SAM_ROLLED
      for (uint64_t g = a1 + lane; g < rend; g += 64u) a.out[g] = tile[g - origin];
      wave_sync();
    }
  }
}

static std::atomic<uint32_t> g_sam_form{0};   /* kfmi_set_sam_form: 0 = the tile, 1 = a lane writes its line */
static thread_local double t_sam_ms[3] = {0.0, 0.0, 0.0};

extern "C" int32_t kfmi_set_sam_form(uint32_t form)
{
  if (form > 1u) return KFMI_E_BAD_ARGUMENT;
  g_sam_form.store(form, std::memory_order_relaxed);
  return KFMI_SUCCESS;
}

extern "C" int32_t kfmi_sam_last_passes(double* ms_length, double* ms_scan, double* ms_write)
{
  if (ms_length) *ms_length = t_sam_ms[0];
  if (ms_scan) *ms_scan = t_sam_ms[1];
  if (ms_write) *ms_write = t_sam_ms[2];
  return KFMI_SUCCESS;
}

static hipError_t launch_write(const SamArgs& a, const TextArgs& ta, bool tiled, hipStream_t st)
{
  return launch_text(ta.m, ta.strands, a.tasks, st, [&](auto W, auto S, dim3 grid, size_t stage) {
    constexpr int MW = decltype(W)::value;
    constexpr bool STR = decltype(S)::value;
    if (tiled) {
      const size_t lds = stage > 4u * SAM_TILE ? stage : 4u * SAM_TILE;   /* the tiles lie over the staging area */
      hipLaunchKernelGGL((sam_write_kernel<MW, STR, true>), grid, dim3(256), lds, st, a, ta);
    } else {
      hipLaunchKernelGGL((sam_write_kernel<MW, STR, false>), grid, dim3(256), stage, st, a, ta);
    }
  });
}

/* device memory of a handle or a table, freed on its device whatever the caller's current device is */
static void free_on(void* p, int32_t device)
{
  DeviceGuard dg;
  if (hipSetDevice(device) == hipSuccess) (void) hipFree(p);
  (void) hipGetLastError();
}

static int32_t fetch_from(const void* d_text, int32_t device, char* dst, uint64_t bytes)
{
  DeviceGuard dg;
  if (hipSetDevice(device) != hipSuccess || hipMemcpy(dst, d_text, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    (void) hipGetLastError();
    return KFMI_E_KERNEL;
  }
  return KFMI_SUCCESS;
}

/* The table's device copy [begins | lengths | name_off | names], made once on `device` (which is current). */
static int32_t contigs_on_device(kfmi_contigs_t* c, int device, kfmi_sam_table* tab)
{
  const uint64_t cnt = c->count, nb = c->name_off[cnt];
  int32_t err = KFMI_SUCCESS;
  pthread_mutex_lock(&c->mu);
  if (c->d_mem && c->d_device != device) err = KFMI_E_BAD_ARGUMENT;
  if (!err && !c->d_mem) {
    uint8_t* p = nullptr;
    if (hipMalloc((void**) &p, 12 * cnt + 4 + nb + 4) != hipSuccess) {
      (void) hipGetLastError();
      err = KFMI_E_DEVICE_ALLOC;
    } else if (hipMemcpy(p, c->begins, 4 * cnt, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(p + 4 * cnt, c->lengths, 4 * cnt, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(p + 8 * cnt, c->name_off, 4 * cnt + 4, hipMemcpyHostToDevice) != hipSuccess ||
               (nb && hipMemcpy(p + 12 * cnt + 4, c->names, nb, hipMemcpyHostToDevice) != hipSuccess)) {
      (void) hipGetLastError();
      (void) hipFree(p);
      err = KFMI_E_KERNEL;
    } else {
      c->d_mem = p;
      c->d_device = device;
      c->d_free = free_on;
    }
  }
  if (!err) {
    const uint8_t* p = (const uint8_t*) c->d_mem;
    tab->begins = reinterpret_cast<const uint32_t*>(p);
    tab->lengths = reinterpret_cast<const uint32_t*>(p + 4 * cnt);
    tab->name_off = reinterpret_cast<const uint32_t*>(p + 8 * cnt);
    tab->names = p + 12 * cnt + 4;
    tab->count = c->count;
  }
  pthread_mutex_unlock(&c->mu);
  return err;
}

struct LenOf {   /* the scan's input: a task's bytes */
  __host__ __device__ uint64_t operator()(uint32_t v) const { return v & KFMI_SAM_LEN_MASK; }
};

extern "C" int32_t kfmi_sam_lines(void* index, void* queries, void* contigs, void* hits, void* paths, void* cigars,
                                  void* quals, uint32_t strands, uint32_t cigar_entries, uint32_t band,
                                  uint32_t options, uint64_t name_base, void** sam)
{
  const uint32_t C = cigar_entries;
  if (band > KFMI_ALIGN_MAX_BAND || C < 1 || C > KFMI_PATH_MAX_ENTRIES) return KFMI_E_BAD_ARGUMENT;
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (options & ~KFMI_SAM_CIGAR_M) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_contigs_t* ct = (kfmi_contigs_t*) contigs;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  kfmi_res_t* rp = (kfmi_res_t*) paths;
  kfmi_res_t* rc = (kfmi_res_t*) cigars;
  kfmi_res_t* rq = (kfmi_res_t*) quals;
  if (!f || !q || !ct || !sam || !rh || !rp || !rc || rp == rh || rc == rh || rc == rp) return KFMI_E_BAD_ARGUMENT;
  if (rq && (rq == rh || rq == rp || rq == rc)) return KFMI_E_BAD_ARGUMENT;
  const uint32_t ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  const uint64_t tasks = ns * q->num;
  if (rh->num != tasks || rp->num != tasks || rc->num != tasks * C || (rq && rq->num != tasks))
    return KFMI_E_BAD_ARGUMENT;
  if (q->size < 1 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  if (name_base + q->num < name_base) return KFMI_E_BAD_ARGUMENT;
  if (f->bwtsize == 0 || (uint64_t) ct->begins[ct->count - 1] + ct->lengths[ct->count - 1] > f->bwtsize - 1u)
    return KFMI_E_BAD_ARGUMENT;
  TextCall c;
  int32_t err = rq ? c.open(f, q, {rh, rp, rc, rq}) : c.open(f, q, {rh, rp, rc});
  if (err) return err;
  SamArgs a{};
  if ((err = contigs_on_device(ct, c.di->device, &a.tab))) return err;
  const TextArgs ta = c.args(strands);
  a.hits = reinterpret_cast<const uint2*>(rh->d_results);
  a.paths = reinterpret_cast<const uint2*>(rp->d_results);
  a.quals = rq ? reinterpret_cast<const uint2*>(rq->d_results) : nullptr;
  a.cigars = rc->d_results;
  a.tasks = tasks;
  a.name_base = name_base;
  a.n = ta.n;
  a.m = ta.m;
  a.band = band;
  a.C = C;
  a.options = options;
  a.strands = strands;
  kfmi_sam_t* s = kfmi_sam_alloc(q->num);
  uint64_t* h_task_off = ns == 2u ? (uint64_t*) malloc(8 * (tasks + 1)) : nullptr;
  DeviceScratch info, off, tmp;
  uint8_t* d_text = nullptr;
  auto fail = [&](int32_t code) {
    if (d_text) (void) hipFree(d_text);
    free(h_task_off);
    if (s) kfmi_sam_free((void**) &s);
    return code;
  };
  if (!s || (ns == 2u && !h_task_off)) return fail(KFMI_E_ALLOCATING_RESULTS);
  const hipStream_t st = c.l.st;
  hipEvent_t* ev = c.l.ev;
  size_t tb = 0;
  if ((err = info.alloc(4 * (tasks + 1))) || (err = off.alloc(8 * (tasks + 1)))) return fail(err);
  const auto lens = rocprim::make_transform_iterator((const uint32_t*) info.p, LenOf{});
  uint64_t* d_off = reinterpret_cast<uint64_t*>(off.p);
  if (rocprim::exclusive_scan(nullptr, tb, lens, d_off, (uint64_t) 0, (size_t) (tasks + 1), rocprim::plus<uint64_t>(),
                              st) != hipSuccess)
    return fail(KFMI_E_KERNEL);
  if ((err = tmp.alloc(tb ? tb : 1))) return fail(err);
  a.info = info.p;
  a.off = d_off;
  uint64_t total = 0;
  bool ok = hipEventRecord(ev[0], st) == hipSuccess;
  hipLaunchKernelGGL(sam_length_kernel, dim3((uint32_t) ((tasks + 1 + 255) / 256)), dim3(256), 0, st, a);
  ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev[1], st) == hipSuccess &&
       rocprim::exclusive_scan(tmp.p, tb, lens, d_off, (uint64_t) 0, (size_t) (tasks + 1), rocprim::plus<uint64_t>(),
                               st) == hipSuccess &&
       hipEventRecord(ev[2], st) == hipSuccess &&
       hipMemcpyAsync(&total, d_off + tasks, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipStreamSynchronize(st) == hipSuccess;
  float ms_len = 0, ms_scan = 0, ms_write = 0;
  ok = ok && hipEventElapsedTime(&ms_len, ev[0], ev[1]) == hipSuccess &&
       hipEventElapsedTime(&ms_scan, ev[1], ev[2]) == hipSuccess;
  if (!ok) {
    fprintf(stderr, "kstepfmi: sam_length_kernel or its scan failed: %s\n", hipGetErrorString(hipGetLastError()));
    return fail(KFMI_E_KERNEL);
  }
  if (hipMalloc((void**) &d_text, total ? total : 1) != hipSuccess) {
    (void) hipGetLastError();
    d_text = nullptr;
    return fail(KFMI_E_DEVICE_ALLOC);
  }
  a.out = d_text;
  hipError_t he = hipSuccess;
  ok = hipEventRecord(ev[0], st) == hipSuccess;
  if (ok && tasks) he = launch_write(a, ta, g_sam_form.load(std::memory_order_relaxed) == 0u, st);
  uint64_t* h_dst = ns == 2u ? h_task_off : s->h_off;
  ok = ok && hipEventRecord(ev[1], st) == hipSuccess &&
       hipMemcpyAsync(h_dst, d_off, 8 * (tasks + 1), hipMemcpyDeviceToHost, st) == hipSuccess;
  ok = hipStreamSynchronize(st) == hipSuccess && ok;   /* waits for what was queued, whatever `he` says */
  ok = ok && hipEventElapsedTime(&ms_write, ev[0], ev[1]) == hipSuccess;
  if (he != hipSuccess || !ok) return fail(launch_result(KFMI_E_KERNEL, he, "sam_write_kernel"));
  if (ns == 2u) {   /* the loser of a read writes nothing, so the read's line begins where its FWD task's does */
    for (uint64_t i = 0; i < q->num; ++i) s->h_off[i] = h_task_off[2 * i];
    s->h_off[q->num] = h_task_off[tasks];
    free(h_task_off);
    h_task_off = nullptr;
  }
  s->bytes = total;
  s->d_text = d_text;
  s->d_device = c.di->device;
  s->d_fetch = fetch_from;
  s->d_free = free_on;
  t_sam_ms[0] = ms_len;
  t_sam_ms[1] = ms_scan;
  t_sam_ms[2] = ms_write;
  t_ms[0] = t_ms[2] = (double) ms_len + ms_scan + ms_write;
  t_ms[1] = 0.0;
  *sam = s;
  return KFMI_SUCCESS;
}

}  // namespace kfmi
