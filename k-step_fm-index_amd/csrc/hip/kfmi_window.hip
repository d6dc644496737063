/*
 * kfmi_window.hip -- window placement and pairing: the best unbanded
 * semi-global placement of every task among the begin positions of a text
 * window, the window each task's mate implies, and one placement per read
 * chosen per pair (kstep_fmi.h section 2, "place windows / pairs"; DESIGN.md
 * 5l; not in the reference, which stops at intervals).
 *
 * window_kernel's frame is kfmi_text.h's: one lane per task, the read in
 * registers -- REV tasks get P' from the strand staging -- over the text's word
 * stream, which holds text base n - 1 - g at bits 2 g.
 * A task has no candidates: it scans the text from its scan end T - 1 down to
 * the window's first position lo, which in the stream is the bases n - T up to
 * n - 1 - lo, consecutive dwords walked upwards.  Every load is one dword at
 * its own 4-byte alignment, never wider, with the next dword in flight while
 * the 16 bases of one are consumed; where the tables are past the translation
 * reach a lane's loads go out under its 16-lane group's mask
 * (word_at below).  Every word index is at most (n - 1) / 16, inside the stream.
 *
 * The score is the multi-word bit-vector column step of kfmi_window_dp.h with
 * the number of 32-cell words a compile-time constant (1, 2, 4 or 8 for reads
 * of up to 32, 64, 128 and 256 bases): the match and delta words are indexed
 * by constants alone and stay in registers.  Lanes of a wave loop to the wave's
 * longest scan; lanes with nothing to scan skip the loop.
 *
 * A window longer than KFMI_WINDOW_MAX_LEN refuses the whole call.  That is
 * decided on the device, so that windows kfmi_mate_windows left there never
 * visit the host: window_check_kernel runs first on the same stream and raises
 * a flag word, window_kernel reads the flag before it writes anything and
 * leaves at once when it is raised, and the host reads the flag after the one
 * wait of the call.
 *
 * mate_kernel and pair_kernel are streaming kernels over the records, one
 * lane per task and per pair, on the arithmetic of kfmi_pairs.h.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kfmi_pairs.h"
#include "kfmi_text.h"
#include "kfmi_window_dp.h"

namespace kfmi {

struct WindowArgs : TextArgs {
  const uint2* __restrict__ win;       /* one (lo, len) per task */
  uint2* __restrict__ hits;            /* one record per task */
  const uint32_t* __restrict__ flag;   /* raised by window_check_kernel: some len is too large */
  uint32_t max_edits;
};

__global__ __launch_bounds__(256) void window_check_kernel(const uint2* __restrict__ win, uint64_t tasks,
                                                            uint32_t* __restrict__ flag)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t < tasks && win[t].y > KFMI_WINDOW_MAX_LEN) *flag = 1u;   /* every writer writes the same value */
}

/* NW: 32-cell words per column; MAXW: the stagers' code words (8 | 16); STR: the strand staging, else forward reads */
template <int NW, int MAXW, bool STR>
__global__ __launch_bounds__(256) void window_kernel(WindowArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  uint64_t t;
  if (!text_task<MAXW, STR>(a.ascii, a.num, a.m, a.strands, stage, cw, t)) return;
  if (*a.flag) return;   /* a refused call writes nothing */
  const uint32_t m = a.m, n = a.n;
  const int grp = lane_group();
  /* Word x of the stream, under the lane's 16-lane group's mask where split4 (wave-uniform) says so.  The kernel's own
   * text and not under_group_mask: its rolled loop of turns around this one load, once per 16 columns of a scan bound
   * by integer issue, cost 7 % of the kernel's time at scale. */
  auto word_at = [&](uint32_t x) {
    uint32_t v = 0u;
    if (a.split4) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (grp == q) v = a.text[x];
    } else {
      v = a.text[x];
    }
    return v;
  };
  const uint2 wn = a.win[t];
  uint32_t hi_b = 0u, T = 0u;
  const int any = window_scan(n, wn.x, wn.y, m, a.max_edits, &hi_b, &T);
  uint32_t E = 0xFFFFFFFFu, bmin = 0u, bmax = 0u;
  if (any) {
    uint32_t peq[4][NW], pv[NW], mv[NW];
    window_match_words<NW, MAXW>(cw, m, peq);
    window_first_column<NW>(pv, mv);
    uint32_t score = m;
    if (hi_b == n) window_fold(score, n, E, bmin, bmax);   /* T = n: the first column is e(n) = m */
    /* text positions T - 1 down to lo are the stream's bases g = n - T up to gl = n - 1 - lo; none when T = lo */
    uint32_t g = n - T;
    const uint32_t gend = n - wn.x;          /* one past gl */
    if (g < gend) {
      const uint32_t xl = (gend - 1u) >> 4;  /* the last word the scan reads: <= (n - 1) / 16 */
      uint32_t word = word_at(g >> 4);
      uint32_t next = (g >> 4) < xl ? word_at((g >> 4) + 1u) : 0u;
      while (g < gend) {
        const uint32_t c = (word >> (2u * (g & 15u))) & 3u;
        score += (uint32_t) window_step<NW>(peq, pv, mv, m, c);
        const uint32_t j = n - 1u - g;
        if (j <= hi_b) window_fold(score, j, E, bmin, bmax);
        ++g;
        if ((g & 15u) == 0u && g < gend) {
          word = next;
          if ((g >> 4) < xl) next = word_at((g >> 4) + 1u);
        }
      }
    }
  }
  uint2 rec;
  window_record(any, E, bmin, bmax, a.max_edits, &rec.x, &rec.y);
  a.hits[t] = rec;
}

static hipError_t launch_window(const WindowArgs& a, uint64_t tasks, hipStream_t st)
{
  return launch_text(a.m, a.strands, tasks, st, [&](auto W, auto S, dim3 grid, size_t lds) {
    auto cells = [&](auto NW) {
      hipLaunchKernelGGL((window_kernel<decltype(NW)::value, decltype(W)::value, decltype(S)::value>), grid, dim3(256),
                         lds, st, a);
    };
    if constexpr (decltype(W)::value == 16) cells(std::integral_constant<int, 8>{});
    else if (a.m <= 32) cells(std::integral_constant<int, 1>{});
    else if (a.m <= 64) cells(std::integral_constant<int, 2>{});
    else cells(std::integral_constant<int, 4>{});
  });
}

extern "C" int32_t kfmi_place_windows(void* index, void* queries, void* windows, void* hits, uint32_t strands,
                                      uint32_t max_edits)
{
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* rw = (kfmi_res_t*) windows;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  if (!f || !q || !rw || !rh || rw == rh) return KFMI_E_BAD_ARGUMENT;
  const uint64_t tasks = (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num;
  if (rw->num != tasks || rh->num != tasks) return KFMI_E_BAD_ARGUMENT;
  if (q->size < 1 || q->size > 256) return KFMI_E_BAD_ARGUMENT;
  TextCall c;
  int32_t err = c.open(f, q, {rw, rh});
  if (err) return err;
  if (!tasks) {
    err = c.begin();
    return err ? err : c.finish();
  }
  DeviceScratch flag;
  if ((err = flag.alloc(sizeof(uint32_t)))) return err;
  WindowArgs a{c.args(strands)};
  a.win = reinterpret_cast<const uint2*>(rw->d_results);
  a.hits = reinterpret_cast<uint2*>(rh->d_results);
  a.flag = flag.p;
  a.max_edits = max_edits;
  uint32_t raised = 0u;
  hipError_t he = hipMemsetAsync(flag.p, 0, sizeof(uint32_t), c.l.st);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(window_check_kernel, dim3((uint32_t) ((tasks + 255) / 256)), dim3(256), 0, c.l.st, a.win, tasks,
                       flag.p);
    he = hipGetLastError();
  }
  err = c.begin();   /* the timing is the window kernel's */
  if (!err && he == hipSuccess) he = launch_window(a, tasks, c.l.st);
  if (!err) err = c.finish();   /* waits for whatever was queued */
  if (!err && he == hipSuccess) he = hipMemcpy(&raised, flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost);
  err = launch_result(err, he, "window_kernel");
  if (err) return err;
  return raised ? KFMI_E_BAD_ARGUMENT : KFMI_SUCCESS;
}

__global__ __launch_bounds__(256) void mate_kernel(const uint32_t* __restrict__ hits, uint32_t* __restrict__ win,
                                                    uint64_t tasks, uint64_t n, uint32_t m, uint32_t min_frag,
                                                    uint32_t max_frag, uint32_t mode)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= tasks) return;   /* tasks % 4 == 0: t ^ 3 is a task too */
  const uint2 own = reinterpret_cast<const uint2*>(hits)[t], mate = reinterpret_cast<const uint2*>(hits)[t ^ 3u];
  const uint32_t o[2] = {own.x, own.y}, u[2] = {mate.x, mate.y};
  uint32_t w[2];
  kfmi_mate_window((uint32_t) (t & 3u), o, u, n, m, min_frag, max_frag, mode, w);
  reinterpret_cast<uint2*>(win)[t] = make_uint2(w[0], w[1]);
}

__global__ __launch_bounds__(256) void pair_kernel(const uint32_t* __restrict__ hits, const uint32_t* __restrict__ resc,
                                                    uint32_t* __restrict__ paired, uint64_t pairs, uint32_t m,
                                                    uint32_t min_frag, uint32_t max_frag)
{
  const uint64_t p = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (p >= pairs) return;
  uint32_t h[8], r[8], out[8];
  /* a pair's records are 32 bytes at a 32-byte offset of a hipMalloc'd array: two 16-byte loads each */
  const uint4* hp = reinterpret_cast<const uint4*>(hits) + 2 * p;
  const uint4* rp = reinterpret_cast<const uint4*>(resc) + 2 * p;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint4 x = hp[i], y = rp[i];
    h[4 * i] = x.x; h[4 * i + 1] = x.y; h[4 * i + 2] = x.z; h[4 * i + 3] = x.w;
    r[4 * i] = y.x; r[4 * i + 1] = y.y; r[4 * i + 2] = y.z; r[4 * i + 3] = y.w;
  }
  kfmi_pair_choice(h, r, m, min_frag, max_frag, out);
  uint4* op = reinterpret_cast<uint4*>(paired) + 2 * p;
  op[0] = make_uint4(out[0], out[1], out[2], out[3]);
  op[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

extern "C" int32_t kfmi_mate_windows(void* index, void* hits, void* windows, uint32_t read_len, uint32_t min_frag,
                                     uint32_t max_frag, uint32_t mode)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  kfmi_res_t* rw = (kfmi_res_t*) windows;
  if (!f || !rh || !rw || rh == rw || rh->num != rw->num || mode > 1u) return KFMI_E_BAD_ARGUMENT;
  int32_t err = kfmi_pair_args(rh->num, read_len, min_frag, max_frag);
  if (err) return err;
  RecordCall c;
  err = c.open(f, {rh, rw});
  if (err) return err;
  err = c.begin();
  if (err) return err;
  if (rh->num) {
    hipLaunchKernelGGL(mate_kernel, dim3((uint32_t) ((rh->num + 255) / 256)), dim3(256), 0, c.l.st, rh->d_results,
                       rw->d_results, rh->num, (uint64_t) c.di->bwtsize - 1u, read_len, min_frag, max_frag, mode);
    HIP_OK(hipGetLastError());
  }
  return c.finish();
}

extern "C" int32_t kfmi_pair_hits(void* index, void* hits, void* rescued, void* paired, uint32_t read_len,
                                  uint32_t min_frag, uint32_t max_frag)
{
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_res_t* rh = (kfmi_res_t*) hits;
  kfmi_res_t* rr = (kfmi_res_t*) rescued;
  kfmi_res_t* rp = (kfmi_res_t*) paired;
  if (!f || !rh || !rr || !rp || rp == rh || rp == rr || rh == rr || rh->num != rr->num || rh->num != rp->num)
    return KFMI_E_BAD_ARGUMENT;
  int32_t err = kfmi_pair_args(rh->num, read_len, min_frag, max_frag);
  if (err) return err;
  RecordCall c;
  err = c.open(f, {rh, rr, rp});
  if (err) return err;
  err = c.begin();
  if (err) return err;
  if (rh->num) {
    const uint64_t pairs = rh->num / 4;
    hipLaunchKernelGGL(pair_kernel, dim3((uint32_t) ((pairs + 255) / 256)), dim3(256), 0, c.l.st, rh->d_results,
                       rr->d_results, rp->d_results, pairs, read_len, min_frag, max_frag);
    HIP_OK(hipGetLastError());
  }
  return c.finish();
}

}  // namespace kfmi
