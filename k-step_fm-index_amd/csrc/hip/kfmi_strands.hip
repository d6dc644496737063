/*
 * kfmi_strands.hip -- searching the reverse strand of every read, or both
 * strands, without a second copy of the reads crossing PCIe (kstep_fmi.h
 * section 2; not in the reference, which searches a read as
 * written).
 *
 * A search of ns strands runs ns * num tasks: in BOTH, task t is read t >> 1
 * on strand t & 1 and its interval goes to res + 2t, so every slice of reads
 * is a contiguous slice of results.  Where the launch plan (kfmi_plan.h) says
 * so, either strand is packed inside the search kernel (task_strands_kernel,
 * kfmi_kernels.h).  Everything else runs the forward LF kernels on ns * num
 * columns of code words; only the words differ.  Three kernels write those
 * task columns on the device:
 *   pack_strands_rows_kernel  from the ASCII reads, whole rows in registers
 *                             (m <= 256, m % K == 0, 16 bases per word)
 *   pack_strands_kernel       from the ASCII reads, any K and m (a mirrored
 *                             index and ^ 3)
 *   strand_words_kernel       from forward code words alone (host-packed
 *                             uploads and stream chunks)
 * the first and the last by the identity of kfmi_strands.h.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <shared_mutex>

#include "../kfmi_internal.h"
#include "kfmi_device.h"
#include "kfmi_runtime.h"
#include "kfmi_strands.h"

namespace kfmi {

/* strands_trace_one<K, NB, LAY> is compiled in kfmi_inst_trace_seeds_*.hip */
KFMI_FOR_LANE_GEOMETRIES(KFMI_SEEDS_TRACE_EXTERN)

hipError_t dispatch_strands_trace(uint32_t K, uint32_t nb, int lay, const SearchLaunch& a)
{
#define KFMI_CASE(KK, NBV, LAYV) \
  if (K == KK && nb == NBV && lay == LAYV) return strands_trace_one<KK, NBV, LAYV>(a);
  KFMI_FOR_LANE_GEOMETRIES(KFMI_CASE)
#undef KFMI_CASE
  return hipErrorInvalidValue;
}

/* ASCII [num][m] -> code words of the ns * num tasks, word w of task t at
 * out[w * ns * num + t] and the remainder codes in row nwords, the layout the
 * LF kernels read with ns * num queries.  A block takes tq reads, staged
 * HBM -> LDS in one contiguous piece when `staged` (reads of up to 1 KiB; longer
 * ones are read in place), and one thread converts each task: base j of a
 * reverse-strand task is base m-1-j of the read, complemented. */
template <int K>
__global__ __launch_bounds__(256) void pack_strands_kernel(const uint8_t* __restrict__ q, uint64_t num, uint32_t m,
                                                           uint32_t steps, uint32_t nwords, uint32_t tq,
                                                           uint32_t staged, uint32_t* __restrict__ out, uint32_t rem,
                                                           uint32_t strands)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
  constexpr int SPW = 32 / (2 * K);
  const uint32_t ns = strands == KFMI_STRAND_BOTH ? 2u : 1u;
  const uint64_t q0 = (uint64_t) blockIdx.x * tq;
  if (q0 >= num) return;
  const uint32_t nq = (uint32_t) ((num - q0) < tq ? (num - q0) : tq);
  if (staged) {
    const uint64_t bytes = (uint64_t) nq * m;
    const uint8_t* src = q + q0 * m;
    if ((((uintptr_t) src) & 15u) == 0) {
      const uint64_t n16 = bytes / 16;
      for (uint64_t i = threadIdx.x; i < n16; i += blockDim.x)
        reinterpret_cast<uint4*>(tile)[i] = reinterpret_cast<const uint4*>(src)[i];
      for (uint64_t i = n16 * 16 + threadIdx.x; i < bytes; i += blockDim.x) tile[i] = src[i];
    } else {
      for (uint64_t i = threadIdx.x; i < bytes; i += blockDim.x) tile[i] = src[i];
    }
    __syncthreads();
  }
  const uint64_t ncol = (uint64_t) ns * num;
  for (uint32_t tt = threadIdx.x; tt < nq * ns; tt += blockDim.x) {
    const uint32_t r = ns == 2u ? tt >> 1 : tt;
    const bool rev = ns == 2u ? (tt & 1u) != 0u : true;
    const uint8_t* p = staged ? tile + (uint64_t) r * m : q + (q0 + r) * m;
    const uint32_t cx = rev ? 3u : 0u;
    /* code of base j of this task's read */
    auto code = [&](uint32_t j) { return code_of(p[rev ? m - 1u - j : j]) ^ cx; };
    const uint64_t col = q0 * ns + tt;
    for (uint32_t w = 0; w < nwords; ++w) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < SPW; ++j) {
        const uint32_t st = w * SPW + j;
        if (st < steps) {
          const uint32_t pos = (m - rem) - 1u - K * st;
          uint32_t c = 0;
#pragma unroll
          for (int i = 0; i < K; ++i) c |= code(pos - i) << (2 * i);
          word |= c << (2 * K * j);
        }
      }
      out[(uint64_t) w * ncol + col] = word;
    }
    if (rem) {   /* remainder table index: the task's last rem bases, base m-1 at bits 0-1 */
      uint32_t c = 0;
      for (uint32_t u = 0; u < rem; ++u) c |= code(m - 1u - u) << (2 * u);
      out[(uint64_t) nwords * ncol + col] = c;
    }
  }
}

/* The same task columns for the common case -- reads of up to 16 * MAXW bases,
 * m % K == 0, 16 bases per word (K in {1, 2, 4}): one thread per read converts
 * its LDS row four bases at a time (row_codes, the fused packers' SWAR form)
 * and derives the reverse strand's words from the forward ones in registers,
 * S' = ~pairreverse_m(S) (kfmi_strands.h): the MAXW words reversed and
 * pair-reversed at fixed register indices, then the whole stream shifted down
 * by the wave-uniform 32 * MAXW - 2m bits (the all-ones pairs that the zero
 * words above base m-1 turn into leave at the bottom, zeros come in at the
 * top).  BOTH stores word w of either strand as one uint2. */
template <int MAXW>
__global__ __launch_bounds__(256) void pack_strands_rows_kernel(const uint8_t* __restrict__ q, uint64_t num, uint32_t m,
                                                                uint32_t nwords, uint32_t tq,
                                                                uint32_t* __restrict__ out, uint32_t strands)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t tile[];
  const uint64_t q0 = (uint64_t) blockIdx.x * tq;
  if (q0 >= num) return;
  const uint32_t nq = (uint32_t) ((num - q0) < tq ? (num - q0) : tq);
  {
    const uint64_t bytes = (uint64_t) nq * m;
    const uint8_t* src = q + q0 * m;
    if ((((uintptr_t) src) & 15u) == 0) {
      const uint64_t n16 = bytes / 16;
      for (uint64_t i = threadIdx.x; i < n16; i += blockDim.x)
        reinterpret_cast<uint4*>(tile)[i] = reinterpret_cast<const uint4*>(src)[i];
      for (uint64_t i = n16 * 16 + threadIdx.x; i < bytes; i += blockDim.x) tile[i] = src[i];
    } else {
      for (uint64_t i = threadIdx.x; i < bytes; i += blockDim.x) tile[i] = src[i];
    }
  }
  __syncthreads();
  const uint32_t r = threadIdx.x;   /* tq <= 256 = the block */
  if (r >= nq) return;
  uint32_t cw[MAXW];
  row_codes<MAXW>(tile, (uint64_t) r * m, m, cw);   /* reads at most 8 bytes past the row: inside the tile's slack */
  uint32_t rv[MAXW];
  reverse_stream<MAXW>(cw, m, rv);
  const uint64_t t = q0 + r;
  if (strands == KFMI_STRAND_BOTH) {
#pragma unroll
    for (int w = 0; w < MAXW; ++w)
      if ((uint32_t) w < nwords) *reinterpret_cast<uint2*>(out + (uint64_t) w * 2u * num + 2u * t) = make_uint2(cw[w], rv[w]);
  } else {
#pragma unroll
    for (int w = 0; w < MAXW; ++w)
      if ((uint32_t) w < nwords) out[(uint64_t) w * num + t] = rv[w];
  }
}

/* Forward code words [rows][n] (16 bases per word: K in {1, 2, 4}; row nwords
 * the remainder codes when rem) -> the words of the ns * n tasks, same rows.
 * One thread per task: a forward task copies its read's column, a reverse one
 * writes S' = ~pairreverse_m(S) word by word (kfmi_strands.h) and splits it
 * into remainder code and K-step stream again. */
__global__ __launch_bounds__(256) void strand_words_kernel(const uint32_t* __restrict__ in, uint64_t n, uint32_t m,
                                                           uint32_t nwords, uint32_t rem,
                                                           uint32_t* __restrict__ out, uint32_t strands)
{
  const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (strands == KFMI_STRAND_BOTH ? 2u : 1u) * n) return;
  strand_words_task(in, n, m, nwords, rem, out, strands, t);
}

/* Test accessor: strand_words_kernel's tasks on the host, the same code
 * (kfmi_strands.h), so a CPU test checks the identity against the host packer
 * on the reverse complement for every K, m and remainder. */
extern "C" int32_t kfmi_strand_words_host(const uint32_t* words, uint64_t num, uint32_t size, uint32_t k,
                                          uint32_t strands, uint32_t* out)
{
  if ((k != 1 && k != 2 && k != 4) || size == 0 || (strands != KFMI_STRAND_REV && strands != KFMI_STRAND_BOTH) ||
      ((!words || !out) && num))
    return KFMI_E_BAD_ARGUMENT;
  const uint32_t rem = size % k, nwords = (size - rem + 15u) / 16u;
  const uint64_t ntasks = (strands == KFMI_STRAND_BOTH ? 2u : 1u) * num;
  for (uint64_t t = 0; t < ntasks; ++t) strand_words_task(words, num, size, nwords, rem, out, strands, t);
  return KFMI_SUCCESS;
}

template <int MAXW>
static void reverse_stream_columns(const uint32_t* words, uint64_t num, uint32_t size, uint32_t* out)
{
  for (uint64_t c = 0; c < num; ++c) {
    uint32_t s[MAXW], rv[MAXW];
    for (int w = 0; w < MAXW; ++w) s[w] = words[(uint64_t) w * num + c];
    reverse_stream<MAXW>(s, size, rv);
    for (int w = 0; w < MAXW; ++w) out[(uint64_t) w * num + c] = rv[w];
  }
}

/* Test accessor: reverse_stream<maxw>, the register form that both ASCII-fed
 * device kernels (task_strands_kernel, pack_strands_rows_kernel) run, on the
 * host: column c of `words` ([maxw][num], 16 bases per word, zero above base
 * size-1) -> column c of `out`, same shape. */
extern "C" int32_t kfmi_reverse_stream_host(const uint32_t* words, uint64_t num, uint32_t size, uint32_t maxw,
                                            uint32_t* out)
{
  if ((maxw != 8 && maxw != 16) || size == 0 || size > 16u * maxw || ((!words || !out) && num))
    return KFMI_E_BAD_ARGUMENT;
  if (maxw == 8) reverse_stream_columns<8>(words, num, size, out);
  else reverse_stream_columns<16>(words, num, size, out);
  return KFMI_SUCCESS;
}

/* The task columns of dq's reads into `out` ((nwords + 1) x ns * num words),
 * queued on st: from the ASCII reads when the device has them, else from the
 * forward code words in dq->packed. */
hipError_t launch_strand_pack(const kfmi_dev_queries* dq, uint32_t* out, uint32_t strands, bool from_words,
                              hipStream_t st)
{
  if (dq->num == 0) return hipSuccess;
  if (!out) return hipErrorInvalidValue;
  const uint64_t ns = strands == KFMI_STRAND_BOTH ? 2 : 1;
  if (from_words || !dq->ascii) {
    if (dq->K == 3 || !dq->packed) return hipErrorInvalidValue;   /* no 15-base words from the host packer */
    const uint64_t blocks = (ns * dq->num + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(strand_words_kernel, dim3((uint32_t) blocks), dim3(256), 0, st, dq->packed, dq->num, dq->size,
                       dq->nwords, dq->rem, out, strands);
    return hipGetLastError();
  }
  if (dq->K != 3 && dq->rem == 0 && dq->size <= 256) {   /* the common case: whole rows in registers */
    uint32_t tr = 256;
    while ((uint64_t) tr * dq->size + 16 > 64 * 1024 && tr > 64) tr >>= 1;
    const uint64_t nblk = (dq->num + tr - 1) / tr;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const size_t lds_rows = (size_t) tr * dq->size + 16;   /* row_codes reads up to 8 bytes past a row */
    if (dq->size <= 128)
      hipLaunchKernelGGL((pack_strands_rows_kernel<8>), dim3((uint32_t) nblk), dim3(256), lds_rows, st, dq->ascii,
                         dq->num, dq->size, dq->nwords, tr, out, strands);
    else
      hipLaunchKernelGGL((pack_strands_rows_kernel<16>), dim3((uint32_t) nblk), dim3(256), lds_rows, st, dq->ascii,
                         dq->num, dq->size, dq->nwords, tr, out, strands);
    return hipGetLastError();
  }
  uint32_t tq = 256;
  while ((uint64_t) tq * dq->size > 64 * 1024 && tq > 64) tq >>= 1;
  const uint32_t staged = (uint64_t) tq * dq->size <= 64 * 1024 ? 1u : 0u;
  const uint64_t blocks = (dq->num + tq - 1) / tq;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const size_t lds = staged ? (size_t) tq * dq->size : 0;   /* <= 64 KiB */
  const dim3 grid((uint32_t) blocks);
#define KFMI_PS(KK)                                                                                              \
  hipLaunchKernelGGL((pack_strands_kernel<KK>), grid, dim3(256), lds, st, dq->ascii, dq->num, dq->size, dq->steps, \
                     dq->nwords, tq, staged, out, dq->rem, strands)
  if (dq->K == 1) KFMI_PS(1);
  else if (dq->K == 2) KFMI_PS(2);
  else if (dq->K == 3) KFMI_PS(3);
  else if (dq->K == 4) KFMI_PS(4);
  else return hipErrorInvalidValue;
#undef KFMI_PS
  return hipGetLastError();
}

/* dq->strand_words grown to the task columns of both strands of `cq` reads
 * (so a later call with another strand mode never replaces it), under the
 * device's upload lock: two searches of one handle may get here together. */
int32_t strand_reserve(kfmi_dev_queries* dq, uint64_t cq, DevCtx* ctx)
{
  const uint64_t need = 2ull * (dq->nwords + 1) * (cq ? cq : 1);
  std::lock_guard<std::mutex> lk(ctx->up_mu);
  if (dq->strand_cap >= need) return KFMI_SUCCESS;
  if (dq->strand_words) (void) hipFree(dq->strand_words);
  dq->strand_words = nullptr;
  dq->strand_cap = 0;
  if (hipMalloc((void**) &dq->strand_words, 4ull * need) != hipSuccess) {
    dq->strand_words = nullptr;
    return KFMI_E_DEVICE_ALLOC;
  }
  dq->strand_cap = need;
  return KFMI_SUCCESS;
}

extern "C" int32_t kfmi_search_strands(void* index, void* queries, void* results, uint32_t strands)
{
  if (strands < KFMI_STRAND_FWD || strands > KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  if (strands == KFMI_STRAND_FWD) return kfmi_search(index, queries, results);
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* r = (kfmi_res_t*) results;
  if (!f || !q || !r) return KFMI_E_BAD_ARGUMENT;
  const uint64_t ns = strands == KFMI_STRAND_BOTH ? 2 : 1;
  if (r->num != ns * q->num) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  const int32_t err = resident_single(f, q, {r});
  SearchWhat w;
  w.strands = strands;
  /* a strand search never takes the text jump */
  return err ? err : search_run(f, q, r->d_results, tables_wanted().no_jump(), w);
}

/* kstep_fmi.h: kfmi_search_strands (REV, BOTH) on resident single-device
 * handles with the traced strand kernels -- search_enqueue itself, so the
 * tables, the staging, the fetch form and the launch rules are the search's
 * own -- and one record per task copied out.  Everything that has no traced
 * kernel is refused before anything is queued. */
extern "C" int32_t kfmi_search_strands_trace(void* index, void* queries, void* results, uint32_t strands,
                                             uint32_t* trace)
{
  if (strands != KFMI_STRAND_REV && strands != KFMI_STRAND_BOTH) return KFMI_E_BAD_ARGUMENT;
  kfmi_fmi_t* f = (kfmi_fmi_t*) index;
  kfmi_qrys_t* q = (kfmi_qrys_t*) queries;
  kfmi_res_t* r = (kfmi_res_t*) results;
  if (!f || !q || !r || !trace) return KFMI_E_BAD_ARGUMENT;
  const uint64_t tasks = (strands == KFMI_STRAND_BOTH ? 2u : 1u) * q->num;
  if (r->num != tasks) return KFMI_E_BAD_ARGUMENT;
  DeviceGuard dg;
  std::shared_lock<RwLock> lk(index_lock(f));
  int32_t err = resident_single(f, q, {r});
  if (err) return err;
  if (!lane_kernels(f->dev)) return KFMI_E_NOT_IMPLEMENTED;
  SearchWhat w;
  w.strands = strands;
  return search_run(f, q, r->d_results, tables_wanted().no_jump(), w, trace, tasks);
}

}  // namespace kfmi
