/*
 * kfmi_runtime.h -- host-side runtime shared by the library's translation
 * units: kfmi_search.hip (backends, devices, uploads, the walk check, the
 * reference's entry points), kfmi_tables.hip and kfmi_jump.hip (the derived
 * tables and their settings), kfmi_group.hip (device groups), kfmi_locate.hip
 * (locate), kfmi_strands.hip / kfmi_seeds.hip / kfmi_verify.hip (strand and
 * seed searches) and kfmi_stream.hip (streamed search, host worker pool).
 * Where a search's code words come from -- maxw, words_maxw, strands, the pack
 * launch -- is decided in one place, kfmi_plan.h; plan_for / plan_launch /
 * plan_pack below are how every search form uses it.
 */
#ifndef KFMI_RUNTIME_H_
#define KFMI_RUNTIME_H_

#include <hip/hip_runtime.h>
#include <atomic>
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <shared_mutex>
#include <pthread.h>

#include "../kfmi_internal.h"
#include "kfmi_devguard.h"
#include "kfmi_kernels.h"
#include "kfmi_plan.h"

#define HIP_OK(x)                                                                   \
  do {                                                                              \
    hipError_t _e = (x);                                                            \
    if (_e != hipSuccess) {                                                         \
      fprintf(stderr, "kstepfmi: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), \
              __FILE__, __LINE__);                                                  \
      return KFMI_E_KERNEL;                                                         \
    }                                                                               \
  } while (0)

/* ------------------------------------------------------------------------ */
/* device-side handles                                                      */
/* ------------------------------------------------------------------------ */

struct kfmi_dev_index {
  int device = -1;
  int backend = -1;
  int layout = -1;
  uint32_t K = 0, d = 0, nb = 0, bwtsize = 0, nentries = 0;
  kfmi::DollarArgs dl{};
  uint32_t* ent = nullptr;     /* device entries */
  uint64_t ent_bytes = 0;
  uint32_t* sa = nullptr;      /* locate: row-sampled suffix array */
  /* every LF_K walk ends at a '$' row (check_lf_walks), checked once before
   * the first locate walk or derivation: -1 not yet, 0 no (refused), 1 yes */
  std::atomic<int> lf_perm{-1};
  uint64_t sa_bytes = 0;
  uint32_t sa_log2 = 0, sa_gen = 0;
  /* jump-start tables, one per base count (built on first use, then immutable
   * until the index leaves the device, so concurrent searches with different
   * kfmi_set_ftab values never free a table another kernel reads) */
  uint2* ftab[17] = {};
  std::mutex ftab_mu;
  /* bases of the auto table (KFMI_FTAB_AUTO), decided once per device copy
   * under ftab_mu (auto_ftab): -1 not yet, 0 none */
  int ftab_auto = -1;
  /* bit N: ftab[N] is in the folded form (kfmi_device.h ftab_entry_at): set by
   * an upload's fold pass (auto_tables) for its auto table alone, under the
   * handle's exclusive lock; cleared with the table */
  uint32_t ftab_folded = 0;
  /* skip table (DESIGN.md 5a'): one {row, code} entry per BWT row, K <= 2, task
   * backends; same lifetime rule and mutex as the ftabs.  skip_auto: the auto
   * decision of this copy (auto_skip): -1 not yet, 0 none, 1 built */
  uint2* skip = nullptr;
  int skip_auto = -1;
  /* text jump (DESIGN.md 5a'', kfmi_jump.hip): one allocation [sa | isa | text],
   * bwtsize + bwtsize + (n / 16 + 2) words; K <= 2, task backends on the plain
   * layouts; same lifetime rule and mutex as the ftabs.  jump_auto: the auto
   * decision of this copy (auto_jump): -1 not yet, 0 none, 1 built; jump_none:
   * the index failed the build's exactness check, so it never gets tables */
  uint32_t* jump_sa = nullptr;
  int jump_auto = -1;
  int jump_none = 0;
  /* remainder tables: [L, R) of every r-base read suffix, r = m % K in 1..3
   * (same lifetime rule as the ftabs, same mutex) */
  uint2* rtab[4] = {};
  uint32_t* ac_tail = nullptr; /* AltCounters layouts, 4 x NC: (LAY_MIDAC) the counters of entries E-1, E,
                                 E+1; row 3 the locate walk's sentinel correction (ac_locate_fix) */
  uint32_t ac_tail_b0 = 0xFFFFFFFFu;
};

struct kfmi_dev_queries {
  int device = -1;
  uint8_t* ascii = nullptr;    /* num*size bytes, plain layout; null when the host packed the
                                  reads on upload (`packed` is then already valid) */
  uint32_t* packed = nullptr;  /* (nwords + 1) x num u32 codes; row nwords: remainder codes */
  uint64_t num = 0;
  /* m = size = rem + K * steps: the last rem (< K) bases of a read are resolved
   * by one remainder-table lookup before its K-steps (query_geometry) */
  uint32_t size = 0, K = 0, steps = 0, nwords = 0, rem = 0;
  uint32_t packed_rows = 0;    /* rows allocated in `packed` (>= nwords + 1) */
  /* strand searches (kfmi_strands.hip): the code words of the ns * num tasks,
   * (nwords + 1) rows; allocated by the first such search (strand_reserve) */
  uint32_t* strand_words = nullptr;
  uint64_t strand_cap = 0;     /* words allocated */
};

namespace kfmi {

/* Guards the device copies of one index handle (f->dev, f->grp): searches,
 * locates, block counts and streamed searches hold it shared for as long as
 * they use the device copy; an upload that replaces it (another backend or
 * device, a new device group) or freeIndexGPU holds it exclusively, so a
 * search running on another thread never sees its tables freed.  One
 * writer-preferring lock per handle (kfmi_fmi_t::rw), so a writer is not
 * starved by a stream of searches and unrelated handles never wait on each
 * other.  RwLock is that pthread lock seen as a SharedMutex. */
struct RwLock {
  pthread_rwlock_t rw;
  void lock() { pthread_rwlock_wrlock(&rw); }
  void unlock() { pthread_rwlock_unlock(&rw); }
  bool try_lock() { return pthread_rwlock_trywrlock(&rw) == 0; }
  void lock_shared() { pthread_rwlock_rdlock(&rw); }
  void unlock_shared() { pthread_rwlock_unlock(&rw); }
  bool try_lock_shared() { return pthread_rwlock_tryrdlock(&rw) == 0; }
};
RwLock& index_lock(const void* f);

/* One non-blocking stream per device, shared by the threads that use it (their
 * work is serialised on it).  Timing events are per calling thread. */
struct DevCtx {
  bool init = false;
  hipStream_t st = nullptr;
  /* pinned chunk buffers of host-packed query uploads (upload_queries) and of
   * device-parsed FASTA loads (fa_upload), kept between calls.  One user at a
   * time per device holds up_mu for its whole pass -- a FASTA load holds it
   * through its file reads too, so a host-packed upload on the same device
   * waits for that load to finish (both are bulk host -> device streams that
   * would share the one link anyway) */
  std::mutex up_mu;
  void* up_buf[2] = {nullptr, nullptr};
  hipEvent_t up_ev[2] = {nullptr, nullptr};
  uint64_t up_cap = 0;
};
void release_upload_staging();   /* kfmi_stream_release */
/* ctx's pinned chunk buffers grown to `need` bytes each (caller holds up_mu) */
hipError_t upload_staging(DevCtx* ctx, uint64_t need);
int32_t ctx_for(int dev, DevCtx** out);   /* selects `dev`, creates its stream once */
/* The calling thread's three timing events on device `dev` (current device). */
hipEvent_t* thread_events(int dev);
/* The calling thread's search lane on device `dev`, which becomes current: the
 * device's context, the thread's own search stream and its timing events;
 * ctx_for's error, or KFMI_E_NO_DEVICE when one of them cannot be created. */
struct SearchLane {
  DevCtx* ctx = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t* ev = nullptr;
};
int32_t search_lane(int dev, SearchLane* lane);

/* per calling thread (kfmi_search.hip) */
extern thread_local int t_device;
extern thread_local int32_t t_last_error;
extern thread_local double t_ms[3];   /* kfmi_last_timing: total, pack, lf (ms) */

/* backends and kernel dispatch (kfmi_search.hip) */
bool is_coop(int backend);
int backend_for(uint32_t K);   /* the selected backend, or coop-grp for K = 4 under the implicit default */
bool fused_on();               /* the fused knob (KFMI_FUSED, kfmi_set_fused) */
/* per-lane kernels on the plain-counter layouts at K <= 2: the copies with seed, traced and verify kernels */
inline bool lane_kernels(const kfmi_dev_index* di) { return !is_coop(di->backend) && lane_kernels(di->K, di->layout); }
int32_t check_lf_walks(kfmi_dev_index* di, hipStream_t st);   /* sets di->lf_perm (kfmi_search.hip) */
hipError_t dispatch(Op op, uint32_t K, uint32_t nb, int lay, const SearchLaunch& a,
                    unsigned long long* d_total = nullptr);
IdxArgs idx_args(const kfmi_dev_index* di);
/* per-lane gathers of a table of this size as lane groups: 4, 2 or 1 (KFMI_SPLIT answers instead) */
uint32_t split_for(uint64_t table_bytes, int layout);
hipError_t launch_pack(const kfmi_dev_queries* dq, hipStream_t st);

/* the derived tables (kfmi_tables.hip): the calling thread's settings, resolved
 * against each other -- ftab: a base count, 0 or KFMI_FTAB_AUTO; skip and jump:
 * 0 off, 1 on, 2 auto and in effect (skip: the ftab setting is auto too; jump:
 * skip is 2).  Taken once on the caller's thread and passed down (a group's or
 * stream's member threads have their own); a search form that never takes the
 * text jump says so where it takes the value: no_jump(). */
struct TableWants {
  uint32_t ftab = 0, skip = 0, jump = 0;
  TableWants no_jump() const { return TableWants{ftab, skip, 0u}; }
};
TableWants tables_wanted(void);
/* ix's tables for one search under `w` with reads of m % K = rem, built where
 * `w` asks for one the copy does not have (the remainder table clears the ftab) */
int32_t use_tables(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, const TableWants& w, uint32_t rem);
/* an upload's part: the tables of a new device copy (`di->device` current) whose
 * setting in `w` is auto; never an error when one does not fit */
int32_t auto_tables(kfmi_dev_index* di, hipStream_t st, const TableWants& w);
/* frees the tables of a device copy about to be replaced (handle locked exclusively) */
void drop_ftabs(kfmi_dev_index* di);
/* the tables' budget now: kfmi_set_ftab_budget's bytes, or a quarter of the free memory of the current device */
uint64_t table_budget_now(void);
/* layouts that take the remainder table */
bool rem_supported(int layout);
/* `of` summed over a handle's device copies (every member of its device group,
 * or the single copy) under its shared lock, and member `member` of them
 * (member 0 = the single copy; caller holds the lock) */
uint64_t sum_members(void* index, uint64_t (*of)(kfmi_dev_index*));
int32_t member_index(const kfmi_fmi_t* f, uint32_t member, kfmi_dev_index** di);
/* the text jump (kfmi_jump.hip), for use_tables and auto_tables: the auto tables
 * of a device copy (never an error when they do not fit or the index fails the
 * check), ix.jsa for a search under the resolved setting `want` (kfmi_verify_seeds
 * calls it with 1 itself), and the tables' release (caller holds ftab_mu or the
 * handle's exclusive lock) */
int32_t auto_jump(kfmi_dev_index* di, hipStream_t st);
int32_t use_jump(kfmi_dev_index* di, hipStream_t st, IdxArgs& ix, uint32_t want);
void free_jump(kfmi_dev_index* di);

/* uploads (kfmi_search.hip) */
int32_t upload_index(kfmi_fmi_t* f, int backend, int dev, DevCtx* ctx, kfmi_dev_index** out = nullptr);
/* the 2K-step index of a K-step one, derived on `dev` (kfmi_derive.hip) */
int32_t derive_index(kfmi_fmi_t* f, uint32_t k_out, int dev, bool host_image, kfmi_fmi_t** out);
/* K of the handle's device copy (a K = 2 file on the grouped layout searches
 * a derived K = 4 index), else of the file: the K queries are packed for */
uint32_t device_steps(const kfmi_fmi_t* f);
int32_t upload_sa(const kfmi_fmi_t* f, kfmi_dev_index* di, DevCtx* ctx);
int32_t upload_queries(kfmi_qrys_t* q, uint32_t K, int dev, DevCtx* ctx);
void query_geometry(kfmi_dev_queries* dq, uint32_t K);
void free_dev_index(kfmi_dev_index* di);
void free_dev_queries(kfmi_dev_queries* dq);
hipError_t h2d(void* dst, const void* src, uint64_t bytes, hipStream_t st);

/* The launch plan (kfmi_plan.h) of one search of dq's reads on di, and what
 * every search form does with it (kfmi_search.hip).  ascii: the batch's or
 * chunk's ASCII rows are on the device; skip: ix.skip != nullptr. */
LaunchPlan plan_for(const kfmi_dev_index* di, const kfmi_dev_queries* dq, bool ascii, bool seeds, uint32_t strands,
                    bool skip, bool traced = false, int fused = -1 /* the knob; 0 / 1 for the counts and the accessor */);
/* the plan's launch, value-initialised: every field a search kernel reads but a seed search's spans and max_seeds */
SearchLaunch plan_launch(const LaunchPlan& p, hipStream_t st, const IdxArgs& ix, const kfmi_dev_queries* dq,
                         uint32_t* res, uint4* trace = nullptr);
hipError_t plan_pack(const LaunchPlan& p, const kfmi_dev_queries* dq, uint32_t strands, hipStream_t st);

/* The checks every entry point on resident single-device handles makes, in this
 * order: group handles (KFMI_E_NOT_IMPLEMENTED; kfmi_search sends them to
 * group_search first), missing device copies, `need` for the callers that refuse
 * these before the last one -- NEED_LANE_KERNELS, NEED_ASCII -- and results on
 * another device than the index. */
enum { NEED_LANE_KERNELS = 1, NEED_ASCII = 2 };
bool any_group(const kfmi_fmi_t* f, const kfmi_qrys_t* q, std::initializer_list<const kfmi_res_t*> rs);
int32_t resident_single(const kfmi_fmi_t* f, const kfmi_qrys_t* q, std::initializer_list<const kfmi_res_t*> rs,
                        unsigned need = 0);

/* one device batch: queue pack + kernel bracketed by ev[0..2], then wait (kfmi_search.hip).  SearchWhat: the strand
 * mode; a seed search's spans and max_seeds (d_res holds its intervals); null, or the device records of the traced
 * twin, one per read or task; the context whose lock strand_reserve takes (every form but the forward search) */
struct SearchWhat {
  uint32_t strands = KFMI_STRAND_FWD;
  uint32_t* spans = nullptr;
  uint32_t max_seeds = 0;
  uint4* trace = nullptr;
  DevCtx* ctx = nullptr;
};
int32_t search_enqueue(kfmi_dev_index* di, kfmi_dev_queries* dq, uint32_t* d_res, hipStream_t st, hipEvent_t* ev,
                       const TableWants& want, const SearchWhat& w = SearchWhat{});
/* the launches of the seed kernels and of the traced strand kernels (kfmi_seeds.hip, kfmi_strands.hip) */
hipError_t dispatch_seeds(uint32_t K, uint32_t nb, int lay, const SearchLaunch& a);
hipError_t dispatch_strands_trace(uint32_t K, uint32_t nb, int lay, const SearchLaunch& a);
/* One resident search of f->dev and q->dev on the calling thread's lane: enqueue and finish (timings in t_ms).  The
 * traced twin (`trace`: 16 bytes per task) owns its device records here: allocated for max(tasks, 1) before anything
 * is queued (KFMI_E_DEVICE_ALLOC), copied out after a successful finish (KFMI_E_KERNEL), always freed. */
int32_t search_run(kfmi_fmi_t* f, kfmi_qrys_t* q, uint32_t* d_res, const TableWants& want, SearchWhat w = SearchWhat{},
                   uint32_t* trace = nullptr, uint64_t tasks = 0);
int32_t search_finish(hipStream_t st, hipEvent_t* ev, double* ms);

/* strand searches (kfmi_strands.hip): dq->strand_words sized for both strands
 * of cq reads, and the launch that fills `out` with the task columns of
 * `strands` (REV or BOTH) -- from dq->ascii, or from the forward code words in
 * dq->packed when from_words (or when the device has no ASCII) */
int32_t strand_reserve(kfmi_dev_queries* dq, uint64_t cq, DevCtx* ctx);
hipError_t launch_strand_pack(const kfmi_dev_queries* dq, uint32_t* out, uint32_t strands, bool from_words,
                              hipStream_t st);

/* host memory helpers (kfmi_stream.hip) */
bool host_pinned(const void* p);
void par_copy(void* dst, const void* src, uint64_t bytes);
/* n ASCII rows of `size` bases -> word-major 2-bit code words (row stride n;
 * row ceil((size - rem) / 16) holds the remainder codes), over the host workers;
 * K in {1, 2, 4} (qpack.c) */
void par_pack(const char* src, uint64_t n, uint32_t size, uint32_t rem, uint32_t* out);
bool par_pread(int fd, void* dst, uint64_t off, uint64_t bytes);

/* device groups (kfmi_group.hip) */
constexpr int KFMI_MAX_GROUP = 16;
struct GroupIndex {
  int n = 0, backend = -1;
  int dev[KFMI_MAX_GROUP] = {};
  kfmi_dev_index* di[KFMI_MAX_GROUP] = {};
  hipStream_t st[KFMI_MAX_GROUP] = {};
  hipEvent_t ev[KFMI_MAX_GROUP][3] = {};
};

/* queries or results of a group: one contiguous slice per member */
struct GroupSlices {
  int n = 0;
  int dev[KFMI_MAX_GROUP] = {};
  uint64_t q0[KFMI_MAX_GROUP] = {}, num[KFMI_MAX_GROUP] = {};
  kfmi_dev_queries* dq[KFMI_MAX_GROUP] = {};
  uint32_t* d_res[KFMI_MAX_GROUP] = {};
};
int group_devices(int* devs);   /* the KFMI_DEVICES / kfmi_set_devices list */
int32_t group_transfer(kfmi_fmi_t* f, kfmi_qrys_t* q, kfmi_res_t* r, const int* devs, int n);
int32_t group_search(kfmi_fmi_t* f, kfmi_qrys_t* q, kfmi_res_t* r);
int32_t group_to_host(kfmi_res_t* r);
void group_free_index(kfmi_fmi_t* f);
void group_free_queries(kfmi_qrys_t* q);
void group_free_results(kfmi_res_t* r);

}  // namespace kfmi

#endif  // KFMI_RUNTIME_H_
