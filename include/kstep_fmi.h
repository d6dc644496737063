/*
 * kstep_fmi.h -- C ABI of the MI355X k-step FM-index backward-search engine
 * (libkstepfmi.so, built from k-step_fm-index_amd/).
 *
 * Section 1 is the reference's own link-time plugin interface
 * (/root/reference/common/interface.h:27-41) plus the common.h helpers its
 * driver calls (/root/reference/common/common.h:87-96): a program written
 * against the reference (common/searchQueries.c) links against this library
 * instead of common.c + fmIndexCPUBaseline*.c + one fmIndexGPU-*.cu file, and
 * runs unchanged.  All handles are opaque `void *`; every
 * size that can exceed 2^32 bytes is 64-bit internally (reference defect B7).
 *
 * Section 2 holds the extensions that the reference fixes at compile time
 * (backend, device, K, d) or does not have (memory-resident handles, status
 * queries, timing, the GPU index builder).  Plain C types only.
 *
 * Error codes are the reference's error_t (common.h:36-62); the index-tag
 * codes 100/101/200/201 mean "this backend needs an index with that tag".
 */
#ifndef KSTEP_FMI_H_
#define KSTEP_FMI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error_t values, common.h:36-62 */
enum {
  KFMI_SUCCESS                = 0,
  KFMI_E_OPENING_INDEX_FILE   = 1,
  KFMI_E_ALLOCATING_BWT       = 2,
  KFMI_E_ALLOCATING_FMI       = 3,
  KFMI_E_READING_BWT          = 4,
  KFMI_E_READING_FMI          = 5,
  KFMI_E_SAVING_INDEX_FILE    = 6,
  KFMI_E_SAVING_BWT_FILE      = 7,
  KFMI_E_BUILDING_BWT         = 8,
  KFMI_E_BUILDING_FMI         = 9,
  KFMI_E_OPENING_REFERENCE_FILE = 10,
  KFMI_E_ALLOCATING_REFERENCE = 11,
  KFMI_E_READING_MFASTA_FILE  = 12,
  KFMI_E_READING_REFERENCE_FILE = 13,
  KFMI_E_OPENING_MFASTA_FILE  = 14,
  KFMI_E_ALLOCATING_MFASTA    = 15,
  KFMI_E_ALLOCATING_RESULTS   = 16,
  KFMI_E_OPENING_RESULTS_FILE = 17,
  KFMI_E_READING_RESULTS_FILE = 18,
  KFMI_E_NOT_IMPLEMENTED      = 19,
  /* extensions (not in the reference) */
  KFMI_E_NO_DEVICE            = 30,  /* no HIP device / HIP runtime error      */
  KFMI_E_DEVICE_ALLOC         = 31,  /* hipMalloc failed                        */
  KFMI_E_KERNEL               = 32,  /* kernel launch / execution failed        */
  KFMI_E_BAD_ARGUMENT         = 33,  /* unsupported K, d, query size, backend   */
  KFMI_E_NOT_ON_DEVICE        = 34,  /* search called before transferCPUtoGPU   */
  KFMI_INDEX_VER_BASELINE      = 100,
  KFMI_INDEX_VER_INTERLEAVE    = 101,
  KFMI_INDEX_VER_BASELINE_AC   = 200,
  KFMI_INDEX_VER_INTERLEAVE_AC = 201
};

/* ===================== 1. reference entry points ======================== */

/* interface.h:27 / fmIndexCPUBaseline.c:71-143.  Reads any index tag
 * (100/101/200/201).  With KFMI_STRICT_TAG=1 in the environment it behaves
 * exactly like the reference loader of the selected backend: a file with
 * another tag is rejected and the required tag is returned. */
int32_t loadIndex(const char *fn, void **index);
/* interface.h:28 / genFMindex.c:155-181: "<fn>.<n>.<d>fmi<K>steps.fmi" (tag 100),
 * or the index's own tag/name suffix for transformed indexes. */
int32_t saveIndex(const char *fn, void *index);
/* interface.h:29 / common.c:248-260: 2*numresults u32, zeroed. */
int32_t initResults(uint32_t numresults, void **results);
/* interface.h:31 / fmIndexGPU-*.cu searchIndexGPU: synchronous search of every
 * query on the device; results stay on the device until transferGPUtoCPU.
 * Returns void like the reference; kfmi_last_error() gives the status. */
void    searchIndexGPU(void *index, void *queries, void *resIntervals);
/* interface.h:30 / fmIndexCPUBaseline.c:157-292 (tags 100/101) and
 * fmIndexCPUBaseline-AltCounters.c:145-310 (tags 200/201): the search on the
 * host, same integers as the reference's CPU searchers.  Like the reference it
 * is called by every thread of the caller's OpenMP parallel region
 * (searchQueries.c:84-95) and shares the queries out with an orphaned
 * `omp for schedule(static)` (GNU OpenMP); called outside a parallel region it
 * runs on the calling thread.  Results go to the host results array; a later
 * saveResults writes "<fn>.res.cpu" as the reference's CPU build does.
 * Returns void like the reference; kfmi_last_error() gives the status (33:
 * unsupported index or query size -- AltCounters indexes need m % K == 0). */
void    searchIndexCPU(void *index, void *queries, void *resIntervals);
/* interface.h:33 / fmIndexCPUBaseline.c:145-155 */
int32_t freeIndex(void **index);
/* interface.h:34 / common.c:313-322 */
int32_t freeReference(void **reference, void **index);
/* interface.h:35 / genFMindex.c:457-543: tag-100 index of a loadRef() text,
 * K and d from KFMI_K / KFMI_D (defaults 2 / 64); built on the GPU when one
 * is present (kfmi_build_index_gpu), else on the host. */
int32_t buildIndex(void *reference, void **index);
/* interface.h:36-41 / e.g. fmIndexGPU-Coop-2Step.cu:231-338 */
int32_t freeQueriesGPU(void **queries);
int32_t freeResultsGPU(void **results);
int32_t freeIndexGPU(void **index);
int32_t transferGPUtoCPU(void *results);
/* The reads go up as ASCII (the reference's form); KFMI_UPLOAD=packed (K in
 * {1, 2, 4}) packs them to 2-bit code words on the host during the upload
 * instead -- a quarter of the PCIe bytes, a win where the host workers
 * out-pack the link; same results.
 *   An index that is on the device for another backend or device is replaced:
 * the new copy is laid out beside the old one, which stays searchable should
 * the upload fail -- except for lack of device memory (a K = 4 layout is 96 GB,
 * and other handles' tables share the card).  Then the old copy is freed and
 * the upload runs once more, so a re-layout needs room for one copy, not two;
 * when that fails as well the call returns KFMI_E_DEVICE_ALLOC and the handle
 * has no device copy (kfmi_device_index_bytes 0) until a later call uploads it. */
int32_t transferCPUtoGPU(void *index, void *queries, void *results);
/* How transferCPUtoGPU left the reads: 0 not on a device, 1 ASCII, 2 code
 * words packed by the host (a device group: its first member's slice). */
int32_t kfmi_queries_upload_form(void *queries);

/* common.h:87-96 / common.c */
double   sampleTime(void);
uint32_t base2index(uint32_t base);
int32_t  loadRef(const char *fn, uint32_t refsize, void **reference);
int32_t  saveRef(const char *fn, void *reference);
int32_t  loadQueries(const char *fn, uint32_t sizequery, uint32_t numqueries, void **queries);
int32_t  writeResults(const char *fn, uint32_t *results, uint32_t numqueries);
int32_t  loadResults(const char *fn, void **results);
int32_t  freeQueries(void **queries);
int32_t  freeResults(void **results);
/* common.c:324-341: "<fn>.res.gpu", or "<fn>.res.cpu" when searchIndexCPU wrote
 * the results last (the reference names the file by its build, CUDA or not) */
int32_t  saveResults(const char *fn, void *results, void *index);
char    *errorCommon(int32_t e);

/* ========================= 2. extensions ================================= */

/* Backends (the reference selects one per binary at link time,
 * makefile:177-207).  Names:
 *   "task"        Task-{1,2}Step   : one thread per query, L and R ends      (tag 101 semantics)
 *   "coop"        Coop-{1,2}Step   : wave64 cooperative gather into LDS     (tag 101 semantics)
 *   "task-ac"     Task-2Step-AltCounters                                    (tag 201 semantics)
 *   "coop-ac"     Coop-2Step-AltCounters                                    (tag 201 semantics)
 *   "task-mid"    task-per-query on the MID128 layout: one 128-byte line per LF (tag 101 semantics)
 *   "coop-mid"    wave64 cooperative gather on the MID128 layout              (tag 101 semantics)
 *   "task-grp" / "coop-grp"   K = 3 and 4 indexes (d = 64): one 128-byte line per (block,
 *                 16-code group) holding the block's planes and those 16 counters -- one line per
 *                 LF, 25 K-steps for 100 bases at K = 4; 4 (K = 3) or 16 (K = 4) lines per block
 *                 (tag 101 semantics)
 *   "task-ac-mid" / "coop-ac-mid" the MID128 lines with AltCounters semantics: the AltCounters
 *                 step only past the last real block, from the tfmiAC sentinel (tag 201 semantics;
 *                 built from a tag 100/101 file, an AC file returns 101)
 * ("task-packed" / "coop-packed" and "task-ac128" / "coop-ac128", layouts that
 * lost to task-mid / task-ac on every measurement, were retired in round 6:
 * kfmi_set_backend returns KFMI_E_BAD_ARGUMENT for them.)
 * The default comes from KFMI_BACKEND, else "task-mid" -- and "coop-grp" for a
 * K = 3 or 4 index while neither KFMI_BACKEND nor kfmi_set_backend has chosen one
 * (kfmi_get_backend still names the selection).  transferCPUtoGPU
 * re-lays-out the loaded index for the backend: plain-counter backends take
 * tag 100 or 101 (an AC file returns 101, as the reference loader would);
 * AC backends take any tag -- a tag-100/101 file first goes through the tfmiAC
 * transform, so the results are those of the AltCounters searcher on it. */
int32_t     kfmi_set_backend(const char *name);
const char *kfmi_get_backend(void);
/* The HIP device used by the calling thread (reference: compile-time DEVICE).
 * Default: KFMI_DEVICE, else 0. */
int32_t     kfmi_set_device(int32_t device);
int32_t     kfmi_device_count(void);
/* PCI bus id ("0000:75:00.0") of HIP device `device`, NUL-terminated in buf
 * (len >= 13): names the physical GPU, which device numbers do not across
 * processes with different HIP_VISIBLE_DEVICES (not in the reference, which
 * has one compile-time DEVICE). */
int32_t     kfmi_device_pci_bus_id(int32_t device, char *buf, int32_t len);
/* Status of the last searchIndexGPU() on this thread. */
int32_t     kfmi_last_error(void);
/* searchIndexGPU with a status return. */
int32_t     kfmi_search(void *index, void *queries, void *results);
/* searchIndexCPU in a parallel region of its own: nthreads threads (0:
 * OMP_NUM_THREADS when set, else this process's CPUs -- affinity mask capped
 * by the cgroup quota).  Returns the status. */
int32_t     kfmi_search_cpu(void *index, void *queries, void *results, int32_t nthreads);
/* ftab (Bowtie-style jump start; not in the reference): every backend looks
 * up [L, R) after the first `bases` bases of each query in a table of all
 * 4^bases codes (8 B each: 134 MB at 12) built on the device with the search's
 * own LF steps, then continue from there -- results are unchanged.  The
 * first bases / K K-steps of a read depend only on the index and on the read's
 * last `bases` bases, and the index stays the same from call to call, so the
 * table is a default like the upload's own re-layout and remainder table, not
 * an option: with KFMI_FTAB unset and no call here the setting is
 * KFMI_FTAB_AUTO -- kfmi_ftab_auto_bases() of the index's rows, its K and a
 * quarter of the device memory free when the table is allocated, built during
 * transferCPUtoGPU (on every member of a device group) so that no search call
 * pays for it; a failed allocation or a budget too small steps the auto table
 * down by K bases or switches it off, never an error.  0 = off: the pure
 * walk of every K-step, as every comparison row is taken.  An explicit count
 * is at most 16 and a multiple of K to take effect; its table is built at the
 * first search that needs it and KFMI_E_DEVICE_ALLOC is returned when it does
 * not fit.  KFMI_FTAB (read once at the first search; a count, 0 or "auto")
 * sets it process-wide; the setter is per calling thread like the backend.
 * Memory: 8 * 4^bases bytes per uploaded index and device, next to the index
 * copy -- 34 GB at 16 bases (a 3 Gbase index), 134 MB at 12 (64 Mbase).  A
 * transfer that replaces a handle's device copy (another backend or device)
 * frees the old copy's tables before it allocates the new copy. */
#define KFMI_FTAB_AUTO 0xFFFFFFFFu
int32_t     kfmi_set_ftab(uint32_t bases);
/* The auto rule (pure host arithmetic, no device): the largest N <= 16 that is
 * a multiple of K with 4^N <= 2 * rows (rows = n + 1; deeper tables are mostly
 * empty intervals), stepped down by K while 8 * 4^N exceeds budget_bytes; 0
 * (off) for an index of fewer than 8 rows, K outside 1..4 or a budget below
 * the smallest table. */
uint32_t    kfmi_ftab_auto_bases(uint64_t rows, uint32_t K, uint64_t budget_bytes);
/* Test knob, process-wide: the byte budget of the auto rule in place of a
 * quarter of the free device memory; KFMI_FTAB_BUDGET_FREE returns to that. */
#define KFMI_FTAB_BUDGET_FREE 0xFFFFFFFFFFFFFFFFull
int32_t     kfmi_set_ftab_budget(uint64_t bytes);
/* Bytes of the jump-start tables the handle's device copies hold (all members
 * of a device group); kfmi_device_index_bytes counts the index copies only. */
uint64_t    kfmi_device_ftab_bytes(void *index);
/* Skip table (not in the reference): once a search interval is the single row
 * [i, i+1), its next 16 bases can keep it non-empty in one way only -- they
 * must equal the 16 text bases before suffix SA[i] -- and then the interval is
 * [LF^J(i), LF^J(i)+1) after J = 16 / K K-steps.  Both are properties of row i,
 * so a table of 8 B per BWT row ({row, 32-bit code of those J steps}), built on
 * the device at upload from the search's own steps, replaces J dependent index
 * lines by one lookup.  A read whose next 16 bases differ from the entry (or
 * whose entry is marked invalid: the steps pass a '$' row) takes the ordinary
 * K-steps from the state it had, so results stay bit for bit what the walk
 * gives, empty intervals included.  The gain belongs to reads whose walk stays
 * on one row -- exact, locally unique matches, the seeding case; a read in a
 * repeat walks until its interval narrows, a read with a mismatch pays one
 * wasted lookup and walks as before.
 *   Used by the per-lane search kernels (task backends) with in-kernel packing
 * (reads of up to 256 bases) at K = 1, 2; the coop backends, K = 3 / 4, longer
 * reads, locate and the statistics calls ignore it, and no table is built for
 * an index uploaded for them.
 *   kfmi_set_skip (per calling thread) / KFMI_SKIP (read once; 0, 1 or "auto"):
 * 0 = off; KFMI_SKIP_AUTO (the default) = in effect exactly when the ftab
 * setting is KFMI_FTAB_AUTO too, so kfmi_set_ftab(0) keeps meaning the pure
 * walk of every K-step and an explicit count the walk after that one table;
 * the table is then built inside transferCPUtoGPU after the auto ftab (on
 * every member of a device group) when kfmi_skip_auto() allows it, and a
 * failed allocation leaves it out, never an error; 1 = on whatever the ftab
 * setting: built at the first search, KFMI_E_DEVICE_ALLOC when it does not fit.
 * Memory: 8 B x rows next to the index copy (24 GB at 3 Gbase) and the same
 * again while it is built; freed with the jump-start tables. */
#define KFMI_SKIP_AUTO 0xFFFFFFFFu
int32_t     kfmi_set_skip(uint32_t mode);
/* The calling thread's setting resolved against its ftab setting: 0 = off,
 * 1 = on (explicit), 2 = auto and in effect. */
uint32_t    kfmi_skip_in_effect(void);
/* The auto rule (pure host arithmetic): 1 when K is 1 or 2, 8 <= rows < 2^32
 * and the table with its transient twin, 16 * rows bytes, is within
 * budget_bytes (a quarter of the free device memory, or kfmi_set_ftab_budget's
 * bytes); else 0. */
uint32_t    kfmi_skip_auto(uint64_t rows, uint32_t K, uint64_t budget_bytes);
/* Bytes of the skip tables the handle's device copies hold (all members of a
 * device group); not part of kfmi_device_ftab_bytes or kfmi_device_index_bytes. */
uint64_t    kfmi_device_skip_bytes(void *index);
/* Test accessor: the single-device copy's table copied to out[entries] (8 B
 * each: u32 row, u32 code; row 0xFFFFFFFF = no skip from this row); entries
 * must be its row count n + 1; *steps (may be null) = J. */
int32_t     kfmi_device_skip_table(void *index, void *out, uint64_t entries, uint32_t *steps);
/* Text jump (not in the reference): once a search interval is the single row
 * [i, i+1), the rest of the walk is no search any more.  One text position
 * p = SA[i] carries the matched suffix; with t K-steps left the walk ends on
 * [ISA[p - tK], ISA[p - tK] + 1) when p >= tK and the tK text bases before p
 * are the read's remaining bases, and on an empty interval otherwise.  That is
 * three lookups whatever t is -- SA[i], the packed text window, ISA[p - tK] --
 * in two dependent round trips, where the skip table takes one per 16 bases.
 * A lane jumps when its interval is one row and at least kfmi_set_jump_min
 * bases remain (default 8, DESIGN.md 5a''); a lane whose compare fails goes on through the
 * skip lookups and K-steps from the state it had, so results stay bit for bit
 * what the walk gives, the particular empty interval included.  Such a read
 * (one with a mismatch) pays two wasted lookups.
 *   The tables -- the full suffix array, its inverse (4 B x rows each) and the
 * text at 2 bits per base, 24.75 GB at 3 Gbase -- are built on the device from
 * the uploaded index alone, with 8 B x rows more while they are built, and
 * kept only when the build's own check finds them exact (every LF walk ends at
 * a '$' row and rows and positions pair up one to one); a 'ref'-mode index
 * that is no permutation gets none, which is no error.
 *   Used by the forward per-lane search kernels with in-kernel packing (reads
 * of up to 256 bases) on the plain layouts (task, task-mid) at K = 1, 2; the
 * AltCounters and coop backends, K = 3 / 4, strand and seed searches, locate
 * and the statistics calls ignore it.
 *   kfmi_set_jump (per calling thread) / KFMI_JUMP (read once; 0, 1 or "auto"):
 * 0 = off; KFMI_JUMP_AUTO (the default) = in effect exactly when the skip
 * setting is auto and in effect, so kfmi_set_ftab(0), KFMI_SKIP=0 and an
 * explicit ftab count keep naming the walks they named; the tables are then
 * built inside transferCPUtoGPU after the auto skip table (on every member of
 * a device group) when kfmi_jump_auto() allows it, and a failed allocation
 * leaves them out, never an error; 1 = on whatever the other settings: built
 * at the first search, KFMI_E_DEVICE_ALLOC when they do not fit.  Freed with
 * the jump-start tables.
 *   Line table (DESIGN.md 5a'''): behind the three tables, in the same
 * allocation, 128-byte lines of 16 ISA entries and the 256 text bases that end
 * where those entries' windows end, so a window of up to 240 bases and its ISA
 * entry cost one memory line instead of two or three.  n / 16 + 2 lines, 8 B x
 * rows and a little: 24 GB at 3 Gbase.  They take the place the build's
 * temporary arrays had, so the build's peak is what it was.  Longer windows
 * use the flat tables.  kfmi_set_jump_lines / KFMI_JUMP_LINES (process-wide, a
 * search reads it when it is queued; default 1): 0 = every window from the
 * flat tables, 1 = from the lines, every load of that round trip issued per
 * 16-lane group where the tables are past the translation reach (as the other
 * gathers are), 2 = from the lines with the window's loads never split (the
 * slower form, kept for measurements: 1.21 against 1.00 ms per 10M 100 bp
 * reads at 3 Gbase, DESIGN.md 5a'''); the lines are built either way and no
 * setting changes a result.  Read-length rule: where the loads go out per
 * 16-lane group (tables past the translation reach, 3 Gbase), a search of
 * reads longer than 192 bases takes the flat tables' form under setting 1 as
 * well -- from about 196 bases on the grouped loads cost more than the saved
 * line (jump_sweep_r12*.jsonl, DESIGN.md 5a''').
 *   Default footprint of an uploaded 3 Gbase index with every auto table:
 * about 110 GB (3 index + 34 ftab + 24 skip + 24.75 + 24 lines). */
#define KFMI_JUMP_AUTO 0xFFFFFFFFu
#define KFMI_JUMP_MIN_DEFAULT 8u
int32_t     kfmi_set_jump(uint32_t mode);
/* The calling thread's setting resolved against its skip setting: 0 = off,
 * 1 = on (explicit), 2 = auto and in effect. */
uint32_t    kfmi_jump_in_effect(void);
/* Fewest remaining bases a lane jumps with (process-wide, >= 1; a search reads
 * it when it is queued), and its current value. */
int32_t     kfmi_set_jump_min(uint32_t bases);
uint32_t    kfmi_jump_min(void);
/* The auto rule (pure host arithmetic): 1 when K is 1 or 2, 2 <= rows < 2^32
 * and the build's peak, 16 * rows + 4 * ((rows - 1) / 16 + 2) bytes, is within
 * budget_bytes (a quarter of the free device memory, or kfmi_set_ftab_budget's
 * bytes); else 0. */
uint32_t    kfmi_jump_auto(uint64_t rows, uint32_t K, uint64_t budget_bytes);
/* Bytes of the text jump's tables the handle's device copies hold (all members
 * of a device group): 8 * rows + 4 * ((rows - 1) / 16 + 2) per copy. */
uint64_t    kfmi_device_jump_bytes(void *index);
/* Test accessor: the tables of the single-device copy (member 0), or of member
 * `member` of a device group, copied to sa[rows], isa[rows] (rows = n + 1;
 * sa 0xFFFFFFFF = a row without a suffix) and text[words], words =
 * n / 16 + 2: base n - 1 - g of the text at bits 2g of the word stream, zeros
 * past the text.  KFMI_E_NOT_ON_DEVICE without tables. */
int32_t     kfmi_device_jump_tables(void *index, uint32_t member, uint32_t *sa, uint32_t *isa, uint64_t rows,
                                    uint32_t *text, uint64_t words);
/* The line table's use by the search (above), and the value in effect. */
int32_t     kfmi_set_jump_lines(uint32_t mode);
uint32_t    kfmi_jump_lines(void);
/* Bytes of the line tables the handle's device copies hold (all members of a
 * device group), not counted in kfmi_device_jump_bytes: 128 * (n / 16 + 2) per
 * copy. */
uint64_t    kfmi_device_jump_line_bytes(void *index);
/* Test accessor: the raw lines of the same copy as kfmi_device_jump_tables,
 * out[32 * lines], lines = n / 16 + 2 (the last one padding).  Line j: dword
 * t < 16 = isa[n - (16 j + t)], 0xFFFFFFFF where 16 j + t > n; dwords 16 .. 31
 * = words j - 15 .. j of the text's word stream, zero outside it. */
int32_t     kfmi_device_jump_lines(void *index, uint32_t member, uint32_t *out, uint64_t lines);
/* Host arithmetic of a lane's reads in the line table, for the tests: out[0] =
 * the lines' first dword in the allocation, out[1] = the line count, and for a
 * jump with nb <= 240 bases left at text position p (nb <= p <= n), as dwords
 * from the lines' start: out[2] = its ISA entry, out[3] = the first dword of
 * its window, out[4] = the window's bit offset there, out[5] = the dwords the
 * compare reads. */
int32_t     kfmi_jump_line_geometry(uint64_t n, uint64_t p, uint32_t nb, uint64_t *out);
/* Folded jump-start table (not in the reference; DESIGN.md 5a''''): a read whose
 * jump-start entry is the one row [L, L + 1) next loads SA[L] for its text
 * jump, a value that depends on the index alone.  The auto table of an upload
 * that also built the text jump's tables therefore carries it: with n = rows - 1,
 * an entry {x, y} holds x = L and y = R - L, except that a one-row entry holds
 * y = 0xFFFFFFFF - SA[L].  The y codes 0xFFFFFFFF - n .. 0xFFFFFFFF are
 * positions, so the form is lossless exactly when every width other than 1 is
 * below 0xFFFFFFFF - n (kfmi_ftab_fold_bound): always for n < 2^31, by the
 * text above that.  The upload decides it with a pass over the table and
 * leaves a table that does not fit as {L, R}; that is no error.  Every kernel
 * that reads the table decodes the entry; only the text jump uses the position,
 * and no result changes.  Tables built at a search (an explicit kfmi_set_ftab
 * count, or an index uploaded under other settings) are never folded.  No
 * device memory is added.
 *   kfmi_set_ftab_fold / KFMI_FTAB_FOLD (process-wide, default 1; an upload
 * reads it when it builds its tables): 0 keeps every table {L, R}.
 * kfmi_set_ftab_fold_bound (test knob, process-wide): a value other than 0
 * lowers the bound of the fit rule to it, so the "does not fit" branch runs on
 * a small index; 0 = the rule's own bound. */
int32_t     kfmi_set_ftab_fold(uint32_t on);
uint32_t    kfmi_ftab_fold(void);
int32_t     kfmi_set_ftab_fold_bound(uint32_t bound);
/* Host arithmetic of the folded form, for the tests.  The fit rule's bound
 * for an n-base text, and whether a table whose largest width other than 1 is
 * max_width fits it. */
uint32_t    kfmi_ftab_fold_bound(uint64_t n);
uint32_t    kfmi_ftab_fold_fits(uint64_t n, uint64_t max_width);
/* out[0 .. 1] = the folded entry {x, y} of [L, R) with p = SA[L] (read only
 * when R = L + 1); KFMI_E_BAD_ARGUMENT when the width does not fit the rule or
 * p > n. */
int32_t     kfmi_ftab_fold_encode(uint64_t n, uint32_t L, uint32_t R, uint32_t p, uint32_t *out);
/* out[0 .. 2] = L, R and p (0xFFFFFFFF when the entry carries none) of the
 * entry {x, y} of a table that is folded (folded != 0) or not: the decode every
 * kernel takes. */
int32_t     kfmi_ftab_fold_decode(uint64_t n, uint32_t x, uint32_t y, uint32_t folded, uint32_t *out);
/* Test accessor: `count` raw entries from entry `first` of the auto
 * jump-start table of the single-device copy (member 0) or of member `member`
 * of a device group, copied to out[2 * count] as stored; *bases and *folded
 * (either may be null) = the table's base count and whether it is in the
 * folded form.  KFMI_E_NOT_ON_DEVICE without an auto table, KFMI_E_BAD_ARGUMENT
 * when the range leaves the table. */
int32_t     kfmi_device_ftab_entries(void *index, uint32_t member, uint32_t *out, uint64_t first, uint64_t count,
                                     uint32_t *bases, uint32_t *folded);
/* Test knobs of the search path (not in the reference), process-wide; their
 * environment variables are read once, at the first search, and these setters
 * switch them afterwards.  Split class (KFMI_SPLIT): the fetch form the task
 * kernels use for an index of that table-size class -- 0 = by the uploaded
 * table's size (default), 1 (< 2 GB), 2 (2-3.5 GB), 4 (larger); other values
 * KFMI_E_BAD_ARGUMENT.  Fused packing (KFMI_FUSED): 1 = reads of up to 256
 * K-step bases are packed inside the search kernel (default), 0 = always the
 * separate pack launch.  Results are identical either way. */
int32_t     kfmi_set_split_class(uint32_t cls);
int32_t     kfmi_set_fused(int32_t on);
/* Walk check of locate and the K = 2 -> 4 derivation (every LF_K walk must end
 * at a '$' row; indexes that fail are refused with KFMI_E_BUILDING_FMI), run
 * once per device copy: 0 = by size (default: full pointer jumping below 2^22
 * rows, the sampled check above), 1 = always full pointer jumping, 2 = always
 * the sampled check (which falls back to full jumping when it cannot decide);
 * other values KFMI_E_BAD_ARGUMENT.  Test knob, process-wide, no environment
 * variable.  kfmi_walk_check_last: how the last check decided -- 0 none yet,
 * 1 full, 2 sampled, 3 sampled then full. */
int32_t     kfmi_set_walk_check(uint32_t mode);
/* Test knob, process-wide, no environment variable: the next n index uploads
 * (each attempt of transferCPUtoGPU counts) find no room on the device for
 * their copy and fail as a full card makes them fail (KFMI_E_DEVICE_ALLOC),
 * without taking any memory; 0 = none (default). */
int32_t     kfmi_fail_index_uploads(uint32_t n);
int32_t     kfmi_walk_check_last(void);
/* Every entry point leaves the caller's current HIP device as it found it
 * (hipGetDevice before == after), whichever devices it used inside. */
/* Device groups (runtime multi-GPU behind the same handles; the reference
 * picks one GPU at compile time with -DDEVICE, Coop-2Step.cu:256).  With two
 * or more devices listed -- here or in KFMI_DEVICES=0,1,... -- transferCPUtoGPU
 * replicates the index on every device and cuts queries and results into
 * contiguous slices (multiples of 64 reads), searchIndexGPU runs all slices
 * concurrently (one stream per device) and transferGPUtoCPU gathers them into
 * h_results; results equal the single-device ones.  A device may be listed
 * twice (two replicas on one GPU).  n = 0 returns to single-device mode, n = 1
 * equals kfmi_set_device.  Per calling thread.  kfmi_locate works on group
 * handles (each device locates its slice), so does kfmi_search_stream (one
 * slice and host thread per member), and reads parsed on a device
 * (kfmi_load_queries_gpu) reach the members device to device, and
 * kfmi_count_blocks sums the members' slices. */
int32_t     kfmi_set_devices(const int32_t *devices, int32_t n);
/* The device list (returns its length; 0 = single-device mode). */
int32_t     kfmi_get_devices(int32_t *devices, int32_t cap);
/* Device-side timing of the last search, from HIP events on the library's
 * stream: total (pack + LF), query packing, and the LF kernel alone (ms). */
int32_t     kfmi_last_timing(double *ms_total, double *ms_pack, double *ms_lf);

/* Strict loader: as the reference, rejects a tag other than `required_tag`
 * and returns that tag (common.c:304-307 turns it into a hint). */
int32_t kfmi_load_index_tag(const char *fn, uint32_t required_tag, void **index);
/* Index from an in-memory file image (header + entries); the bytes are copied. */
int32_t kfmi_index_from_image(const void *image, uint64_t bytes, void **index);
/* Serialised file image of an index (header + entries); pointer owned by the index. */
int32_t kfmi_index_image(void *index, const void **image, uint64_t *bytes);
/* Header fields: out[0..5] = tag, steps, bwtsize, ncounters, nentries, chunk;
 * out[6..9] dollarPositionBWT; out[10..13] dollarBaseBWT. */
int32_t kfmi_index_header(void *index, uint32_t *out14);

/* Layout transforms (transformIndexBitmaps.c:269-295, transformIndexAlternateCounters.c:387-479). */
int32_t kfmi_transform_interleave(void *index100, void **index101);
int32_t kfmi_transform_ac(void *index100, void **index200, void **index201);
/* The inverse of kfmi_transform_ac: a tag-200/201 (AltCounters) index back to
 * the tag-100 file it came from, byte for byte (no reference counterpart; the
 * AltCounters-semantics MID128 backends take AltCounters files through it). */
int32_t kfmi_transform_plain(void *index_ac, void **index100);

/* Queries/results handles over caller memory-resident data (the FFI form of
 * loadQueries/initResults).  `ascii` is num*size bytes, query q at q*size. */
int32_t   kfmi_queries_from_buffer(const char *ascii, uint64_t num, uint32_t size, void **queries);
int32_t   kfmi_results_alloc(uint64_t num, void **results);
uint32_t *kfmi_results_host(void *results);      /* 2*num u32, [L0,R0,L1,R1,...] */
uint64_t  kfmi_results_num(void *results);

/* Index construction (genFMindex.c:457-543) from an ACGT text of n bases.
 * _gpu: suffix sort and all layout passes on the device.  want_host_image != 0
 * copies the tag-100 image to host memory at once; 0 keeps the entries in HBM
 * only (the handle owns them): transferCPUtoGPU then lays them out device to
 * device, and the host image is fetched on first use (kfmi_index_image,
 * saveIndex, the transforms, the AltCounters layouts).  Returns a tag-100
 * index. */
int32_t kfmi_build_index_cpu(const char *text, uint64_t n, uint32_t k, uint32_t d, void **index);
int32_t kfmi_build_index_gpu(const char *text, uint64_t n, uint32_t k, uint32_t d,
                             int32_t want_host_image, void **index);
/* A 2K-step index derived on the current device from a K-step one (K = 1 or
 * 2, tag 100 or 101; k_out = 2K), without the text: row i's 2K-mer is its
 * K-mer plus the K-mer of row LF_K(i) (DESIGN.md 5d').  The result is the
 * tag-100 index the builders write for that text at k_out, byte for byte
 * (ACGT texts; an index with an LF_K walk that never reaches a '$' row --
 * 'ref'-mode indexes of texts with other bytes -- returns
 * KFMI_E_BUILDING_FMI, from the walk check run before deriving, see
 * kfmi_set_walk_check); its entries stay in HBM unless want_host_image.  The
 * reference's K = 2 files thus search on the K = 4 layout (coop-grp). */
int32_t kfmi_derive_index_gpu(void *index, uint32_t k_out, int32_t want_host_image, void **out);
/* Alphabet of the builders (process-wide; NULL = KFMI_ALPHABET, else "acgt"):
 *   "acgt" only A/C/G/T (anything else: KFMI_E_BUILDING_BWT);
 *   "map"  every byte through base2index (N -> G, lowercase -> uppercase), a
 *          consistent index of that text (true suffix-array intervals);
 *   "ref"  byte-compatible with the reference builder (genFMindex.c) on any
 *          text: raw-byte suffix order (divbwt64), base2index codes, and for
 *          K >= 2 its LF walk; rows the walk never writes hold code 0 (A)
 *          where the reference leaves uninitialised malloc memory (the
 *          tests emulate its bytes, tests/ref_fill.py).  loadRef also copies the
 *          file the reference's way (readRef, common.c:42-76: later header
 *          lines kept, 255-byte fgets pieces each losing their last byte).
 * All three agree on ACGT-only text. */
int32_t kfmi_set_alphabet(const char *mode);
/* Diagnostics of the last GPU build in this process: sorted positions whose
 * 32-base key tied with their predecessor, and the prefix-doubling rounds the
 * device spent resolving them (0 when there were none). */
int32_t kfmi_build_stats(uint64_t *ties, uint32_t *rounds);

/* Dedup-aware algorithmic traffic of the last search: sum over queries and
 * steps of distinct d-blocks touched (1 if L/d == R/d else 2), SURVEY 8(d). */
int32_t kfmi_count_blocks(void *index, void *queries, uint64_t *blocks);
/* The 128-B lines the active backend's task-kernel fetches touch over the
 * batch (statistics, not timed): out[0] distinct lines per K-step summed over
 * the batch (lines the two ends share counted once), out[1] LF ends whose
 * counter lies outside their planes' line, out[2] LF ends fetched, out[3] ends
 * counted forward from block b-1 (line-local, tags 101/201).  Set the backend
 * and transfer the index first (as for kfmi_count_blocks). */
int32_t kfmi_count_lines(void *index, void *queries, uint64_t out[4]);

/* Streamed search from host memory: `num` queries of `size`
 * ASCII bytes at `ascii`, results [L0,R0,L1,R1,...] into `results` (2*num
 * u32).  The index must already be on the device (transferCPUtoGPU(index,
 * NULL, NULL)).  Chunks of `chunk` queries (0: KFMI_STREAM_CHUNK, else 2^19,
 * or 2^16 when every chunk goes as ASCII) rotate over KFMI_STREAM_SLOTS
 * (default 6) HIP streams so that host packing, H2D, LF and result D2H of
 * successive chunks overlap.  Each
 * chunk either is packed by the host to code words (kfmi_pack_queries; PCIe
 * carries 4 bytes per 16 bases) or goes as ASCII (pinned: DMA'd directly;
 * pageable: staged through pinned buffers) and is packed on the device.  By
 * default the choice is made per chunk from the measured host-packing and
 * link rates (whichever finishes first; KFMI_LINK_SHARERS=n when n processes
 * share the device's PCIe link); KFMI_STREAM_HOSTPACK=1 packs every
 * chunk on the host, =0 sends every chunk as ASCII.  Host work runs on KFMI_HOST_THREADS threads (default min(16,
 * cores)).  Blocking; kfmi_last_timing: total = wall time of the call, pack =
 * host packing / staging time, lf = time blocked on chunks in flight.
 * Results equal kfmi_search's. */
int32_t kfmi_search_stream(void *index, const char *ascii, uint64_t num, uint32_t size,
                           uint32_t *results, uint64_t chunk);
/* loadQueries with the parsing on the device: the file is read
 * in 64 MB pieces into pinned buffers (parallel pread) and DMA'd to the current
 * device, where kernels find the read lines, check them and lay the first
 * `numqueries` reads out as loadQueries would (0 = every read in the file);
 * same format and errors as loadQueries.  The returned queries live on the
 * device only (no host copy): transferCPUtoGPU uses them as they are (on the
 * device they were loaded on); on a device group every member copies its slice
 * device to device, and the parsing device's full copy stays allocated beside
 * the slices (its bytes count twice there) so that the same handle still works
 * in single-device mode afterwards -- freeQueriesGPU releases both. */
int32_t kfmi_load_queries_gpu(const char *fn, uint32_t sizequery, uint64_t numqueries, void **queries);
/* Packs num reads of `size` bases (plain layout q*size, as loadQueries keeps
 * them, common.c:163-173) into the 2-bit code words the search consumes, on the
 * host: word-major, word w of read q at words[w * num + q], ceil(size/16) words
 * per read, the base at reversed index r (base size-1-r) at bits 2r..2r+1 of
 * the read's bit string (fmIndexCPUBaseline.c:200-226 order; K-independent).
 * kfmi_search_stream uses it to send 4 bytes per 16 bases over PCIe. */
int32_t kfmi_pack_queries(const char *ascii, uint64_t num, uint32_t size, uint32_t *words);
/* The same for a K-step index (K = 1, 2 or 4) and reads of any length: with
 * r = size % K, the stream covers bases 0 .. size-r-1 (ceil((size-r)/16) word
 * rows) and, when r > 0, one more row holds each read's remainder-table index
 * (base size-1 at bits 0-1, size-2 at 2-3, ...) -- what kfmi_search_stream
 * sends for such reads.  r = 0 gives kfmi_pack_queries' words. */
int32_t kfmi_pack_queries_k(const char *ascii, uint64_t num, uint32_t size, uint32_t k, uint32_t *words);
/* Host threads of the parallel host paths (loadQueries, the streamed search's
 * packers, the device loader's reads): KFMI_HOST_THREADS, else this process's
 * CPUs (affinity mask capped by the cgroup quota) divided among the ranks on
 * this host (LOCAL_WORLD_SIZE), 2 to 16. */
int32_t kfmi_host_threads(void);
/* Pinned (page-locked) host memory for query/result buffers. */
int32_t kfmi_host_alloc(uint64_t bytes, void **p);
int32_t kfmi_host_free(void *p);
/* Frees the staging and device buffers kfmi_search_stream keeps per device. */
int32_t kfmi_stream_release(void);
/* Share of the reads of this thread's last kfmi_search_stream that were packed
 * on the host (the rest went over PCIe as ASCII). */
double  kfmi_stream_hostpacked_fraction(void);

/* ---- both strands (not in the reference, which searches a read as written) --
 * A sequencing read comes from either strand of the genome.  With code =
 * base2index(byte) (A0 C1 G2 T3), the reverse strand of a read P of m bases is
 * the read P' with
 *     P'[j] = "ACGT"[3 - base2index(P[m-1-j])].
 * The definition is on codes: N and every other byte go the way base2index
 * sends them (N -> G, lowercase like uppercase) and are complemented from
 * there, so P' is always ACGT.  A reverse-strand interval is, bit for bit,
 * what the forward search of the same backend returns for P' -- every backend
 * and its semantics (AltCounters included), K = 1-4, any m (m % K != 0 through
 * the remainder table; AltCounters layouts return 33 there, as the forward
 * search does), jump-start table on or off.
 *   strands = KFMI_STRAND_FWD is exactly kfmi_search / kfmi_search_stream /
 * kfmi_search_cpu (the same code path).  KFMI_STRAND_REV: `results` holds num
 * intervals, interval q that of P'_q.  KFMI_STRAND_BOTH: a results handle of
 * 2 * num intervals (kfmi_results_alloc(2 * num), transferred as usual), or
 * 4 * num u32 for the streamed call: interval 2q is the forward interval of
 * read q, 2q + 1 its reverse one, so every slice of reads is a contiguous slice
 * of results and kfmi_locate works on such a handle unchanged (it sees 2 * num
 * intervals).  Any other `strands` value, or a results handle whose num does
 * not fit, returns KFMI_E_BAD_ARGUMENT.  No environment variable and no
 * per-thread setting select the strands: the result size differs, so every
 * existing call stays as it is.
 *   On the device the reverse strand's code words are derived from the forward
 * reads already there: no second copy of the reads is made on
 * the host, crosses PCIe or is kept in HBM as ASCII.  The task backends at
 * K = 1, 2 pack either strand inside the search kernel (reads of up to 256
 * bases with m % K == 0, ASCII on the device, fused packing on): one launch
 * and no memory beyond the forward search's.  Every other case -- the coop
 * backends, K = 3 / 4, m % K != 0, longer reads, KFMI_UPLOAD=packed handles
 * and host-packed stream chunks -- first writes the code words of the ns * num
 * tasks with a pack launch and runs the backend's forward LF kernel on them
 * (with the skip table where it is in effect).  Those words take
 * 8 * (ceil(m / 16) + 1) bytes per read of device memory (64 B at m = 100),
 * allocated by the first such search of a queries handle and kept until
 * freeQueriesGPU / a new transfer, and as much per read of a stream slot
 * (freed by kfmi_stream_release).  They belong to the queries handle: two
 * strand searches of ONE queries handle must not run at the same time (REV and
 * BOTH lay the words out differently); searches of different handles, and
 * forward searches, run concurrently as before.
 *   Device groups: kfmi_search_stream_strands supports them (each member
 * streams its slice of reads [a, b) into results + 2 * ns * a, ns = 1 or 2
 * strands); kfmi_search_strands returns KFMI_E_NOT_IMPLEMENTED on group handles
 * for strands != FWD (the group transfer cuts results by their own count,
 * which is then not the read slices').
 *   kfmi_search_cpu_strands is the host search of the same tasks (it writes the
 * reverse complements to a temporary; the results handle may be larger than
 * ns * num, as for kfmi_search_cpu).  kfmi_revcomp_queries writes P' of every
 * read (num * size bytes at `out`, which must not overlap `ascii`), over the
 * host workers like loadQueries. */
enum { KFMI_STRAND_FWD = 1, KFMI_STRAND_REV = 2, KFMI_STRAND_BOTH = 3 };
int32_t kfmi_search_strands(void *index, void *queries, void *results, uint32_t strands);
int32_t kfmi_search_stream_strands(void *index, const char *ascii, uint64_t num, uint32_t size,
                                   uint32_t *results, uint64_t chunk, uint32_t strands);
int32_t kfmi_search_cpu_strands(void *index, void *queries, void *results, uint32_t strands, int32_t nthreads);
int32_t kfmi_revcomp_queries(const char *ascii, uint64_t num, uint32_t size, char *out);   /* P -> P', host */
/* Test accessor (host only, no device): the code words of the ns * num tasks of
 * `strands` (REV or BOTH) from the forward code words of kfmi_pack_queries_k
 * (k in {1, 2, 4}; rows x num in, rows x ns * num out), computed by the same
 * code as the device kernel that serves KFMI_UPLOAD=packed handles and
 * host-packed stream chunks.  A reverse task's column equals
 * kfmi_pack_queries_k of kfmi_revcomp_queries of the read. */
int32_t kfmi_strand_words_host(const uint32_t *words, uint64_t num, uint32_t size, uint32_t k,
                               uint32_t strands, uint32_t *out);
/* Test accessor (host only, no device): reverse_stream<maxw> of every column of
 * `words` -- the register form of the same identity, which the kernels that
 * pack from ASCII rows run (the fused strand kernel and the whole-row strand
 * pack).  words and out are maxw x num, 16 bases per word, word-major; a
 * column holds the forward code words of a read of `size` bases, zero above
 * base size-1.  maxw must be 8 or 16 and 1 <= size <= 16 * maxw, else
 * KFMI_E_BAD_ARGUMENT. */
int32_t kfmi_reverse_stream_host(const uint32_t *words, uint64_t num, uint32_t size, uint32_t maxw,
                                 uint32_t *out);

/* ---- seed search (not in the reference, which answers for the whole read) ----
 * Every other search returns one interval per task, the whole read's, so a
 * read with one sequencing error gets an empty interval and nothing else.  A
 * seed search returns the greedy right-to-left factorisation of each task
 * into maximal exact segments (the adaptive-region seeding of GEM-style
 * mappers): a read that yields f segments cannot align with fewer than f - 1
 * differences, and each segment's interval is a seed for kfmi_locate.
 *   A task is a read P of m bases on one strand (KFMI_STRAND_REV tasks are the
 * read P' above and their coordinates are those of P').  With K the index's
 * step count (1 or 2) and rem = m % K, the units of a task are, from the right,
 * its last rem bases (if rem > 0) and then consecutive groups of K bases down
 * to base 0.  With e = m and S = max_seeds, while e > 0 and fewer than S
 * records exist:
 *   1. take the unit ending at e; if that unit alone does not occur in the
 *      text (tiny or low-complexity texts only), set e to its start, emit
 *      nothing and go on;
 *   2. else extend leftwards unit by unit while the substring still occurs,
 *      b the start of the longest such substring P[b .. e);
 *   3. emit the record {L, R, start = b, len = e - b}, [L, R) the suffix-array
 *      interval of P[b .. e) -- the integers the forward search of that
 *      substring returns on this backend -- and set e = b.
 * "Occurs" is R > L.  The granularity is the index's K: at K = 2 a segment ends
 * on a 2-base boundary counted from the right end (after the rem bases), so it
 * can stop one base short of the longest match; that is what the K-step walk
 * decides without a second index.  A task whose whole-read interval is not
 * empty yields exactly the one record {that interval, 0, m}; max_seeds = 1 asks
 * how deep a read matches from its right end and where that suffix occurs.
 *   `intervals` and `spans` are two ordinary results handles of S * ns * num
 * entries each (kfmi_results_alloc, transferred as usual; ns = 1 for FWD and
 * REV, 2 for BOTH) and must be exactly that large.  Slot t * S + s holds
 * record s of task t -- in BOTH t = 2q + strand, as for kfmi_search_strands --
 * as (L, R) in `intervals` and (start, len) in `spans`; the slots a task does
 * not use are written as zeros in both by the search itself, whatever they held.
 * Task-major, so a slice of reads is a contiguous slice of results.  Two
 * handles, so kfmi_locate(index, intervals, max_occ, ..) works unchanged: it
 * sees S * ns * num intervals, the empty ones without positions;
 * transferGPUtoCPU moves each handle.
 *   kfmi_search_seeds: the plain-counter task backends ("task", "task-mid") at
 * K = 1, 2, reads of 1 .. 256 bases with any m % K, every strand mode, fused
 * packing on or off, ASCII and KFMI_UPLOAD=packed uploads, one device.  The
 * jump-start and skip tables are used where the settings put them in effect
 * (each new segment may take them again) and never change a result.  Returns
 * KFMI_E_BAD_ARGUMENT for max_seeds outside 1 .. 8, an unknown `strands`,
 * handles of another size and reads over 256 bases; KFMI_E_NOT_IMPLEMENTED for
 * the coop and AltCounters backends, K = 3 / 4 and device-group handles.  A
 * refused call writes nothing.  kfmi_last_timing as for kfmi_search.  REV and
 * BOTH searches that take the pack launch (fused packing off, m % K != 0,
 * host-packed uploads) use the queries handle's strand words, so the rule of
 * kfmi_search_strands holds: not two of them on ONE queries handle at a time.
 *   kfmi_search_seeds_cpu: the same tasks on the host (searchIndexCPU's LF step
 * and remainder table; a temporary holds the reverse complements), index tags
 * 100 / 101; AltCounters images return KFMI_E_BAD_ARGUMENT.  nthreads as for
 * kfmi_search_cpu. */
int32_t kfmi_search_seeds(void *index, void *queries, void *intervals, void *spans,
                          uint32_t max_seeds, uint32_t strands);
int32_t kfmi_search_seeds_cpu(void *index, void *queries, void *intervals, void *spans,
                              uint32_t max_seeds, uint32_t strands, int32_t nthreads);

/* ---- verify seeds (not in the reference, which stops at intervals) -----------
 * The step a mapper takes after seeding: score the read at the text position
 * each seed implies and keep the best placement.  Tasks, their order and the
 * S = max_seeds slots per task are those of kfmi_search_seeds (ns = 2 for
 * BOTH, task 2q + strand; a REV task is the read P').  `intervals` and `spans`
 * are two results handles of S * ns * num entries as the seed search leaves
 * them on the device -- any caller-filled handles of that size are accepted
 * too -- and `hits` is a third handle of exactly ns * num entries, entry t the
 * record of task t.  With n the text's length, rows = n + 1, m the read length
 * and sa the text's suffix array (sa[0] = n, the '$' suffix):
 *   Candidates.  Slot s of task t with {L, R} and {start, len} gives the rows
 * L, L + 1, .. in row order, below min(R, rows, L + max_occ).  A slot
 * contributes nothing when R <= L, L >= rows, len == 0 or start + len > m.  Row
 * r gives p = sa[r] and the origin o = p - start.  The candidate is scored iff
 * sa[r] < rows, p >= start and o + m <= n; otherwise it is skipped and not
 * counted.
 *   Score: the number of j in [0, m) with base2index(P[j]) != code(T[o + j])
 * (N -> G, lowercase like uppercase, as everywhere).
 *   Record.  Over all scored candidates of the task, the minimum of (mism, o)
 * in lexicographic order; KFMI_HIT_MULTI iff two distinct origins attain the
 * minimal mism (two slots that point at one origin are one origin).  If that
 * mism <= max_mism: x = o, y = mism | MULTI | scored << 20, scored the number
 * of scored candidates (at most 8 * 256).  Otherwise, and with no scored
 * candidate: x = KFMI_HIT_NONE, y = scored << 20.  The result depends on no
 * evaluation order, and every entry of `hits` is written whatever it held.
 *   Arguments: max_seeds 1 .. 8; strands FWD, REV or BOTH; max_occ 1 ..
 * KFMI_VERIFY_MAX_OCC (there is no "all": a poly-A interval must not make one
 * lane loop millions of times); max_mism any value (>= m accepts everything);
 * exact handle sizes; reads of at most 256 bases -- else KFMI_E_BAD_ARGUMENT.
 *   kfmi_verify_seeds covers the device copies the seed search covers ("task",
 * "task-mid", K = 1, 2, one device) and needs the queries' ASCII rows on the
 * device.  KFMI_E_NOT_IMPLEMENTED: the coop and AltCounters backends, K = 3 / 4,
 * device-group handles, KFMI_UPLOAD=packed queries, and a device copy whose
 * index fails the text jump's exactness check.  A refused call writes nothing.
 *   Tables: the call reads the flat tables [sa | isa | text] of the text jump
 * and never the FM index.  Where the device copy has none it builds them, on
 * the path kfmi_set_jump(1) takes at a first search and whatever the calling
 * thread's jump setting is; KFMI_E_DEVICE_ALLOC when they do not fit.  Tables
 * built this way stay with the device copy like any others: later searches
 * under the auto setting may use them, with the same results.
 *   kfmi_last_timing: total, 0, the verify kernel (ms).
 *   kfmi_verify_seeds_cpu: the same definition on the host (OpenMP, nthreads as
 * for kfmi_search_cpu), on the text as ASCII and a full suffix array of rows =
 * n + 1 entries -- the one kfmi_device_jump_tables returns, or kfmi_index_sa at
 * rate 1; entries >= rows are rows without a suffix.  It reads and writes the
 * handles' host arrays and needs neither an index nor a device.
 *   kfmi_results_to_device copies the host array of a results handle that is on
 * a device (transferCPUtoGPU, which zeroes the device array and copies nothing
 * up) to that device array: the way caller-filled `intervals` and `spans` reach
 * the device.  KFMI_E_NOT_ON_DEVICE before the transfer, KFMI_E_NOT_IMPLEMENTED
 * for device-group handles. */
#define KFMI_HIT_NONE         0xFFFFFFFFu
#define KFMI_HIT_MISM_MASK    0x0000FFFFu   /* y bits 0-15: mismatches of the reported hit            */
#define KFMI_HIT_MULTI        0x00010000u   /* y bit 16: >= 2 distinct origins attain that count       */
#define KFMI_HIT_SCORED_SHIFT 20            /* y bits 20-31: candidates scored (<= 8 * 256 = 2048)     */
#define KFMI_VERIFY_MAX_OCC   256u
int32_t kfmi_verify_seeds(void *index, void *queries, void *intervals, void *spans, void *hits,
                          uint32_t max_seeds, uint32_t strands, uint32_t max_occ, uint32_t max_mism);
int32_t kfmi_verify_seeds_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows,
                              void *queries, void *intervals, void *spans, void *hits,
                              uint32_t max_seeds, uint32_t strands, uint32_t max_occ, uint32_t max_mism,
                              int32_t nthreads);
int32_t kfmi_results_to_device(void *results);

/* ---- align seeds (not in the reference, which stops at intervals) ------------
 * "verify seeds" with a banded edit distance in place of the Hamming count, so
 * that a read with an inserted or deleted base is placed too.  Tasks, their
 * order, the S = max_seeds slots per task, the strand modes, the three handles
 * and their sizes, the candidates of a slot (rows L, L + 1, .. below min(R,
 * rows, L + max_occ)), the ignored-slot forms, which candidates are scored
 * (sa[r] < rows, p >= start, o + m <= n with o = p - start) and the `scored`
 * count are those of "verify seeds".  What changes is a candidate's score and
 * what x and KFMI_HIT_MULTI mean.
 *   Score of a scored candidate with origin o under band w, 0 <= w <=
 * KFMI_ALIGN_MAX_BAND.  Cells are (i, d) with 0 <= i <= m and -w <= d <= w;
 * cell (i, d) stands at text position j = o + i + d and is valid iff 0 <= j <=
 * n.  A(i, d) is the least number of edits that align P[i .. m) to text
 * beginning at j and ending anywhere inside the band: A(m, d) = 0 for valid d,
 * and for i < m and a valid cell the minimum, over the transitions that exist,
 * of
 *     A(i+1, d)   + [base2index(P[i]) != code(T[j])]   when j < n,
 *     A(i+1, d-1) + 1   when d - 1 >= -w      (a read base with no text base),
 *     A(i, d+1)   + 1   when d + 1 <= w and j < n      (a text base skipped);
 * invalid cells are +infinity.  The candidate's edits are e = min over d of
 * A(0, d), its begin positions every o + d with A(0, d) = e.  d = 0 is valid in
 * every row of a scored candidate, so e never exceeds the Hamming count, and
 * with w = 0 it is the Hamming count.  (The prefix form -- a free start in the
 * band, rows 0 -> m, the minimum at row m -- gives the same e; the suffix form
 * is the definition because its last row carries the begin positions.)
 *   Record.  E is the least e over the task's scored candidates, B_min and
 * B_max the smallest and the largest begin position over all (candidate, d)
 * pairs that attain E.  If E <= max_edits: x = B_min, y = E | KFMI_HIT_MULTI
 * iff B_max - B_min > 2w | scored << 20.  Otherwise, and with no scored
 * candidate: x = KFMI_HIT_NONE, y = scored << 20.  Nothing depends on the
 * evaluation order.  Two seeds on either side of one indel imply origins that
 * differ by the indel's length and lead to one begin position, which is why
 * MULTI looks at the spread of begin positions and not at distinct origins.
 * With band = 0 every record equals kfmi_verify_seeds' bit for bit.
 *   What a record does not hold: the alignment itself (no traceback, no CIGAR)
 * and its end position, which kfmi_align_paths forms from x; costs are 1 per substitution, inserted or deleted
 * base; an indel longer than the band is not found.
 *   Arguments, coverage, refusals, the tables built on demand and
 * kfmi_last_timing (total, 0, the align kernel) are exactly those of
 * kfmi_verify_seeds; band > KFMI_ALIGN_MAX_BAND is KFMI_E_BAD_ARGUMENT;
 * max_edits may be any value.  A refused call writes nothing.
 *   kfmi_align_seeds_cpu: the same definition on the host, with the arguments
 * of kfmi_verify_seeds_cpu. */
#define KFMI_ALIGN_MAX_BAND 15u
int32_t kfmi_align_seeds(void *index, void *queries, void *intervals, void *spans, void *hits,
                         uint32_t max_seeds, uint32_t strands, uint32_t max_occ,
                         uint32_t band, uint32_t max_edits);
int32_t kfmi_align_seeds_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows,
                             void *queries, void *intervals, void *spans, void *hits,
                             uint32_t max_seeds, uint32_t strands, uint32_t max_occ,
                             uint32_t band, uint32_t max_edits, int32_t nthreads);

/* ---- align paths (not in the reference, which stops at intervals) ------------
 * The alignment itself: for every task the CIGAR and the end position of its
 * placement at a given begin position, under the costs and the band of "align
 * seeds".  Tasks, their order and the strand modes are those of
 * kfmi_align_seeds (ns = 2 for BOTH, task t = 2q + strand; a REV task is the
 * read P', and its CIGAR is in P' order against the forward text).
 *   Handles.  `hits`: a results handle of ns * num entries as kfmi_align_seeds
 * or kfmi_verify_seeds leaves it on the device -- caller-filled handles sent up
 * with kfmi_results_to_device are accepted too; only word x of an entry is
 * read, the begin position B or KFMI_HIT_NONE.  `paths`: a handle of exactly
 * ns * num entries.  `cigars`: a handle of exactly ns * num * C entries, C =
 * cigar_entries in 1 .. KFMI_PATH_MAX_ENTRIES; task t owns the entries t * C ..
 * t * C + C - 1, which are 2C u32 words, one per run.  Every entry of `paths`
 * and `cigars` is written, whatever it held before.
 *   Definition.  n is the text's length, m the read length, w = band with 0 <=
 * w <= KFMI_ALIGN_MAX_BAND.  A task has no path when x = KFMI_HIT_NONE, n < m,
 * B > n, or B - c > w, where c = min(B, n - m) is the band's centre.  Otherwise
 * cells are (i, d) with 0 <= i <= m and -w <= d <= w; cell (i, d) stands at
 * text position j = c + i + d and is valid iff 0 <= j <= n.  A(i, d) is the
 * least number of edits that align P[i .. m) to text beginning at j and ending
 * anywhere inside the band: A(m, d) = 0 for valid d, and for i < m and a valid
 * cell the minimum, over the transitions that exist, of
 *     A(i+1, d)   + [base2index(P[i]) != code(T[j])]   when j < n,
 *     A(i+1, d-1) + 1   when d - 1 >= -w      (a read base with no text base),
 *     A(i, d+1)   + 1   when d + 1 <= w and j < n      (a text base skipped);
 * invalid cells are +infinity.  That is the table of "align seeds" with o := c.
 * With d0 = B - c the task's edits are D = A(0, d0), which is finite; if D >
 * max_edits the task has no path.
 *   The path is one walk from (0, d0) with v = D.  While i < m, take the first
 * of these that exists and attains v (invalid cells attain nothing):
 *     1. text base skipped: d + 1 <= w, j < n and A(i, d+1) + 1 = v.
 *        Op D, d += 1, v -= 1.
 *     2. read base with no text base: d - 1 >= -w and A(i+1, d-1) + 1 = v.
 *        Op I, i += 1, d -= 1, v -= 1.
 *     3. diagonal: j < n and A(i+1, d) + [base2index(P[i]) != code(T[j])] = v.
 *        Op = or X, i += 1, v -= that bracket.
 * The walk stops when i = m: the end is free inside the band, so no D follows
 * the last read base.  Gaps come first, so a gap in a repeat sits at its
 * leftmost place in read order, the usual normal form.  The result depends on
 * no evaluation order.
 *   Record.  paths[t]: x = the end position c + m + d, one past the last text
 * base used; y = D | runs << KFMI_PATH_RUNS_SHIFT | KFMI_PATH_OVERFLOW, runs
 * the number of runs of the path (12 bits).  cigars: run r of the task is the
 * u32 word len << 4 | op with BAM's codes I = 1, D = 2, '=' = 7, X = 8, runs
 * in read order; unused words are 0 and no run has length 0.  A path of more
 * than 2C runs leaves every word of the task 0 and sets KFMI_PATH_OVERFLOW,
 * with `runs` the number needed and x and D as usual; a path has at most 2D +
 * 1 runs, so C >= max_edits + 1 never overflows.  No path: x = KFMI_HIT_NONE,
 * y = 0, every word 0.
 *   What holds of every record with a path that fits:
 *     the lengths of its =, X and I runs sum to m;
 *     B plus the lengths of its =, X and D runs is x;
 *     the lengths of its X, I and D runs sum to D;
 *     replaying the runs over P and T finds equal bases under = and different
 *     ones under X;
 *     with w = 0 the path is m diagonal ops and D is the Hamming count;
 *     if the hit came from kfmi_align_seeds at the same band with E <= w and
 *     B + m <= n, then D <= E: a path with E edits drifts at most E diagonals
 *     from its begin, so it lies in the band around c = B.  D < E is allowed:
 *     E is the best over the bands around the seeds' origins, and the band
 *     around B may hold a cheaper path that those do not.
 *   What a record does not hold: affine gap costs, indels longer than the band
 * and soft clipping.
 *   Arguments, coverage, refusals.  The tables built on demand are those of
 * kfmi_align_seeds; only the 2-bit text of the text jump's tables is read.
 * Coverage: "task" and "task-mid", K = 1, 2, one device, the queries' ASCII
 * rows on the device, reads of at most 256 bases.  KFMI_E_BAD_ARGUMENT: band >
 * KFMI_ALIGN_MAX_BAND, C outside 1 .. KFMI_PATH_MAX_ENTRIES, an unknown
 * `strands`, handles of another size; KFMI_E_NOT_IMPLEMENTED: the cases of
 * kfmi_align_seeds.  A refused call writes nothing.  max_edits may be any value.
 *   The kernel keeps three words per row and task in a device workspace that
 * the call allocates and frees (KFMI_E_DEVICE_ALLOC when it does not fit), and
 * launches in chunks of tasks so that the workspace stays under 1 GiB.
 * kfmi_set_path_chunk(tasks) is a process-wide test knob: chunks of `tasks`
 * tasks, rounded up to a multiple of 64, whatever the batch; 0 = by the cap.
 * No result depends on it.
 *   kfmi_last_timing: total, 0, the sum of the paths kernel's launches (ms);
 * both are device time, so the workspace's allocation is in neither.
 *   kfmi_align_paths_cpu: the same definition on the host as a plain full-band
 * table and the walk (OpenMP, nthreads as for kfmi_search_cpu), on the text as
 * ASCII and the handles' host arrays; no suffix array, no index, no device. */
#define KFMI_PATH_EDITS_MASK  0x0000FFFFu   /* y bits 0-15: the path's edits D                         */
#define KFMI_PATH_RUNS_SHIFT  16            /* y bits 16-27: the runs of the path (<= 2 D + 1)         */
#define KFMI_PATH_RUNS_MASK   0x00000FFFu
#define KFMI_PATH_OVERFLOW    0x80000000u   /* y bit 31: more than 2C runs, no word written            */
#define KFMI_PATH_MAX_ENTRIES 32u
int32_t kfmi_align_paths(void *index, void *queries, void *hits, void *paths, void *cigars,
                         uint32_t strands, uint32_t band, uint32_t max_edits, uint32_t cigar_entries);
int32_t kfmi_align_paths_cpu(const char *text, uint64_t n, void *queries, void *hits, void *paths, void *cigars,
                             uint32_t strands, uint32_t band, uint32_t max_edits, uint32_t cigar_entries,
                             int32_t nthreads);
int32_t kfmi_set_path_chunk(uint64_t tasks);

/* ---- place windows / pairs (not in the reference, which stops at intervals) --
 * The two steps a paired-end mapper takes after the single-end pass: place a
 * read inside a text window without any seed, and choose per pair of reads the
 * concordant combination of placements.  Three calls: kfmi_mate_windows forms
 * the window each task's mate implies, kfmi_place_windows places every task in
 * its window, kfmi_pair_hits chooses.  Every record has the `hits` format of
 * "verify seeds" (x, y; KFMI_HIT_NONE, KFMI_HIT_MULTI), so kfmi_align_paths
 * takes each of them as it is.
 *
 *   kfmi_place_windows.  Tasks, their order and the strand modes are those of
 * kfmi_align_seeds (ns = 2 for BOTH, task t = 2q + strand; a REV task is the
 * read P').  `windows` and `hits` are results handles of exactly ns * num
 * entries.  Entry t of `windows` is (lo, len) and names the begin positions lo,
 * lo + 1, .., lo + len - 1; len = 0 means the task places nothing.  A `windows`
 * handle may be caller-filled and sent up with kfmi_results_to_device, or left
 * on the device by kfmi_mate_windows.  With n the text's length and m the read
 * length:
 *   Table.  A(i, j), 0 <= i <= m, 0 <= j <= n, is the least number of unit-cost
 * edits that align P[i .. m) to text beginning at j and ending anywhere at or
 * before n: A(m, j) = 0 for every j, A(i, n) = m - i, and for i < m, j < n the
 * minimum of
 *     A(i+1, j+1) + [base2index(P[i]) != code(T[j])],
 *     A(i+1, j)   + 1      (a read base with no text base),
 *     A(i,   j+1) + 1      (a text base skipped).
 * e(b) = A(0, b) for 0 <= b <= n; in particular e(n) = m and e(b) <= m.  There
 * is no band: the path drifts as far as its edits allow, so an indel of any
 * length up to max_edits is found.
 *   Record.  The begin positions of task t are the b with lo <= b < lo + len
 * and b <= n.  E is the least e(b) over them, B_min and B_max the smallest and
 * the largest b that attain E.  If a begin position exists and E <= max_edits:
 * x = B_min, y = E | KFMI_HIT_MULTI iff B_max > B_min.  Otherwise x =
 * KFMI_HIT_NONE, y = 0.  Bits 20 to 31 of y are 0 -- there are no candidates to
 * count.  Every entry of `hits` is written, and nothing depends on evaluation
 * order.
 *   Scan bound.  A placement with e edits that begins at b uses at most m + e
 * text bases, so with K = min(max_edits, m) the call may treat the text as
 * ending at min(n, lo + len - 1 + m + K): every e(b) <= max_edits keeps its
 * value and every other one stays above max_edits, so no record changes.  The
 * cost of a task is (len + m + K) columns of m cells, whatever n is.
 *   Into kfmi_align_paths.  That call reads word x alone and needs its band
 * given explicitly; a placement found here whose path drifts more than that
 * band from its begin position is then simply not reproduced there (its record
 * is the banded table's, or no path).  For a record with E <= band and B + m <=
 * n the path's edits D satisfy D <= E, by the argument given there.
 *   Refusals.  len > KFMI_WINDOW_MAX_LEN in any entry: KFMI_E_BAD_ARGUMENT and
 * nothing is written.  kfmi_place_windows decides that on the device -- a check
 * kernel raises a flag that the placing kernel reads before it writes and the
 * host reads after the call's one wait -- so windows left on the device never
 * visit the host; kfmi_place_windows_cpu checks the host array first.  Unknown
 * `strands`, handles of another size, reads over 256 bases:
 * KFMI_E_BAD_ARGUMENT.  Coverage and KFMI_E_NOT_IMPLEMENTED are exactly those
 * of kfmi_align_seeds ("task" and "task-mid", K = 1, 2, one device, the reads'
 * ASCII rows on the device), the tables built on demand too; only the 2-bit
 * text of the text jump's tables is read.  max_edits may be any value.  A
 * refused call writes nothing.  kfmi_last_timing: total, 0, the window kernel.
 *   kfmi_place_windows_cpu: the same definition on the host as a plain table
 * per task (OpenMP, nthreads as for kfmi_search_cpu) on the text as ASCII and
 * the handles' host arrays; no suffix array, no index, no device.
 *
 *   kfmi_mate_windows.  Reads 2p and 2p + 1 are mates (interleaved, as in
 * interleaved FASTQ), all of one length m = read_len, and `hits` and `windows`
 * have 2 * num entries in BOTH order, num even.  The layout is forward-reverse:
 * a FWD task that begins at B_f and a REV task that begins at B_r form the
 * fragment frag = B_r + m - B_f, and the two are concordant iff B_r >= B_f and
 * min_frag <= frag <= max_frag.  The mate task of t = 2q + s is u = 2 (q ^ 1) +
 * (s ^ 1) = t ^ 3.  If hits[u].x is KFMI_HIT_NONE the window of t is (0, 0).
 * Otherwise, with B_u = hits[u].x, the begin positions concordant with it are
 *     [B_u + min_frag - m, B_u + max_frag - m]   when s is REV,
 *     [B_u + m - max_frag, B_u + m - min_frag]   when s is FWD,
 * clipped to [0, n] in 64-bit signed arithmetic; (0, 0) if nothing is left,
 * else (lo, hi - lo + 1).  mode 0 also writes (0, 0) when the task's own hit
 * exists and is concordant with hits[u] already, so that only the tasks that
 * need it are rescued; mode 1 writes the window regardless.  Required: 1 <= m
 * <= 256, m <= min_frag <= max_frag, max_frag - min_frag + 1 <=
 * KFMI_WINDOW_MAX_LEN, mode 0 or 1, an entry count that is a multiple of 4 and
 * equal in both handles -- else KFMI_E_BAD_ARGUMENT.  n comes from the index;
 * kfmi_mate_windows_cpu takes it as an argument and works on the host arrays.
 *
 *   kfmi_pair_hits.  `hits` (each task's own record), `rescued` (the records
 * kfmi_place_windows formed in the mate windows) and `paired` have 2 * num
 * entries in BOTH order.  Per pair p with reads a = 2p and b = 2p + 1:
 * orientation k = 0 is (f, r) = (task(a, FWD), task(b, REV)), k = 1 is
 * (task(b, FWD), task(a, REV)); each side takes its own hit (source 0) or its
 * rescued record (source 1).  A combination (k, s_f, s_r) is admissible iff
 * both records exist, they are concordant and s_f + s_r <= 1 (a rescued record
 * is anchored on the mate's own hit, so two rescued records anchor nothing).
 * The admissible combination with the lexicographically least (E_f + E_r, s_f +
 * s_r, k, B_f, B_r, s_f) is chosen -- the last key only separates two
 * combinations that reach the same two places with the sources swapped.  Then
 * paired[f] and paired[r] are x = B, y = E | the source record's KFMI_HIT_MULTI
 * bit | KFMI_PAIR_PROPER | KFMI_PAIR_RESCUED iff that side's source is 1, and
 * the pair's other two tasks are (KFMI_HIT_NONE, 0).  With no admissible
 * combination each read alone keeps the least (E, strand) of its own two hits,
 * without KFMI_PAIR_PROPER; its other task, or both if it has no hit, is
 * (KFMI_HIT_NONE, 0).  Rescued records are never used unpaired.  Bits 20 to 31
 * of y are 0.  Every entry is written; nothing depends on evaluation order.
 * kfmi_align_paths(.., paired, .., KFMI_STRAND_BOTH, ..) then gives the CIGARs
 * of exactly the chosen tasks.  Arguments as for kfmi_mate_windows; three
 * distinct handles of one size.
 *   Both record calls run on the device the index is on, refuse what
 * kfmi_align_seeds refuses (KFMI_E_NOT_IMPLEMENTED: coop and AltCounters
 * backends, K = 3 / 4, device groups; KFMI_E_NOT_ON_DEVICE) and set
 * kfmi_last_timing to total, 0, their kernel.
 *   What the three calls do not do: reads of unequal length within a pair,
 * layouts other than forward-reverse, affine gaps, soft clipping, the pair
 * fields of a SAM line (see "SAM lines"). */
#define KFMI_WINDOW_MAX_LEN 4096u
#define KFMI_PAIR_PROPER  0x00020000u   /* y bit 17: the record is one side of the pair's chosen combination */
#define KFMI_PAIR_RESCUED 0x00040000u   /* y bit 18: that side is the record placed in the mate's window    */
int32_t kfmi_place_windows(void *index, void *queries, void *windows, void *hits,
                           uint32_t strands, uint32_t max_edits);
int32_t kfmi_place_windows_cpu(const char *text, uint64_t n, void *queries, void *windows, void *hits,
                               uint32_t strands, uint32_t max_edits, int32_t nthreads);
int32_t kfmi_mate_windows(void *index, void *hits, void *windows, uint32_t read_len,
                          uint32_t min_frag, uint32_t max_frag, uint32_t mode);
int32_t kfmi_mate_windows_cpu(uint64_t n, void *hits, void *windows, uint32_t read_len,
                              uint32_t min_frag, uint32_t max_frag, uint32_t mode);
int32_t kfmi_pair_hits(void *index, void *hits, void *rescued, void *paired, uint32_t read_len,
                       uint32_t min_frag, uint32_t max_frag);
int32_t kfmi_pair_hits_cpu(void *hits, void *rescued, void *paired, uint32_t read_len,
                           uint32_t min_frag, uint32_t max_frag);

/* ---- second placement / mapping quality (not in the reference) ---------------
 * How much worse a task's next-best place is than the one kfmi_align_seeds
 * reported: the gap every consumer of a mapper filters on.  A second pass over
 * the same candidates, because "second-best" has to mean "best outside the
 * neighbourhood of the reported begin position" -- else the two seeds either
 * side of one indel would count as two places (see KFMI_HIT_MULTI under "align
 * seeds") -- and that position is known only after every candidate was scored.
 *
 *   kfmi_align_second.  The tasks and their order, the S = max_seeds slots per
 * task, the strand modes, the handle sizes of `intervals` and `spans`, the
 * ignored-slot forms, the candidates of a slot (rows L, L + 1, .. below min(R,
 * rows, L + max_occ)), which candidates are scored, the table A(i, d) and w =
 * band are those of "align seeds".
 *   Handles.  `hits`: ns * num entries, of which only word x is read: X, the
 * begin position, or KFMI_HIT_NONE; left on the device by kfmi_align_seeds or
 * caller-filled through kfmi_results_to_device.  `second`: exactly ns * num
 * entries; every entry is written, whatever it held.
 *   Definition for task t with X != KFMI_HIT_NONE.  A pair (scored candidate
 * with origin o, d in [-w, w]) whose cell (0, d) is valid begins at b = o + d.
 * The pair is far iff |b - X| > 2w, in signed 64-bit arithmetic.  E2 is the
 * least A(0, d) over the far pairs, B2_min and B2_max the smallest and the
 * largest far b that attain E2.  `counted` is the number of scored candidates
 * with |o - X| > w: exactly the candidates that can own a far cell; the others
 * may be skipped without a dynamic programme.  TRUNC is set iff some slot of
 * the task that is not ignored has min(R, rows) - L > max_occ, so that rows of
 * the interval were never looked at.
 *   Record.  If a far pair exists and E2 <= max_second: x = B2_min, y = E2 |
 * KFMI_HIT_MULTI iff B2_max - B2_min > 2w | KFMI_SECOND_TRUNCATED iff TRUNC |
 * counted << 20.  Otherwise x = KFMI_HIT_NONE, y = (KFMI_SECOND_TRUNCATED iff
 * TRUNC) | counted << 20.  X = KFMI_HIT_NONE: the record is (KFMI_HIT_NONE, 0).
 * KFMI_SECOND_TRUNCATED is y bit 19; bits 17 and 18 are the pair flags.
 * Nothing depends on the evaluation order.
 *   What then holds.  If `hits` came from kfmi_align_seeds with the same slots,
 * max_occ and band, with record edits E, and max_second >= E:
 *     E2 >= E wherever a second exists;
 *     E2 = E  <=>  the hit carries KFMI_HIT_MULTI (B_max - B_min > 2w is the
 *     same test, because X = B_min);
 *     counted <= scored;
 *     with band 0, E2 is the least Hamming count over origins != X.
 *   Arguments, coverage, refusals, the tables built on demand and
 * kfmi_last_timing (total, 0, this kernel) are exactly those of
 * kfmi_align_seeds, with `hits` and `second` two more distinct handles on the
 * index's device; band > KFMI_ALIGN_MAX_BAND is KFMI_E_BAD_ARGUMENT; max_second
 * may be any value.  A refused call writes nothing.
 *   What a second does not see: a place no seed slot leads to.  The greedy
 * seed search gives an exactly matching read one seed, the whole read, so a
 * near-copy of its locus never becomes a candidate.  Caller-filled slots of
 * fixed-length pieces of the read (the binding's piece_seeds, built from
 * kfmi_search / kfmi_search_strands and kfmi_results_to_device) close that.
 *   kfmi_align_second_cpu: the same definition on the host as a plain full
 * table per candidate, with the arguments of kfmi_align_seeds_cpu plus `second`
 * and max_second; no index, no device.
 *
 *   kfmi_map_quality.  A streaming call on records alone.  `hits`, `second` and
 * `quals` have ns * num entries each (an even number in BOTH mode), and every
 * entry of `quals` is written.  For task t with hits[t] = (X, y) and E = y &
 * KFMI_HIT_MISM_MASK:
 *     X = KFMI_HIT_NONE: the record is (0, 0).
 *     C is the least of: E2 of second[t] if its x != KFMI_HIT_NONE; in BOTH
 *     mode only, the edits of hits[t ^ 1] if that record exists (the read's
 *     other strand competes with it); max_second + 1.
 *     gap = max(C - E, 0), except in BOTH mode when hits[t ^ 1] has the same
 *     edits and t is the REV task: then gap = 0.  (Equal edits give both tasks
 *     gap 0 already; the clause keeps the rule explicit.)  gap is formed in 64
 *     bits and its word saturates at 2^32 - 1.
 *     q = min(KFMI_MAPQ_MAX, KFMI_MAPQ_PER_EDIT * gap).
 *     If second[t] carries KFMI_SECOND_TRUNCATED, or in BOTH mode second[t ^ 1]
 *     does, q = min(q, KFMI_MAPQ_TRUNCATED).
 *     Record: x = q, y = gap.
 * The constants 60, 10 and 3 are this project's definition and no claim of
 * calibration against any other mapper's mapping quality.
 *   Refusals are those of kfmi_pair_hits: three distinct handles of one size on
 * the index's device, an unknown `strands` or an odd size in BOTH mode is
 * KFMI_E_BAD_ARGUMENT; KFMI_E_NOT_IMPLEMENTED for the coop and AltCounters
 * backends, K = 3 / 4 and device groups; KFMI_E_NOT_ON_DEVICE.
 * kfmi_last_timing: total, 0, the kernel.  kfmi_map_quality_cpu works on the
 * handles' host arrays.
 *   What neither call does: the quality of a pair (where the second-best
 * combination matters, not only the second-best side), affine gaps, soft
 * clipping. */
#define KFMI_SECOND_TRUNCATED 0x00080000u   /* y bit 19: a slot held more rows than max_occ looked at        */
#define KFMI_MAPQ_MAX         60u
#define KFMI_MAPQ_PER_EDIT    10u
#define KFMI_MAPQ_TRUNCATED   3u
int32_t kfmi_align_second(void *index, void *queries, void *intervals, void *spans, void *hits, void *second,
                          uint32_t max_seeds, uint32_t strands, uint32_t max_occ,
                          uint32_t band, uint32_t max_second);
int32_t kfmi_align_second_cpu(const char *text, uint64_t n, const uint32_t *sa, uint64_t rows,
                              void *queries, void *intervals, void *spans, void *hits, void *second,
                              uint32_t max_seeds, uint32_t strands, uint32_t max_occ,
                              uint32_t band, uint32_t max_second, int32_t nthreads);
int32_t kfmi_map_quality(void *index, void *hits, void *second, void *quals,
                         uint32_t strands, uint32_t max_second);
int32_t kfmi_map_quality_cpu(void *hits, void *second, void *quals, uint32_t strands, uint32_t max_second);

/* ---- SAM lines (not in the reference, which stops at intervals) --------------
 * The text form of a batch: one SAM record per read from the records the calls
 * above leave on the device, with positions as a sequence name and a 1-based
 * coordinate and with NM and MD, so that a consumer needs neither this library
 * nor the text.
 *
 *   Contig table.  kfmi_contigs_create(names, begins, lengths, count, &contigs):
 * `names` holds `count` NUL-terminated names back to back, contig i is the text
 * positions [begins[i], begins[i] + lengths[i]).  KFMI_E_BAD_ARGUMENT, and
 * nothing is created, for count = 0; a name that is empty, longer than 254
 * bytes or holds a byte outside 33 .. 126; a length of 0; begins[i] +
 * lengths[i] > begins[i + 1] (contigs ascend and do not overlap; gaps between
 * them are allowed, because the `ref` loader leaves header bytes in the text)
 * or a contig ending past 2^32 - 1.  The table's end is checked against the
 * text's length by the call that uses it.  kfmi_sam_header(contigs, buf, cap)
 * returns the bytes of "@HD\tVN:1.6\tSO:unknown\n" followed by one
 * "@SQ\tSN:<name>\tLN:<length>\n" per contig and writes them to buf if cap
 * holds them (no terminator); a negative error code for no table.  The device
 * copy of the table is made by the first kfmi_sam_lines that uses it, on that
 * index's device -- begins, lengths, the names as one byte array with a u32
 * offset per contig -- and freed with the table; a table serves one device.
 *
 *   kfmi_sam_lines.  The handles, the strand modes and the task numbering are
 * those of kfmi_align_paths: `hits`, `paths` and, where given, `quals` have ns *
 * num entries, `cigars` ns * num * C with C = cigar_entries; `band` is the band
 * the paths were made with.  Of `hits` only word x is read (the begin position
 * B), of `paths` x (the end), D = y & KFMI_PATH_EDITS_MASK, the runs and
 * KFMI_PATH_OVERFLOW, of `quals` only word x.  quals may be NULL.
 *   Status of task t, n the text's length, m the read length, w = band.  The
 * first of these that holds:
 *     NONE      paths[t].x = KFMI_HIT_NONE.
 *     OVERFLOW  paths[t].y carries KFMI_PATH_OVERFLOW.
 *     SPAN      no contig i has begins[i] <= B and end <= begins[i] +
 *               lengths[i]; or end <= B (a path of insertions only uses no
 *               text base); or the placement does not lie in the window of its
 *               band: n < m, B > n, B - c > w or end > c + m + w with c =
 *               min(B, n - m) -- which a path made at another band may do, and
 *               which covers end - B > m + 2w; or its runs are not between 1
 *               and 2C runs of I, D, = or X, each of at least one base, whose
 *               =, X and I lengths sum to m and whose =, X and D lengths sum
 *               to end - B -- which no record of kfmi_align_paths does.
 *     OK        otherwise; its contig is the i above, found by a binary search
 *               over begins.
 *   One line per read, in read order, each ending in "\n"; offsets[q] is where
 * read q's line begins, offsets[num] the total.  With one strand the read's
 * task is its only task.  In BOTH mode it is chosen among the read's OK tasks:
 * the one with fewer path edits D, the FWD task on a tie.
 *   A mapped line (the read's task is OK), fields separated by one tab:
 *     QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ * NM:i:<D> MD:Z:<md>
 *   QNAME: name_base + q in decimal.  FLAG: 0, or 16 for a REV task.  RNAME:
 * the contig's name.  POS: B - begins[i] + 1.  MAPQ: min(quals[t].x, 254), 255
 * when quals is NULL.  CIGAR: the task's runs in order as <len><op> with the
 * character "MIDNSHP=X"[op]; under KFMI_SAM_CIGAR_M every maximal sequence of
 * adjacent = and X runs is one M run of the summed length.  SEQ: "ACGT"[code]
 * of the task's code words in the order they were aligned, which for a REV
 * task is the reverse complement, as SAM wants it beside flag 16.  MD: with a
 * counter c = 0, over the runs: = adds its length to c; I does nothing; X
 * writes, per base, c in decimal and the text's letter at that position, then
 * c = 0; D writes c, "^" and the run's text letters, then c = 0; at the end c
 * is written.  Runs 3= 1X 1D 4= give "3A0^C4", a leading X "0A..", two adjacent
 * mismatches "..A0C..".  Text letters are "ACGT"[code] of the 2-bit text.
 *   An unmapped line (no OK task):
 *     QNAME 4 * 0 0 * * 0 0 SEQ * YU:i:<r>
 * with SEQ the read as given (the FWD form) and r the largest status code
 * among the read's tasks, NONE = 0, OVERFLOW = 1, SPAN = 2.
 *   Nothing depends on the evaluation order; kfmi_sam_lines_cpu writes the
 * same bytes from the handles' host arrays and the ASCII text (OpenMP over
 * reads, a length pass, a prefix sum, a write pass; no index, no device).
 *   Limits.  SEQ is in the mapped alphabet: base2index of the read's bytes, so
 * a read's N appears as G, consistently with the = and X of its CIGAR; read
 * names and the original letters are not kept.  No base qualities (QUAL is
 * "*").  No pair fields: RNEXT, PNEXT and TLEN are "*", 0, 0 and flags 1, 2,
 * 32, 64 and 128 are never set, whatever kfmi_pair_hits chose.  A placement
 * that crosses a contig's edge is unmapped (SPAN), not clipped.  No BAM.
 *   Arguments, coverage, refusals.  Coverage and the tables built on demand are
 * those of kfmi_align_paths; `hits`, `paths`, `cigars` and `quals` are distinct
 * handles on the index's device.  KFMI_E_BAD_ARGUMENT: what kfmi_align_paths
 * refuses, an option bit other than KFMI_SAM_CIGAR_M, name_base + num
 * overflowing 64 bits, a table whose last contig ends past n, a table whose
 * device copy is on another device, sam = NULL.  A refused call writes nothing
 * and leaves *sam untouched.
 *   The handle.  kfmi_sam_num: the lines; kfmi_sam_bytes: their bytes;
 * kfmi_sam_offsets: num + 1 host values; kfmi_sam_text: the bytes on the host
 * (no terminator), copied from the device at the first call, NULL when that
 * fails; kfmi_sam_free frees host and device memory and clears the pointer.
 *   The device side is two kernels around a scan: a length pass on records
 * alone, an exclusive scan of the lengths (u32 -> u64), and a write pass with
 * the read in registers that formats a wave's lines into a 16 KB tile of LDS
 * and copies the tile out with 16-byte stores.
 * kfmi_set_sam_form(1) is a process-wide test knob that makes every lane write
 * its line straight to device memory instead; 0 = the tile.  No byte depends on
 * it.  kfmi_last_timing: total, 0, the sum of both passes and the scan (ms,
 * device time; the allocation of the text between them is not in it);
 * kfmi_sam_last_passes gives the calling thread's last call apart: the length
 * pass, the scan, the write pass. */
#define KFMI_SAM_CIGAR_M 1u   /* options bit 0: adjacent = and X runs merge into one M run */
int32_t kfmi_contigs_create(const char *names, const uint32_t *begins, const uint32_t *lengths,
                            uint32_t count, void **contigs);
int32_t kfmi_contigs_free(void **contigs);
int64_t kfmi_sam_header(void *contigs, char *buf, uint64_t cap);
int32_t kfmi_sam_lines(void *index, void *queries, void *contigs, void *hits, void *paths, void *cigars,
                       void *quals, uint32_t strands, uint32_t cigar_entries, uint32_t band,
                       uint32_t options, uint64_t name_base, void **sam);
int32_t kfmi_sam_lines_cpu(const char *text, uint64_t n, void *queries, void *contigs, void *hits, void *paths,
                           void *cigars, void *quals, uint32_t strands, uint32_t cigar_entries, uint32_t band,
                           uint32_t options, uint64_t name_base, int32_t nthreads, void **sam);
uint64_t        kfmi_sam_num(void *sam);
uint64_t        kfmi_sam_bytes(void *sam);
const uint64_t *kfmi_sam_offsets(void *sam);
const char     *kfmi_sam_text(void *sam);
int32_t         kfmi_sam_free(void **sam);
int32_t         kfmi_set_sam_form(uint32_t form);
int32_t         kfmi_sam_last_passes(double *ms_length, double *ms_scan, double *ms_write);

/* ---- walk trace (tests and diagnosis; not in the reference, not timed) -------
 * The fused forward task kernel ends a walk early through three shortcuts --
 * the jump start, the skip table and the text jump (DESIGN.md 5a .. 5a''') --
 * and each of them checks itself: a lookup that does not apply leaves the lane
 * walking, so a shortcut that never fires returns the same intervals as one
 * that always does.  kfmi_search_trace runs the search kfmi_search would run on
 * the same resident handles under the calling thread's settings -- the same
 * tables, the same fetch form, the same launch rules, through the same host
 * code -- with the traced instantiation of the same kernel body, writes the
 * intervals into `results` as kfmi_search does, and copies one record of four
 * words per read to the host array `trace` (4 * num words, read q at 4 * q):
 *   word 0  what the walk took: bits 0-15 the ordinary K-steps, bits 16-23 the
 *           skip lookups that matched (each covers 16 / K steps), bits 24-31
 *           those that did not (a lane stops looking up after its first);
 *   word 1  the text jump, 0 when the lane never tried one (it tries at most
 *           once): bit 0 tried; bit 1 the window and the ISA entry came from a
 *           line of the line table (else from the flat tables; only set when
 *           the loads were issued, i.e. not on KFMI_TRACE_JUMP_REFUSED); bits
 *           2-3 the outcome, KFMI_TRACE_JUMP_*: TAKEN, REFUSED before the loads
 *           (the row holds no text position, or fewer bases precede it than are
 *           left), DIFFERED (the window is not the read's remaining bases),
 *           BAD_ISA (the ISA entry is no row; never on a valid table); bits
 *           4-15 the K-step position `pos` at which it tried; bits 16-31 the
 *           bases left there, (steps - pos) * K;
 *   word 2  bits 0-30 the K-steps the jump start covered: 0, or the table's
 *           step count; bit 31 (KFMI_TRACE_START_FOLDED) the lane's jump used
 *           the text position its jump-start entry carried (a folded table,
 *           kfmi_set_ftab_fold), so it issued no SA load;
 *   word 3  IdxArgs::jump_split as the kernel received it, after the launch's
 *           read-length rule: bit 2 the gathers in four 16-lane groups, 0x100
 *           the line table in use, 0x200 its grouped form; 1 without the jump
 *           (the kernel's own bit for a folded jump-start table is not stored).
 * Steps + 16 / K * matches + word 2 is the K-step count of the read, unless the
 * jump was TAKEN (then pos + bases left / K is).
 *   Only what the text jump serves has a traced kernel: one device, the
 * plain-counter task backends ("task", "task-mid"), K = 1, 2, queries whose
 * ASCII rows are resident and fit the fused packing (at most 256 bases, fused
 * packing on).  Everything else -- device-group handles, the coop and
 * AltCounters backends, K = 3 / 4, packed or longer queries -- returns
 * KFMI_E_NOT_IMPLEMENTED and a null `trace` KFMI_E_BAD_ARGUMENT, before anything
 * runs or is written.  With every table off the traced launch still takes the
 * walk of the tables' kernel and records plain steps only. */
enum {
  KFMI_TRACE_STEP = 1u, KFMI_TRACE_SKIP_HIT = 1u << 16, KFMI_TRACE_SKIP_MISS = 1u << 24,
  KFMI_TRACE_JUMP_TRIED = 1u, KFMI_TRACE_JUMP_LINE = 2u,
  KFMI_TRACE_JUMP_OUT_SHIFT = 2, KFMI_TRACE_JUMP_POS_SHIFT = 4, KFMI_TRACE_JUMP_NB_SHIFT = 16,
  KFMI_TRACE_JUMP_TAKEN = 0, KFMI_TRACE_JUMP_REFUSED = 1, KFMI_TRACE_JUMP_DIFFERED = 2, KFMI_TRACE_JUMP_BAD_ISA = 3
};
#define KFMI_TRACE_START_FOLDED 0x80000000u
int32_t kfmi_search_trace(void *index, void *queries, void *results, uint32_t *trace);

/* The same for the strand and seed searches.  skip_walk inside the strand
 * kernels and seed_walk take the jump-start and skip tables as shortcuts that
 * check themselves too: a lookup that brings nothing, or never happens, leaves
 * the lane on the ordinary K-steps, which end on the very intervals and records
 * the lookup would have led to.  Both calls run the search their untraced
 * counterpart would run on the same resident handles under the calling thread's
 * settings -- the same tables, the same staging (fused or packed first), the
 * same fetch form, through the same host code -- with the traced instantiation
 * of the same kernel body, write their results as that call does, and copy one
 * record of four words per task to the host array `trace`, in results order
 * (task t at 4 * t; in BOTH t = 2q + strand).
 *
 * kfmi_search_strands_trace(index, queries, results, strands, trace): REV and
 * BOTH only (FWD is kfmi_search_trace; here KFMI_E_BAD_ARGUMENT).  Words 0 and
 * 2 are those of kfmi_search_trace; a strand search never takes the text jump,
 * so word 1 is 0 and bit 31 of word 2 is never set; word 3 is the launch
 * identity below.  A search that packs first while no skip table is in effect
 * runs the plain walk of the packed words, which has no traced form:
 * KFMI_E_NOT_IMPLEMENTED.
 *
 * kfmi_search_seeds_trace(index, queries, intervals, spans, max_seeds,
 * strands, trace): kfmi_search_seeds, and per task
 *   word 0  bits 0-15 the rounds in which the lane took an ordinary K-step --
 *           the step that ends a segment counts, and so does the step on a unit
 *           that does not occur on its own; bits 16-23 the skip lookups that
 *           matched; bits 24-31 those that did not;
 *   word 1  bits 0-15 the jump-start lookups whose decoded entry was not empty
 *           (each covers the table's step count), bits 16-31 those whose entry
 *           was empty;
 *   word 2  bits 0-15 the units that did not occur on their own (the remainder
 *           unit among them: its empty table entry costs no step); bits 16-23
 *           the records stored, before the zero fill of the unused slots;
 *   word 3  the launch identity.
 *
 * The launch identity (word 3 of both calls): bits 0-3 the fetch form of the
 * kernel that ran (its SPLIT template value: 8, 7, 4 or 1); bits 4-7 its code
 * registers / 8 (1 or 2); bits 8-11 the kernel, KFMI_TRACE_KERNEL_*; bits 12-15
 * IdxArgs::skip_split as the kernel received it (1 without a skip table, else
 * the table's size class; the gathers go out in four groups at 4); bit 16 the
 * jump-start table in use is folded; bits 24-31 the jump-start table's step
 * count, 0 without a table.
 *
 * Both refuse what has no traced kernel before anything runs or is written:
 * KFMI_E_NOT_IMPLEMENTED for the coop and AltCounters backends, K = 3 / 4 and
 * device-group handles, KFMI_E_BAD_ARGUMENT for a null `trace` and wherever the
 * untraced call gives it.  For tests and diagnosis; not timed. */
enum {
  KFMI_SEED_TRACE_START_HIT = 1u, KFMI_SEED_TRACE_START_EMPTY = 1u << 16, KFMI_SEED_TRACE_RECORDS_SHIFT = 16,
  KFMI_TRACE_ID_MAXW_SHIFT = 4, KFMI_TRACE_ID_KERNEL_SHIFT = 8, KFMI_TRACE_ID_SKIP_SPLIT_SHIFT = 12,
  KFMI_TRACE_ID_FTAB_FOLDED = 1u << 16, KFMI_TRACE_ID_FTAB_STEPS_SHIFT = 24,
  KFMI_TRACE_KERNEL_SEED = 0, KFMI_TRACE_KERNEL_SEED_STRANDS = 1, KFMI_TRACE_KERNEL_SEED_WORDS = 2,
  KFMI_TRACE_KERNEL_TASK_STRANDS = 3, KFMI_TRACE_KERNEL_TASK_WORDS_SKIP = 4,
  /* the forward kernels (kfmi_launch_plan alone names them: their records' word 3 is no launch identity): the
   * fused task kernel plain, with the tables' walk and with the text jump; the plain walk of packed words; the
   * cooperative kernel */
  KFMI_TRACE_KERNEL_TASK_FUSED = 5, KFMI_TRACE_KERNEL_TASK_TABLES = 6, KFMI_TRACE_KERNEL_TASK_JUMP = 7,
  KFMI_TRACE_KERNEL_TASK_WORDS = 8, KFMI_TRACE_KERNEL_COOP = 9
};
int32_t kfmi_search_strands_trace(void *index, void *queries, void *results, uint32_t strands, uint32_t *trace);
int32_t kfmi_search_seeds_trace(void *index, void *queries, void *intervals, void *spans, uint32_t max_seeds,
                                uint32_t strands, uint32_t *trace);
/* Test accessor (host only, no device, no handle): the launch plan of one search
 * from values alone -- the library's own rules (DESIGN.md "launch plan"), the
 * ones every search form asks.  A search (seeds = 0) or seed search (seeds = 1)
 * of `strands` on the backend of that name over a K = k, d index in table-size class cls (1, 2,
 * 4) with reads of m bases; ascii: the ASCII rows are on the device (0: packed by
 * the host); fused, skip, jump: the fused knob, and whether the skip table and
 * the text jump are in effect; traced: the traced twin of the call.  Returns the
 * code the call is refused with, or 0 and out[0 .. 4] = the fetch form (0 for
 * the cooperative kernel), maxw, words_maxw, the pack launch before the kernel
 * (0 none, 1 the forward pack, 2 the strand pack from ASCII, 3 from words) and
 * the kernel, KFMI_TRACE_KERNEL_*.  KFMI_E_BAD_ARGUMENT for a geometry no kernel
 * is built for. */
int32_t kfmi_launch_plan(const char *backend, uint32_t k, uint32_t d, uint32_t cls, uint32_t m, uint32_t seeds,
                         uint32_t strands, uint32_t ascii, uint32_t fused, uint32_t skip, uint32_t jump,
                         uint32_t traced, int32_t *out);

/* Diagnostic (not in the reference): replays the line requests a
 * task-mid / coop-mid search of `queries` makes (MID128 layout, K = 2, d = 64,
 * m % K == 0, both uploaded) without the LF chain's dependence: a trace launch
 * records every (K-step, read) end's line, then `reps` timed replay launches
 * issue the task kernel's loads for them with `unroll` (1, 2, 4, 8) K-steps in
 * flight per lane, as `groups` (1, 2) exec-masked lane groups (unroll 0: the
 * task kernel's own asm fetch, one K-step in flight).  *ms: mean replay launch time; *lines: lines fetched per
 * launch (= kfmi_count_blocks); *trace_bytes: the trace streamed beside them. */
int32_t kfmi_probe_replay(void *index, void *queries, int32_t unroll, int32_t groups, int32_t reps, double *ms,
                          uint64_t *lines, uint64_t *trace_bytes);

/* Bytes of the device-resident index for the current backend (incl. SA samples). */
uint64_t kfmi_device_index_bytes(void *index);

/* ---- locate: SA interval -> text positions --------------
 * Not in the reference, which stops at [L, R) (fmIndexCPUBaseline.c:288-290).
 * The index keeps a row-sampled suffix array, SA[r] for rows r % rate == 0
 * (rate a power of two <= 65536; 1 = the full SA, 4 B per row), and every other
 * row is walked back with LF_K to a sampled or '$' row on the device. */

/* kfmi_build_index_cpu/_gpu plus SA samples (sa_rate 0: none); `on_device`
 * selects the GPU builder. */
int32_t kfmi_build_index_ex(const char *text, uint64_t n, uint32_t k, uint32_t d, uint32_t sa_rate,
                            int32_t on_device, void **index);
/* The index's samples (count 0 / rate 0 when it has none); owned by the index. */
int32_t kfmi_index_sa(void *index, const uint32_t **sa, uint64_t *count, uint32_t *rate);
/* Sample file: u32 "KSA1", rate, bwtsize, 0; u64 count; u32 samples[count].
 * kfmi_load_sa attaches a file's samples to an index of the same text. */
int32_t kfmi_save_sa(const char *fn, void *index);
int32_t kfmi_load_sa(const char *fn, void *index);
/* Text positions of the rows of every query's [L, R) -- at most max_occ per
 * query (the first rows; 0 = all) -- from results still on the device (after
 * searchIndexGPU / kfmi_search) and an index with samples on the device.
 * Query q's positions are positions[offsets[q] .. offsets[q+1]), in row order
 * (positions[offsets[q] + j] = SA[L_q + j]).  Rows from n+1 on hold no
 * suffix and are not reported (an AltCounters interval can end past n+1).
 * Before the first walk on a device copy, the walk check (kfmi_set_walk_check:
 * one LF_K per row, then the sampled check or pointer jumping; 0.16 s at 3
 * Gbase) verifies that every LF_K walk ends at a '$' row; an index that fails
 * it ('ref'-mode indexes of texts with bytes other than A/C/G/T, whose walks
 * can cycle and would never end) returns KFMI_E_BUILDING_FMI (9) instead of
 * walking, so no slot ever runs the walk_lost cap of n/K steps.  kfmi_last_timing: total, scan, locate kernel (ms).  Errors: 34
 * before transfer/search, 33 without samples, 9 as above. */
int32_t         kfmi_locate(void *index, void *results, uint32_t max_occ, void **locations);
uint64_t        kfmi_locations_total(void *locations);
const uint64_t *kfmi_locations_offsets(void *locations);    /* num + 1 */
const uint32_t *kfmi_locations_positions(void *locations);  /* total */
int32_t         kfmi_locations_free(void **locations);

#ifdef __cplusplus
}
#endif

#endif /* KSTEP_FMI_H_ */
