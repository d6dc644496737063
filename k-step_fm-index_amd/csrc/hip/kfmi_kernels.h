/*
 * kfmi_kernels.h -- the search-side kernels and their launchers, shared by
 * kfmi_search.hip (host logic, dispatch) and the kfmi_inst_*.hip translation
 * units that instantiate dispatch_one<K, NB, LAY> for one (K, layout) each, so
 * the ~700 kernel instantiations compile in parallel.
 */
#ifndef KFMI_KERNELS_H_
#define KFMI_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "../../../include/kstep_fmi.h"
#include "kfmi_device.h"
#include "kfmi_grid.h"
#include "kfmi_strands.h"
#include "kfmi_coop.h"
#include "kfmi_locate.h"

namespace kfmi {

/* ------------------------------------------------------------------------ */
/* task-per-query kernel: one thread owns QPT queries (both ends each)       */
/* MAXW == 0: codes come from the pack kernel's words (qp);                 */
/* MAXW  > 0: the thread reads its own ASCII row once and keeps the codes   */
/*            in MAXW registers (fused packing, no pack launch, no qp).     */
/* ------------------------------------------------------------------------ */


/* Both ends' blocks of one step: block(L), and block(R) only when it differs. */
template <class G, int QPT>
__device__ __forceinline__ void fetch_ends(const IdxArgs& ix, const uint32_t (&L)[QPT], const uint32_t (&R)[QPT],
                                           const uint32_t (&c)[QPT], Blk<G> (&kl)[QPT], Blk<G> (&kr)[QPT])
{
#pragma unroll
  for (int i = 0; i < QPT; ++i) fetch_block<G>(ix, L[i] / (uint32_t) G::D, c[i], kl[i]);
#pragma unroll
  for (int i = 0; i < QPT; ++i) {
    const uint32_t br = R[i] / (uint32_t) G::D;
    if (br != kl[i].b) fetch_block<G>(ix, br, c[i], kr[i]);
    else kr[i] = kl[i];
  }
}

/* Issue-all-then-wait fetch for 32-byte, 16-byte-aligned plane blocks (K=2
 * d=64, K=1 d=128) with one u32 counter word: every load of both ends from ONE
 * asm block that sets exec per lane group and per condition (R only where its
 * block differs from L's, block b-1's planes only where line_local_prev chose
 * them), then a single vmcnt(0).  Written in C++ (fetch_ends) the compiler
 * copies block(L) into block(R) before R's loads issue -- a wait for L's
 * data -- so the two ends' lines are never in flight together.
 * A part no lane of a group needs (R where every R shares L's block, the
 * b-1 planes where no lane counts forward) is branched over.  Forms (the
 * SPLIT template value): 8 = one group, 7 = two 32-lane groups (32 pages per
 * instruction at most).  3 Gbase, 10M x 100 bp, against the C++ four-group
 * split (profiles/r03/sweep_r3n.jsonl): task (tag 101, 4.5 GB) 12.52 ->
 * 10.93 ms with 7 (four 16-lane groups: 11.28, removed in round 4; 8: 16.11
 * -- past the translation reach one group stalls); task-ac (tag 201, 3 GB) 11.47 ->
 * 9.51 (8: 9.79); task-mid 9.46 -> 9.40; 150 bp task-ac 17.01 -> 14.43,
 * task-mid 14.41 -> 14.34.  Issuing every part unconditionally, empty exec
 * or not, cost 15-19 % on task / task-ac (sweep_r3m.jsonl): an instruction
 * with no active lane still takes its issue slot.
 */
template <class G>
struct X4 {
  static constexpr bool OK = G::SMALL && G::BMW == 8 && G::BOFF % 4 == 0 && G::EW % 4 == 0;
};

#define KFMI_X4_BODY(T)                                      \
  "s_and_b64 exec, %[sv], %[gm]\n"                           \
  "global_load_dwordx4 %[l0], %[al], off\n"                  \
  "global_load_dwordx4 %[l1], %[al], off offset:16\n"        \
  "global_load_dword %[cl], %[acl], off\n"                   \
  KFMI_X4_PREV_L(T)                                          \
  "s_and_b64 exec, %[sv], %[gm]\n"                           \
  "s_and_b64 exec, exec, %[nr]\n"                            \
  KFMI_X4_SJ("r" T)                                          \
  "global_load_dwordx4 %[r0], %[ar], off\n"                  \
  "global_load_dwordx4 %[r1], %[ar], off offset:16\n"        \
  "global_load_dword %[cr], %[acr], off\n"                   \
  KFMI_X4_PREV_R(T)                                          \
  KFMI_X4_SL("r" T)
#define KFMI_X4_G1 "s_mov_b64 %[gm], -1\n" KFMI_X4_BODY("a")
#define KFMI_X4_G2 "s_bfm_b64 %[gm], 32, 0\n" KFMI_X4_BODY("a") "s_bfm_b64 %[gm], 32, 32\n" KFMI_X4_BODY("b")
#define KFMI_X4_ASM(GROUPS) "s_mov_b64 %[sv], exec\n" GROUPS "s_mov_b64 exec, %[sv]\ns_waitcnt vmcnt(0)\n"
#define KFMI_X4_OUT                                                                                          \
  [l0] "=&v"(l0), [l1] "=&v"(l1), [r0] "=&v"(r0), [r1] "=&v"(r1), [cl] "=&v"(cl), [cr] "=&v"(cr), [sv] "=&s"(sv), \
      [gm] "=&s"(gm)
#define KFMI_X4_IN [al] "v"(wl.planes), [acl] "v"(wl.cnt), [ar] "v"(wr.planes), [acr] "v"(wr.cnt), [nr] "s"(nr)
#define KFMI_X4_OUTP KFMI_X4_OUT, [p0] "=&v"(p0), [p1] "=&v"(p1), [q0] "=&v"(q0), [q1] "=&v"(q1)
#define KFMI_X4_INP KFMI_X4_IN, [pl] "s"(pl), [pr] "s"(pr), [po0] "i"(PO), [po1] "i"(PO + 16)
/* empty-exec skips: a branch over a part no lane of the group needs */
#define KFMI_X4_SJ(L) "s_cbranch_execz .Lx4" L "_%=\n"
#define KFMI_X4_SL(L) ".Lx4" L "_%=:\n"
#define KFMI_X4_PREV_L_ON(T)                                 \
  "s_and_b64 exec, exec, %[pl]\n"                            \
  KFMI_X4_SJ("p" T)                                          \
  "global_load_dwordx4 %[p0], %[al], off offset:%[po0]\n"    \
  "global_load_dwordx4 %[p1], %[al], off offset:%[po1]\n"    \
  KFMI_X4_SL("p" T)
#define KFMI_X4_PREV_R_ON(T)                                 \
  "s_and_b64 exec, exec, %[pr]\n"                            \
  KFMI_X4_SJ("r" T)                                          \
  "global_load_dwordx4 %[q0], %[ar], off offset:%[po0]\n"    \
  "global_load_dwordx4 %[q1], %[ar], off offset:%[po1]\n"

template <class G, int SPLIT>
__device__ __forceinline__ void fetch_ends_x4(const IdxArgs& ix, uint32_t L, uint32_t R, uint32_t c, Blk<G>& kl,
                                              Blk<G>& kr)
{
  static_assert(SPLIT == 7 || SPLIT == 8, "fetch form: 7, 8 = two, one lane group(s)");
  const uint32_t bl = L / (uint32_t) G::D, br = R / (uint32_t) G::D;
  Where<G> wl = locate<G>(ix, bl, c);
  Where<G> wr = locate<G>(ix, br, c);
  line_local_prev<G>(ix, bl, c, wl);
  line_local_prev<G>(ix, br, c, wr);
  const bool needR = br != bl;
  const uint64_t nr = __ballot(needR);
  v4u l0, l1, r0, r1;
  uint32_t cl, cr;
  uint64_t sv, gm;
  if constexpr (G::NEIGHBOR) {
    const uint64_t pl = __ballot(wl.prev), pr = __ballot(wr.prev);
    constexpr int PO = -4 * G::EW;   /* block b-1's planes, relative to block b's */
    v4u p0, p1, q0, q1;
#define KFMI_X4_PREV_L(T) KFMI_X4_PREV_L_ON(T)
#define KFMI_X4_PREV_R(T) KFMI_X4_PREV_R_ON(T)
    if constexpr (SPLIT == 8)
      asm volatile(KFMI_X4_ASM(KFMI_X4_G1) : KFMI_X4_OUTP : KFMI_X4_INP : "memory", "scc");
    else
      asm volatile(KFMI_X4_ASM(KFMI_X4_G2) : KFMI_X4_OUTP : KFMI_X4_INP : "memory", "scc");
#undef KFMI_X4_PREV_L
#undef KFMI_X4_PREV_R
    const v4u pa = needR ? q0 : p0, pb = needR ? q1 : p1;
    kl.bp[0] = p0.x; kl.bp[1] = p0.y; kl.bp[2] = p0.z; kl.bp[3] = p0.w;
    kl.bp[4] = p1.x; kl.bp[5] = p1.y; kl.bp[6] = p1.z; kl.bp[7] = p1.w;
    kr.bp[0] = pa.x; kr.bp[1] = pa.y; kr.bp[2] = pa.z; kr.bp[3] = pa.w;
    kr.bp[4] = pb.x; kr.bp[5] = pb.y; kr.bp[6] = pb.z; kr.bp[7] = pb.w;
  } else {
#define KFMI_X4_PREV_L(T)
#define KFMI_X4_PREV_R(T)
    if constexpr (SPLIT == 8)
      asm volatile(KFMI_X4_ASM(KFMI_X4_G1) : KFMI_X4_OUT : KFMI_X4_IN : "memory", "scc");
    else
      asm volatile(KFMI_X4_ASM(KFMI_X4_G2) : KFMI_X4_OUT : KFMI_X4_IN : "memory", "scc");
#undef KFMI_X4_PREV_L
#undef KFMI_X4_PREV_R
  }
  const v4u ra = needR ? r0 : l0, rb = needR ? r1 : l1;
  kl.bm[0] = l0.x; kl.bm[1] = l0.y; kl.bm[2] = l0.z; kl.bm[3] = l0.w;
  kl.bm[4] = l1.x; kl.bm[5] = l1.y; kl.bm[6] = l1.z; kl.bm[7] = l1.w;
  kr.bm[0] = ra.x; kr.bm[1] = ra.y; kr.bm[2] = ra.z; kr.bm[3] = ra.w;
  kr.bm[4] = rb.x; kr.bm[5] = rb.y; kr.bm[6] = rb.z; kr.bm[7] = rb.w;
  kl.cnt = cl;
  kr.cnt = needR ? cr : cl;
  kl.b = bl;
  kr.b = br;
  kl.e = wl.e;
  kr.e = wr.e;
  kl.prev = wl.prev;
  kr.prev = wr.prev;
}
#undef KFMI_X4_BODY
#undef KFMI_X4_G1
#undef KFMI_X4_G2
#undef KFMI_X4_ASM
#undef KFMI_X4_OUT
#undef KFMI_X4_IN
#undef KFMI_X4_OUTP
#undef KFMI_X4_INP
#undef KFMI_X4_SJ
#undef KFMI_X4_SL
#undef KFMI_X4_PREV_L_ON
#undef KFMI_X4_PREV_R_ON

/* The fetch forms (the SPLIT template value, launch_task): 1 = the C++ fetch
 * in one group; 4 = the same loads as four exec-masked 16-lane groups, so one
 * wave instruction touches at most 16 pages (IdxArgs::split); 7 / 8 = the asm
 * fetch in two / one group(s) (X4 geometries only). */
template <class G, int QPT, int SPLIT>
__device__ __forceinline__ void fetch_ends_split(const IdxArgs& ix, const uint32_t (&L)[QPT],
                                                 const uint32_t (&R)[QPT], const uint32_t (&c)[QPT],
                                                 Blk<G> (&kl)[QPT], Blk<G> (&kr)[QPT])
{
  static_assert(SPLIT == 1 || SPLIT == 4 || ((SPLIT == 7 || SPLIT == 8) && QPT == 1 && X4<G>::OK),
                "fetch form: 1 / 4 (C++ fetch), 7 / 8 (asm fetch, X4 geometries)");
  if constexpr (SPLIT >= 7) {
    fetch_ends_x4<G, SPLIT>(ix, L[0], R[0], c[0], kl[0], kr[0]);
  } else if constexpr (SPLIT == 1) {
    fetch_ends<G, QPT>(ix, L, R, c, kl, kr);
  } else {
    const int grp = (int) (threadIdx.x & 63) / 16;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (grp == g) fetch_ends<G, QPT>(ix, L, R, c, kl, kr);
  }
}

/* The trace policy of skip_walk and task_kernel (TR, below): whether the walk
 * records what it does, and the type of the pointer it records through -- the
 * records of a launch (Trace) or an empty object (NoTrace, every search). */
struct NoTrace {
  static constexpr bool ON = false, STRANDS = false;
  struct Out {};
  static Out from(uint4*) { return Out{}; }
  __device__ static Out at(Out, uint64_t) { return Out{}; }
};
struct Trace {
  static constexpr bool ON = true, STRANDS = false;
  typedef uint4* Out;
  static Out from(uint4* t) { return t; }
  __device__ static Out at(Out t, uint64_t q) { return t + q; }   /* read q's record */
};
/* Trace for the strand kernels (kfmi_search_strands_trace): launch_task_split
 * picks task_strands_kernel / task_words_skip_kernel with it and nothing else,
 * so the forward traced units (Trace) stay what they were. */
struct StrandTrace : Trace {
  static constexpr bool STRANDS = true;
};

/* Word 3 of the seed and strand trace records (kstep_fmi.h): which kernel ran,
 * in which fetch form and with how many code registers, and the table
 * settings it received.  KID: KFMI_TRACE_KERNEL_*. */
template <int SPLIT, int MAXW, int KID>
__device__ __forceinline__ uint32_t trace_launch_id(const IdxArgs& ix)
{
  const bool ft = ix.ftab != nullptr;
  return (uint32_t) SPLIT | ((uint32_t) (MAXW / 8) << KFMI_TRACE_ID_MAXW_SHIFT) | ((uint32_t) KID << KFMI_TRACE_ID_KERNEL_SHIFT) |
         ((ix.skip_split & 15u) << KFMI_TRACE_ID_SKIP_SPLIT_SHIFT) |
         (ft && (ix.jump_split & JUMP_FTAB_FOLDED) ? (uint32_t) KFMI_TRACE_ID_FTAB_FOLDED : 0u) |
         (ft ? ix.ftab_steps << KFMI_TRACE_ID_FTAB_STEPS_SHIFT : 0u);
}

/* The walk of the fused task kernel with the skip table (IdxArgs::skip,
 * DESIGN.md 5a'): every lane keeps its own step position `pos`, and each
 * round of the wave-uniform loop a lane takes either one table lookup or one
 * ordinary K-step -- one line either way, issued before anything waits, so a
 * round is one memory round trip for the whole wave.
 *   A lane looks up skip[L] when its interval is the one row [L, L+1), L is a
 * table row and J = skip_steps more steps remain.  The entry holds the code
 * stream of the only J steps that keep that row's interval non-empty and the
 * row they end in; when it equals the read's next 32 code bits the lane is at
 * [row, row+1) J steps later, exactly as the walk would be (the entry is the
 * composition of the search's own J steps, skip_level0_kernel).  Otherwise
 * the lane walks on from the state it had and never looks up again: the walk
 * empties the interval within those J steps, and a lookup from any row on the
 * way compares a window that still holds the differing step.
 *   The code words live in LDS after the staging (64 lanes x MAXW words per
 * wave, word-major so a wave's reads of one word index hit 64 banks): `pos`
 * differs per lane, and a register array indexed by it would go to scratch.
 * Lanes only read what they wrote themselves, so no barrier follows.
 *   JUMP (DESIGN.md 5a'', IdxArgs::jsa): a lane on one row [L, L+1) with at
 * least jump_min bases left ends its walk with three lookups.  p = jsa[L] is
 * the one text position that carries the matched suffix, and each of the t
 * steps left either empties the interval or moves to the row of suffix p - K;
 * so the walk ends on [jisa[p - tK], + 1) iff p >= tK and the tK text bases
 * before p are the read's remaining code stream, and empties otherwise.  The
 * round that would look up the skip table loads jsa[L] instead; a second
 * round trip, taken only when a lane of the wave jumps, loads the text window
 * (dwords of jtext, issued together, each lane only its own words) and
 * jisa[p - tK] -- its address clamped to 0 before the load when p < tK.  A
 * window of at most JUMP_LINE_W bases and its ISA entry come from one 128-byte
 * line of the line table instead (DESIGN.md 5a''', IdxArgs::jsa): a per-lane
 * choice of addresses for the same loads, the same wait and the same compare.
 * A lane whose compare fails keeps the state it had, never jumps again and goes
 * on through the skip lookups and K-steps, so it returns the very empty
 * interval the walk returns.  A lane whose jump-start entry carried sa[L] (p0,
 * a folded table: DESIGN.md 5a'''') takes that value in its first round and
 * issues no jsa[L] load; everything after is the same.
 *   TR (kstep_fmi.h kfmi_search_trace): with Trace the same
 * body counts what the lane does -- K-steps, skip lookups that matched and that
 * did not, its one text jump -- and stores one 16-byte record when it leaves
 * the loop.  Every hook is an `if constexpr (TR::ON)` block; with NoTrace, the
 * default, none of them is instantiated and `tr` is an empty object. */
template <class G, int MAXW, int SPLIT, bool JUMP = false, class TR = NoTrace>
__device__ __forceinline__ void skip_walk(const IdxArgs& ix, const uint32_t (&cw)[MAXW], uint32_t steps, uint32_t pos,
                                          uint32_t& Lq, uint32_t& Rq, typename TR::Out tr = typename TR::Out{},
                                          uint32_t p0 = SKIP_NONE)
{
  static_assert(G::K <= 2 && MAXW > 0, "skip table: fused task kernels at K <= 2");
  /* TR: the record's words 0 .. 2 (kstep_fmi.h); the start is `pos` as the caller passed it */
  [[maybe_unused]] uint32_t tr_walk = 0, tr_jump = 0, tr_line = 0, tr_fold = 0;
  [[maybe_unused]] const uint32_t tr_start = pos;
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t* cl = reinterpret_cast<uint32_t*>(stage) + wv * (64u * MAXW) + lane;
#pragma unroll
  for (int k = 0; k < MAXW; ++k) cl[64 * k] = cw[k];
  const uint32_t J = ix.skip_steps;
  const int grp = (int) lane / 16;
  uint32_t L[1] = {Lq}, R[1] = {Rq};
  bool dead = false;   /* a lookup differed: the ordinary steps from here on */
  /* JUMP: `dead` (bit 0) and "a text jump failed: the skip lookups and steps
   * from here on" (bit 1) in one VGPR; as two more lane masks they take the
   * 8-word kernel past 96 SGPRs, a wave per SIMD */
  uint32_t fl = 0;
  auto is_dead = [&]() -> bool {
    if constexpr (JUMP) return (fl & 1u) != 0u;
    else return dead;
  };
  while (__ballot(pos < steps)) {
    const bool act = pos < steps;
    const uint32_t bit = pos * (2u * G::K), k = bit >> 5;
    const uint32_t lo = k < (uint32_t) MAXW ? cl[64u * k] : 0u;
    const uint32_t hi = k + 1u < (uint32_t) MAXW ? cl[64u * (k + 1u)] : 0u;
    const uint32_t code = __builtin_amdgcn_alignbit(hi, lo, bit & 31u);   /* the stream from step `pos` on */
    const bool row1 = act && R[0] == L[0] + 1u;
    bool jmp = false;
    uint32_t p = SKIP_NONE;
    if constexpr (JUMP) {
      jmp = row1 && !(fl & 2u) && L[0] < ix.bwtsize && (steps - pos) * (uint32_t) G::K >= ix.jump_min;
      /* p0: sa[L] from the lane's jump-start entry (a folded table, DESIGN.md
       * 5a''''), for its first round only -- then no jsa[L] load goes out */
      const bool ld = jmp && p0 == SKIP_NONE;
      if (ix.jump_split & JUMP_SPLIT4) {   /* wave-uniform */
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (ld && grp == g) p = ix.jsa[L[0]];
      } else if (ld) {
        p = ix.jsa[L[0]];
      }
      if (jmp && !ld) {
        p = p0;
        if constexpr (TR::ON) tr_fold = KFMI_TRACE_START_FOLDED;
      }
      p0 = SKIP_NONE;
    }
    const bool one = row1 && !jmp && !is_dead() && L[0] < ix.skip_rows && pos + J <= steps;
    uint2 e = make_uint2(SKIP_NONE, 0u);
    if (ix.skip_split == 4u) {   /* wave-uniform: at most 16 pages per gather instruction */
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (one && grp == g) e = ix.skip[L[0]];
    } else if (one) {
      e = ix.skip[L[0]];
    }
    if (act && !one && !jmp) {
      uint32_t c[1] = {code & (uint32_t) (G::NC - 1)};
      uint32_t sx[2 * G::K];
      plane_xor<G::K>(c[0], sx);
      if constexpr (G::SMALL) {
        Blk<G> kl[1], kr[1];
        fetch_ends_split<G, 1, SPLIT>(ix, L, R, c, kl, kr);
        L[0] = lf_from_block<G>(ix, kl[0], L[0], c[0], sx);
        R[0] = lf_from_block<G>(ix, kr[0], R[0], c[0], sx);
      } else {
        L[0] = lf_stream<G>(ix, L[0], c[0], sx);
        R[0] = lf_stream<G>(ix, R[0], c[0], sx);
      }
      ++pos;
      if constexpr (TR::ON) tr_walk += KFMI_TRACE_STEP;
    }
    if (one) {
      if (e.x != SKIP_NONE && e.y == code) {
        L[0] = e.x;
        R[0] = e.x + 1u;
        pos += J;
        if constexpr (TR::ON) tr_walk += KFMI_TRACE_SKIP_HIT;
      } else {
        if constexpr (JUMP) fl |= 1u;
        else dead = true;
        if constexpr (TR::ON) tr_walk += KFMI_TRACE_SKIP_MISS;
      }
    }
    if constexpr (JUMP) {
      if (__ballot(jmp)) {   /* wave-uniform: the text window and the ISA entry, one more round trip */
        const uint32_t nb = (steps - pos) * (uint32_t) G::K;          /* bases left: the window */
        const bool ok = jmp && p < ix.bwtsize && p >= nb;             /* SKIP_NONE fails the first test */
        const uint32_t q = ok ? p - nb : 0u;                          /* in range before the load is issued */
        const uint32_t off = ok ? ix.bwtsize - 1u - p : 0u;                /* the stream at p starts at bit 2 * off */
        uint32_t tsh = (off & 15u) * 2u;
        const uint32_t nw = ok ? (nb + 15u) >> 4 : 0u;                /* words compared, <= MAXW */
        /* per lane: where its window and its ISA entry lie, and how many words
         * of the window go out.  The flat tables take nw + 1 words of jtext and
         * jisa[q]; a lane with nb <= JUMP_LINE_W takes both from its one line
         * (DESIGN.md 5a'''), and there only the words the compare needs, so no
         * load leaves the line.  One set of loads for both kinds of lane. */
        const uint32_t* tp = ix.jsa + (2ull * ix.bwtsize + (off >> 4));
        const uint32_t* ip = ix.jsa + ((uint64_t) ix.bwtsize + q);
        uint32_t lim = ok ? nw + 1u : 0u;
        if (ok && (ix.jump_split & JUMP_LINES) && nb <= JUMP_LINE_W) {
          const JumpLineAt at = jump_line_at(ix.bwtsize - 1u, p, nb);
          const uint32_t* lb = ix.jsa + jump_lines_off(ix.bwtsize);
          tp = lb + at.text_dw;
          ip = lb + at.isa_dw;
          tsh = at.shift;
          lim = at.ndw;
          if constexpr (TR::ON) tr_line = KFMI_TRACE_JUMP_LINE;
        }
        uint32_t tx[MAXW + 1];
#pragma unroll
        for (int j = 0; j <= MAXW; ++j) tx[j] = 0u;
        uint32_t r = SKIP_NONE;
        if (ix.jump_split & JUMP_LINES_GROUPED) {   /* wave-uniform: all of a lane's loads under its group's mask */
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (ok && grp == g) {
#pragma unroll
              for (int j = 0; j <= MAXW; ++j)
                if ((uint32_t) j < lim) tx[j] = tp[j];
              r = *ip;
            }
        } else {
#pragma unroll
          for (int j = 0; j <= MAXW; ++j)
            if ((uint32_t) j < lim) tx[j] = tp[j];
          if (ix.jump_split & JUMP_SPLIT4) {   /* wave-uniform */
#pragma unroll
            for (int g = 0; g < 4; ++g)
              if (ok && grp == g) r = *ip;
          } else if (ok) {
            r = *ip;
          }
        }
        uint32_t diff = 0u;
#pragma unroll
        for (int j = 0; j < MAXW; ++j) {
          if ((uint32_t) j < nw) {
            const uint32_t kj = k + (uint32_t) j;
            const uint32_t rl = kj < (uint32_t) MAXW ? cl[64u * kj] : 0u;
            const uint32_t rh = kj + 1u < (uint32_t) MAXW ? cl[64u * (kj + 1u)] : 0u;
            const uint32_t rw = __builtin_amdgcn_alignbit(rh, rl, bit & 31u);
            const uint32_t tv = __builtin_amdgcn_alignbit(tx[j + 1], tx[j], tsh);
            const uint32_t left = 2u * nb - 32u * (uint32_t) j;   /* bits of the window from this word on */
            diff |= (rw ^ tv) & (left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u);
          }
        }
        if constexpr (TR::ON) {   /* before pos moves: where the lane stood, and how the jump ended */
          if (jmp) {
            const uint32_t out = !ok ? KFMI_TRACE_JUMP_REFUSED
                                     : (diff != 0u ? KFMI_TRACE_JUMP_DIFFERED
                                                   : (r < ix.bwtsize ? KFMI_TRACE_JUMP_TAKEN : KFMI_TRACE_JUMP_BAD_ISA));
            tr_jump = KFMI_TRACE_JUMP_TRIED | tr_line | (out << KFMI_TRACE_JUMP_OUT_SHIFT) |
                      (pos << KFMI_TRACE_JUMP_POS_SHIFT) | (nb << KFMI_TRACE_JUMP_NB_SHIFT);
          }
        }
        if (ok && diff == 0u && r < ix.bwtsize) {
          L[0] = r;
          R[0] = r + 1u;
          pos = steps;
        } else if (jmp) {
          fl |= 2u;
        }
      }
    }
  }
  Lq = L[0];
  Rq = R[0];
  if constexpr (TR::ON) *tr = make_uint4(tr_walk, tr_jump, tr_start | tr_fold, ix.jump_split & ~JUMP_FTAB_FOLDED);
}

/* The walk of a seed search (kfmi_seeds.hip, kstep_fmi.h section 2, DESIGN.md
 * 5g): the greedy right-to-left factorisation of one task into maximal exact
 * segments, on skip_walk's frame -- the same code words in LDS, the same
 * per-lane `pos`, one line per lane and round.  A task of m bases has the
 * units, from the right, of its last rem = m % K bases and then of K bases
 * each; `mk` = m - rem, and after `pos` K-steps the walk stands at base
 * b = mk - K * pos.  Beside [L, R) a lane keeps the end `e` of its segment
 * (e == b: nothing matched yet, [L, R) is the full interval), the interval it
 * had before the round's step, and its record count.
 *   When a step leaves R <= L the segment P[b .. e) is maximal: the lane stores
 * {previous L, R} into iv[cnt] and {b, e - b} into sp[cnt] -- as the record
 * completes, at a runtime address, so no register array is indexed by cnt --
 * and starts again from [0, bwtsize) at the same pos.  When the step started
 * from the full interval the unit alone does not occur: nothing is stored and
 * the lane moves on by one unit.  A new segment may take the tables again: a
 * lane on the full interval looks up the jump-start table with the window
 * `code` (its low 2K * ftab_steps bits are the table's index), a lane on one
 * row the skip table; both tables are uint2, so a round's lookup is one load
 * either way.  An empty jump-start entry only says that the segment ends
 * within those steps, not where, and a differing skip entry the same: the lane
 * takes the ordinary steps until its segment ends (`dead`).
 *   The loop ends when no lane has steps or free slots left; the segment that
 * reaches base 0 is stored then, and the slots a task did not use are zeroed.
 * Start: pos = 0 and [L, R), e from the caller -- the remainder-table entry
 * with e = m where it is not empty, else the full interval with e = mk.
 *   TR (kstep_fmi.h kfmi_search_seeds_trace): with Trace the same body counts
 * the lane's K-steps, its lookups in either table by how they ended, the units
 * that did not occur on their own and its records, and stores one 16-byte record
 * with the caller's `ident` as word 3 when the walk is over.  Every hook is an
 * `if constexpr (TR::ON)` block, as in skip_walk. */
template <class G, int MAXW, int SPLIT, class TR = NoTrace>
__device__ __forceinline__ void seed_walk(const IdxArgs& ix, const uint32_t (&cw)[MAXW], uint32_t steps, uint32_t mk,
                                          uint32_t Lq, uint32_t Rq, uint32_t e, uint32_t S, uint2* __restrict__ iv,
                                          uint2* __restrict__ sp, typename TR::Out tr = typename TR::Out{},
                                          [[maybe_unused]] uint32_t ident = 0u)
{
  static_assert(G::K <= 2 && MAXW > 0, "seed search: task kernels at K <= 2");
  /* TR: the record's words 0 .. 2; a remainder unit that does not occur (the caller's e == mk) is a lone unit */
  [[maybe_unused]] uint32_t tr_walk = 0, tr_start = 0, tr_lone = ix.rem && e == mk ? 1u : 0u;
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t* cl = reinterpret_cast<uint32_t*>(stage) + wv * (64u * MAXW) + lane;
#pragma unroll
  for (int k = 0; k < MAXW; ++k) cl[64 * k] = cw[k];
  const uint32_t J = ix.skip_steps, F = ix.ftab ? ix.ftab_steps : 0u;
  const int grp = (int) lane / 16;
  uint32_t L[1] = {Lq}, R[1] = {Rq};
  uint32_t pos = 0, cnt = 0;
  bool dead = false;   /* a lookup failed: the ordinary steps until this segment ends */
  while (__ballot(pos < steps && cnt < S)) {
    const bool act = pos < steps && cnt < S;
    const uint32_t bit = pos * (2u * G::K), k = bit >> 5;
    const uint32_t lo = k < (uint32_t) MAXW ? cl[64u * k] : 0u;
    const uint32_t hi = k + 1u < (uint32_t) MAXW ? cl[64u * (k + 1u)] : 0u;
    const uint32_t code = __builtin_amdgcn_alignbit(hi, lo, bit & 31u);   /* the stream from step `pos` on */
    const uint32_t b = mk - (uint32_t) G::K * pos;
    const bool fresh = e == b;
    const bool jump = act && !dead && fresh && F != 0u && pos + F <= steps;
    const bool one = act && !dead && !fresh && R[0] == L[0] + 1u && L[0] < ix.skip_rows && pos + J <= steps;
    const bool look = one || jump;
    const uint2* tp = one ? ix.skip + L[0] : ix.ftab + (jump ? code & ix.ftab_mask : 0u);
    uint2 te = make_uint2(SKIP_NONE, 0u);
    if (ix.skip_split == 4u) {   /* wave-uniform: at most 16 pages per gather instruction */
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (look && grp == g) te = *tp;
    } else if (look) {
      te = *tp;
    }
    if (act && !look) {
      const uint32_t pL = L[0], pR = R[0];
      uint32_t c[1] = {code & (uint32_t) (G::NC - 1)};
      uint32_t sx[2 * G::K];
      plane_xor<G::K>(c[0], sx);
      if constexpr (G::SMALL) {
        Blk<G> kl[1], kr[1];
        fetch_ends_split<G, 1, SPLIT>(ix, L, R, c, kl, kr);
        L[0] = lf_from_block<G>(ix, kl[0], L[0], c[0], sx);
        R[0] = lf_from_block<G>(ix, kr[0], R[0], c[0], sx);
      } else {
        L[0] = lf_stream<G>(ix, L[0], c[0], sx);
        R[0] = lf_stream<G>(ix, R[0], c[0], sx);
      }
      if constexpr (TR::ON) tr_walk += KFMI_TRACE_STEP;
      if (R[0] <= L[0]) {   /* the segment ends at b */
        if (fresh) {        /* this unit alone does not occur: past it, no record */
          ++pos;
          e = b - (uint32_t) G::K;
          if constexpr (TR::ON) ++tr_lone;
        } else {
          iv[cnt] = make_uint2(pL, pR);
          sp[cnt] = make_uint2(b, e - b);
          ++cnt;
          e = b;
        }
        L[0] = 0u;
        R[0] = ix.bwtsize;
        dead = false;
      } else {
        ++pos;
      }
    }
    if (one) {
      if (te.x != SKIP_NONE && te.y == code) {
        L[0] = te.x;
        R[0] = te.x + 1u;
        pos += J;
        if constexpr (TR::ON) tr_walk += KFMI_TRACE_SKIP_HIT;
      } else {
        dead = true;
        if constexpr (TR::ON) tr_walk += KFMI_TRACE_SKIP_MISS;
      }
    } else if (jump) {
      const FtabAt fe = ftab_entry_at(te, (ix.jump_split & JUMP_FTAB_FOLDED) != 0u, ix.bwtsize - 1u);
      if (fe.R > fe.L) {
        L[0] = fe.L;
        R[0] = fe.R;
        pos += F;
        if constexpr (TR::ON) tr_start += KFMI_SEED_TRACE_START_HIT;
      } else {
        dead = true;
        if constexpr (TR::ON) tr_start += KFMI_SEED_TRACE_START_EMPTY;
      }
    }
  }
  const uint32_t b = mk - (uint32_t) G::K * pos;   /* 0 unless the slots ran out */
  if (cnt < S && e != b) {
    iv[cnt] = make_uint2(L[0], R[0]);
    sp[cnt] = make_uint2(b, e - b);
    ++cnt;
  }
  if constexpr (TR::ON) *tr = make_uint4(tr_walk, tr_start, tr_lone | (cnt << KFMI_SEED_TRACE_RECORDS_SHIFT), ident);
  for (; cnt < S; ++cnt) {
    iv[cnt] = make_uint2(0u, 0u);
    sp[cnt] = make_uint2(0u, 0u);
  }
}

/* SKIP (last template value, fused K <= 2 only): the walk with the skip table,
 * launched when ix.skip or ix.jsa is set; without it the kernel is the plain
 * walk.  JUMP (with SKIP, plain layouts): skip_walk with the text jump, launched
 * when ix.jsa is set; the strand and words kernels are compiled without it.
 * TR = Trace (with SKIP): skip_walk writes read q's record to trace[q]; with
 * NoTrace `trace` is an empty object and the kernel is what it was. */
template <class G, int QPT, int MAXW, int SPLIT = 1, bool SKIP = false, bool JUMP = false, class TR = NoTrace>
__global__ __launch_bounds__(256) void task_kernel(IdxArgs ix, const uint32_t* __restrict__ qp,
                                                   const uint8_t* __restrict__ ascii, uint32_t m, uint64_t num,
                                                   uint32_t steps, uint32_t nwords, uint32_t* __restrict__ res,
                                                   typename TR::Out trace)
{
  static_assert(!TR::ON || SKIP, "walk trace: skip_walk's hooks");
  constexpr int SPW = G::SPW;
  constexpr int CW = MAXW > 0 ? (G::K == 3 ? k3_words<(MAXW > 0 ? MAXW : 1)>() : MAXW) : 1;
  static_assert(MAXW == 0 || QPT == 1, "fused packing: one query per thread");
  static_assert(!SKIP || (MAXW > 0 && G::K <= 2), "skip table: fused task kernels at K <= 2");
  static_assert(!JUMP || (SKIP && (G::LAY == LAY_INTER || G::LAY == LAY_MID)), "text jump: skip_walk, plain layouts");
  const uint64_t base = (uint64_t) blockIdx.x * (256 * QPT) + threadIdx.x;
  uint32_t cw[QPT][CW];
  uint32_t rc = 0;
  if constexpr (MAXW > 0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    if constexpr (G::K == 3) {   /* 16 bases per word -> 5 K-steps per word */
      uint32_t raw[MAXW];
      stage_query_codes<MAXW>(ascii, num, m, stage, raw, ix.rem, rc);   /* whole block, before any exit */
      recut30<MAXW>(raw, cw[0]);
    } else {
      stage_query_codes<MAXW>(ascii, num, m, stage, cw[0], ix.rem, rc);   /* whole block, before any exit */
    }
  }
  if (base >= num) return;
  uint64_t q[QPT];
  uint32_t L[QPT], R[QPT];
#pragma unroll
  for (int i = 0; i < QPT; ++i) {
    q[i] = base + (uint64_t) i * 256;
    if (q[i] >= num) q[i] = base;   /* duplicate work for the tail, never stored twice */
    L[i] = 0;
    R[i] = ix.bwtsize;
  }
  uint32_t skip = 0;
  [[maybe_unused]] uint32_t p0 = SKIP_NONE;
  if (ix.ftab && steps >= ix.ftab_steps) {   /* wave-uniform: jump start from the ftab */
    skip = ix.ftab_steps;
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
      uint32_t w0;
      if constexpr (MAXW > 0) w0 = cw[i][0];
      else w0 = qp[q[i]];
      const FtabAt lr = ftab_lookup(ix, w0);
      L[i] = lr.L;
      R[i] = lr.R;
      if constexpr (JUMP) p0 = lr.p;   /* sa[L] of a one-row entry of a folded table */
    }
  }
  if (ix.rem) {   /* wave-uniform: m % K != 0, the last rem bases from the remainder table */
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
      const uint2 lr = ix.rtab[MAXW > 0 ? rc : qp[(uint64_t) nwords * num + q[i]]];
      L[i] = lr.x;
      R[i] = lr.y;
    }
    p0 = SKIP_NONE;   /* no jump start beside the remainder table (use_rtab) */
  }
  if constexpr (SKIP) {
    skip_walk<G, MAXW, SPLIT, JUMP, TR>(ix, cw[0], steps, skip, L[0], R[0], TR::at(trace, base), p0);
    *reinterpret_cast<uint2*>(res + 2 * base) = make_uint2(L[0], R[0]);
    return;
  }
  for (uint32_t w = 0; w < nwords; ++w) {
    uint32_t word[QPT];
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
      if constexpr (MAXW > 0) {
        word[i] = cw[i][0];
#pragma unroll
        for (int k = 0; k + 1 < CW; ++k) cw[i][k] = cw[i][k + 1];
      } else {
        word[i] = qp[(uint64_t) w * num + q[i]];
      }
    }
    const uint32_t left = steps - w * SPW;
#pragma unroll
    for (int j = 0; j < SPW; ++j) {
      if ((uint32_t) j >= left) continue;   /* only the last word is partial (wave-uniform) */
      if (w * SPW + j < skip) continue;      /* steps covered by the ftab (wave-uniform) */
      uint32_t c[QPT];
#pragma unroll
      for (int i = 0; i < QPT; ++i) c[i] = (word[i] >> (2 * G::K * j)) & (uint32_t) (G::NC - 1);
      if constexpr (G::SMALL) {
        Blk<G> kl[QPT], kr[QPT];
        fetch_ends_split<G, QPT, SPLIT>(ix, L, R, c, kl, kr);
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
          uint32_t sx[2 * G::K];
          plane_xor<G::K>(c[i], sx);
          L[i] = lf_from_block<G>(ix, kl[i], L[i], c[i], sx);
          R[i] = lf_from_block<G>(ix, kr[i], R[i], c[i], sx);
        }
      } else {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
          uint32_t sx[2 * G::K];
          plane_xor<G::K>(c[i], sx);
          L[i] = lf_stream<G>(ix, L[i], c[i], sx);
          R[i] = lf_stream<G>(ix, R[i], c[i], sx);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < QPT; ++i) {
    const uint64_t qi = base + (uint64_t) i * 256;
    if (qi < num) *reinterpret_cast<uint2*>(res + 2 * qi) = make_uint2(L[i], R[i]);
  }
}

/* Strand searches (kfmi_strands.hip): the walk with the skip
 * table on code words a pack launch wrote -- the ns * num task columns of qp,
 * word-major, 16 bases per word (K <= 2), at most MAXW words per task.  A lane
 * loads its column (a word row is consecutive tasks: coalesced) where the fused
 * kernel converts its ASCII row; the jump start, the remainder lookup and
 * skip_walk are the fused kernel's.  The forward kernels are not touched.
 * TR = StrandTrace (kfmi_search_strands_trace): skip_walk writes task q's record
 * to trace[q] and the kernel replaces its word 3 by the launch identity. */
template <class G, int MAXW, int SPLIT, class TR = NoTrace>
__global__ __launch_bounds__(256) void task_words_skip_kernel(IdxArgs ix, const uint32_t* __restrict__ qp, uint64_t num,
                                                              uint32_t steps, uint32_t nwords,
                                                              uint32_t* __restrict__ res, typename TR::Out trace)
{
  static_assert(G::K <= 2 && MAXW > 0, "skip table: task kernels at K <= 2");
  const uint64_t q = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (q >= num) return;
  uint32_t cw[MAXW];
#pragma unroll
  for (int k = 0; k < MAXW; ++k) cw[k] = (uint32_t) k < nwords ? qp[(uint64_t) k * num + q] : 0u;
  uint32_t L = 0, R = ix.bwtsize, skip = 0;
  if (ix.ftab && steps >= ix.ftab_steps) {   /* wave-uniform: jump start from the ftab */
    skip = ix.ftab_steps;
    const FtabAt lr = ftab_lookup(ix, cw[0]);
    L = lr.L;
    R = lr.R;
  }
  if (ix.rem) {   /* wave-uniform: m % K != 0, the last rem bases from the remainder table */
    const uint2 lr = ix.rtab[qp[(uint64_t) nwords * num + q]];
    L = lr.x;
    R = lr.y;
  }
  skip_walk<G, MAXW, SPLIT, false, TR>(ix, cw, steps, skip, L, R, TR::at(trace, q));
  if constexpr (TR::ON) TR::at(trace, q)->w = trace_launch_id<SPLIT, MAXW, KFMI_TRACE_KERNEL_TASK_WORDS_SKIP>(ix);
  *reinterpret_cast<uint2*>(res + 2 * q) = make_uint2(L, R);
}

/* Strand-aware fused packing for a 256-thread block, one task
 * per thread, m % K == 0: stage_query_codes for the ns * num tasks of
 * `strands` (2 = the reverse strand, 3 = both: task 2q + strand).  In BOTH a
 * wave's 64 lanes are 32 reads, so it stages half the rows per task, and lanes
 * 2i and 2i + 1 convert the same LDS row; a wave's first read, 32 * (waves
 * before it), keeps r0 * m % 16 == 0 for every m.  Every lane packs its row
 * forward (row_codes), derives the reverse stream in registers
 * (reverse_stream: fixed indices, a wave-uniform shift) and keeps one of the
 * two under a per-lane select -- no divergent branch around two packers.
 * LDS per wave: stage_slot_bytes(m).  Every thread of the block must call it. */
template <int MAXW>
__device__ __forceinline__ void stage_strand_codes(const uint8_t* __restrict__ ascii, uint64_t num, uint32_t m,
                                                   uint8_t* __restrict__ lds, uint32_t (&cw)[MAXW], uint32_t strands)
{
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t both = strands == 3u ? 1u : 0u;
  const uint32_t rpr = stage_rows(m);
  const uint32_t lr = lane >> both;                  /* the lane's read among its wave's 64 >> both */
  const bool rev = both ? (lane & 1u) != 0u : true;
  uint8_t* wl = lds + wv * stage_slot_bytes(m);
  const uint64_t q0 = ((uint64_t) blockIdx.x * 256 + wv * 64) >> both;
#pragma unroll 1
  for (uint32_t h = 0; h < (64u >> both) / rpr; ++h) {
    const uint64_t r0 = q0 + h * rpr;
    const uint64_t nr = r0 < num ? (num - r0 < rpr ? num - r0 : rpr) : 0;
    const uint32_t n16 = (uint32_t) ((nr * m + 15) / 16);           /* <= 15 bytes of slack read */
    const uint4* src = reinterpret_cast<const uint4*>(ascii + r0 * m);   /* r0*m % 16 == 0 */
    for (uint32_t i = lane; i < n16; i += 64) reinterpret_cast<uint4*>(wl)[i] = src[i];
    __syncthreads();
    if (lr / rpr == h) {
      uint32_t fw[MAXW], rv[MAXW];
      row_codes<MAXW>(wl, (uint64_t) (lr % rpr) * m, m, fw);
      reverse_stream<MAXW>(fw, m, rv);
#pragma unroll
      for (int k = 0; k < MAXW; ++k) cw[k] = rev ? rv[k] : fw[k];
    }
    __syncthreads();
  }
}

/* The fused task kernel of a strand search: ns * num tasks on the ASCII reads
 * of num reads, K <= 2, m % K == 0, m <= 16 * MAXW.  Only the staging differs
 * from task_kernel<G, 1, MAXW, SPLIT, true>: the jump start and skip_walk are
 * the same (without a skip table skip_walk takes every K-step from the code
 * words in LDS).  The forward kernels are not touched.  TR: as for
 * task_words_skip_kernel, task t's record at trace[t]. */
template <class G, int MAXW, int SPLIT, class TR = NoTrace>
__global__ __launch_bounds__(256) void task_strands_kernel(IdxArgs ix, const uint8_t* __restrict__ ascii, uint32_t m,
                                                           uint64_t num, uint32_t steps, uint32_t strands,
                                                           uint32_t* __restrict__ res, typename TR::Out trace)
{
  static_assert(G::K <= 2 && MAXW > 0, "strand staging: task kernels at K <= 2");
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  stage_strand_codes<MAXW>(ascii, num, m, stage, cw, strands);   /* whole block, before any exit */
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= (strands == 3u ? 2u : 1u) * num) return;
  uint32_t L = 0, R = ix.bwtsize, skip = 0;
  if (ix.ftab && steps >= ix.ftab_steps) {   /* wave-uniform: jump start from the ftab */
    skip = ix.ftab_steps;
    const FtabAt lr = ftab_lookup(ix, cw[0]);
    L = lr.L;
    R = lr.R;
  }
  skip_walk<G, MAXW, SPLIT, false, TR>(ix, cw, steps, skip, L, R, TR::at(trace, t));
  if constexpr (TR::ON) TR::at(trace, t)->w = trace_launch_id<SPLIT, MAXW, KFMI_TRACE_KERNEL_TASK_STRANDS>(ix);
  *reinterpret_cast<uint2*>(res + 2 * t) = make_uint2(L, R);
}

/* Seed search (kfmi_seeds.hip): task t's start state and its
 * walk.  The last rem bases are one unit: a remainder-table entry that is not
 * empty starts the first segment at base m, an empty one means that unit does
 * not occur and the walk starts past it.  The jump start is seed_walk's own
 * first round.  Slot t * S + s of either array is record s of task t.
 * TR = Trace: seed_walk's record of task t goes to trace[t], its word 3 the
 * launch identity of the kernel KID (KFMI_TRACE_KERNEL_*). */
template <class G, int MAXW, int SPLIT, int KID, class TR = NoTrace>
__device__ __forceinline__ void seed_task(const IdxArgs& ix, const uint32_t (&cw)[MAXW], uint32_t rc, uint32_t m,
                                          uint32_t steps, uint64_t t, uint32_t S, uint32_t* __restrict__ res,
                                          uint32_t* __restrict__ spans, typename TR::Out trace)
{
  const uint32_t mk = m - ix.rem;
  uint32_t L = 0, R = ix.bwtsize, e = mk;
  if (ix.rem) {   /* wave-uniform */
    const uint2 lr = ix.rtab[rc];
    if (lr.y > lr.x) {
      L = lr.x;
      R = lr.y;
      e = m;
    }
  }
  if constexpr (TR::ON)
    seed_walk<G, MAXW, SPLIT, TR>(ix, cw, steps, mk, L, R, e, S, reinterpret_cast<uint2*>(res) + t * S,
                                  reinterpret_cast<uint2*>(spans) + t * S, TR::at(trace, t),
                                  trace_launch_id<SPLIT, MAXW, KID>(ix));
  else
    seed_walk<G, MAXW, SPLIT>(ix, cw, steps, mk, L, R, e, S, reinterpret_cast<uint2*>(res) + t * S,
                              reinterpret_cast<uint2*>(spans) + t * S);
}

/* The three seed kernels: an existing staging each, then seed_task.  They are
 * launched with or without a skip table.
 * Forward reads, fused packing: task_kernel's staging (m <= 16 * MAXW, any rem). */
template <class G, int MAXW, int SPLIT, class TR = NoTrace>
__global__ __launch_bounds__(256) void seed_kernel(IdxArgs ix, const uint8_t* __restrict__ ascii, uint32_t m,
                                                   uint64_t num, uint32_t steps, uint32_t S,
                                                   uint32_t* __restrict__ res, uint32_t* __restrict__ spans,
                                                   typename TR::Out trace)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  uint32_t rc = 0;
  stage_query_codes<MAXW>(ascii, num, m, stage, cw, ix.rem, rc);   /* whole block, before any exit */
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= num) return;
  seed_task<G, MAXW, SPLIT, KFMI_TRACE_KERNEL_SEED, TR>(ix, cw, rc, m, steps, t, S, res, spans, trace);
}

/* Either strand or both, fused packing: task_strands_kernel's staging (m % K == 0). */
template <class G, int MAXW, int SPLIT, class TR = NoTrace>
__global__ __launch_bounds__(256) void seed_strands_kernel(IdxArgs ix, const uint8_t* __restrict__ ascii, uint32_t m,
                                                           uint64_t num, uint32_t steps, uint32_t strands, uint32_t S,
                                                           uint32_t* __restrict__ res, uint32_t* __restrict__ spans,
                                                           typename TR::Out trace)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
  uint32_t cw[MAXW];
  stage_strand_codes<MAXW>(ascii, num, m, stage, cw, strands);   /* whole block, before any exit */
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= (strands == 3u ? 2u : 1u) * num) return;
  seed_task<G, MAXW, SPLIT, KFMI_TRACE_KERNEL_SEED_STRANDS, TR>(ix, cw, 0u, m, steps, t, S, res, spans, trace);
}

/* Code words a pack launch or the host wrote (num task columns of qp, row
 * nwords the remainder codes): task_words_skip_kernel's loads. */
template <class G, int MAXW, int SPLIT, class TR = NoTrace>
__global__ __launch_bounds__(256) void seed_words_kernel(IdxArgs ix, const uint32_t* __restrict__ qp, uint32_t m,
                                                         uint64_t num, uint32_t steps, uint32_t nwords, uint32_t S,
                                                         uint32_t* __restrict__ res, uint32_t* __restrict__ spans,
                                                         typename TR::Out trace)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (t >= num) return;
  uint32_t cw[MAXW];
#pragma unroll
  for (int k = 0; k < MAXW; ++k) cw[k] = (uint32_t) k < nwords ? qp[(uint64_t) k * num + t] : 0u;
  const uint32_t rc = ix.rem ? qp[(uint64_t) nwords * num + t] & ((1u << (2u * ix.rem)) - 1u) : 0u;
  seed_task<G, MAXW, SPLIT, KFMI_TRACE_KERNEL_SEED_WORDS, TR>(ix, cw, rc, m, steps, t, S, res, spans, trace);
}

/* ftab construction: [L, R) of every code stream v of ftab_steps K-steps
 * (the search's own first steps, from [0, n+1)), each end by lf_stream --
 * the per-row step of every non-search kernel.  Round 5 detoured this build
 * through the task kernels' fetch when lf_stream's K = 1, d = 64 AltCounters
 * form returned wrong entries; the cause was the 16-byte load at 8-byte
 * alignment LLVM formed from two 8-byte plane loads, which
 * load_words now keeps out, so the build is lf_stream's again and
 * test_ftab_table_every_entry checks its tables entry by entry.
 *
 * Level by level, in place, one launch per level t = 0 .. ftab_steps-1
 * (launch_ftab): the entries of the `parents` = NC^t code streams of t K-steps
 * sit at out[0 .. parents) (level 0: the one interval [0, n+1), not stored),
 * and the entry of v followed by K-step c is out[v | c << 2Kt].  The thread of
 * parent v reads its own [L, R) first and then writes its NC children: child 0
 * overwrites only that parent's slot, every other child lands at or past
 * `parents`, where this level reads nothing.  All NC children of a parent step
 * from the same two rows, so they read the same lines: the deepest level
 * fetches NC times fewer lines than a walk per entry, and no level repeats the
 * steps of the ones before it. */
template <class G>
__global__ __launch_bounds__(256) void ftab_level_kernel(IdxArgs ix, uint32_t t, uint64_t parents, uint2* out)
{
  /* grid-stride: the launch's grid is capped (grid_blocks) */
  for (uint64_t v = (uint64_t) blockIdx.x * 256 + threadIdx.x; v < parents; v += (uint64_t) gridDim.x * 256) {
    uint2 lr = make_uint2(0u, ix.bwtsize);
    if (t) lr = out[v];
#pragma unroll 1
    for (uint32_t c = 0; c < (uint32_t) G::NC; ++c) {
      uint32_t sx[2 * G::K];
      plane_xor<G::K>(c, sx);
      const uint32_t L = lf_stream<G>(ix, lr.x, c, sx);
      const uint32_t R = lf_stream<G>(ix, lr.y, c, sx);
      out[v | ((uint64_t) c << (2 * G::K * t))] = make_uint2(L, R);
    }
  }
}

/* Skip table, level 0 (DESIGN.md 5a'): entry i = one K-step from the one-row
 * interval [i, i+1) with row i's own K-mer code c -- the only code that can
 * keep the interval non-empty -- taken on both ends by lf_stream, the search's
 * own step (as ftab_level_kernel takes it), so every backend's semantics,
 * lf_cap and the padding entries carry over; lf_row would take the
 * AltCounters correction off, which the search keeps.  The entry {L', c} is
 * valid iff the result is one row again (R' == L' + 1), i is no '$' row D_s
 * (its K-mer holds the '$': no read code matches it) and L' is a table row.
 *
 * Exactness: skip_double_kernel composes two valid entries into one of twice
 * the steps, {in[in[i].row].row, in[i].code | in[in[i].row].code << bits},
 * and leaves it invalid when either half is.  By induction on the level every
 * valid entry is exactly the composition of that many search steps from
 * [i, i+1), each on a one-row interval, with the codes it records; a search
 * that finds its next code bits equal to the entry's takes those same steps,
 * so the jump changes no result.  A read whose bits differ does not use the
 * entry at all. */
template <class G>
__global__ __launch_bounds__(256) void skip_level0_kernel(IdxArgs ix, uint64_t rows, uint2* __restrict__ out)
{
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256) {
    const uint32_t X = (uint32_t) i;
    const uint32_t c = row_code<G>(ix, X);
    uint32_t sx[2 * G::K];
    plane_xor<G::K>(c, sx);
    const uint32_t L = lf_stream<G>(ix, X, c, sx);
    const uint32_t R = lf_stream<G>(ix, X + 1u, c, sx);
    bool ok = R == L + 1u && (uint64_t) L < rows;
#pragma unroll
    for (int s = 0; s < G::K; ++s) ok = ok && ix.dl.dpos[s] != X;
    out[i] = ok ? make_uint2(L, c) : make_uint2(SKIP_NONE, 0u);
  }
}

/* Text jump, the code stream of the text (DESIGN.md 5a'', IdxArgs::jtext): one
 * thread per word.  Word w holds the 16 bases before text position
 * p0 = n - 16w, base p0-1-r at bits 2r; they are the K-mer codes of the rows
 * of suffixes p0, p0 - K, ... (row_code: base p-1-s at bits 2s), found through
 * isa -- consecutive words read isa 16 entries apart, one index line per K
 * bases, whole words stored.  Bases before position 0 and the words past the
 * text are zero.  With `split` the index gather goes out as four 16-lane
 * groups, like the task kernels' (the rows are random in the index). */
template <class G>
__global__ __launch_bounds__(256) void jump_text_kernel(IdxArgs ix, const uint32_t* __restrict__ isa, uint64_t n,
                                                        uint64_t words, uint32_t split, uint32_t* __restrict__ out)
{
  const int grp = (int) (threadIdx.x & 63) / 16;
  for (uint64_t w0 = (uint64_t) blockIdx.x * 256 + (threadIdx.x & ~63u); w0 < words; w0 += (uint64_t) gridDim.x * 256) {
    const uint64_t w = w0 + (threadIdx.x & 63u);
    uint32_t v = 0;
#pragma unroll 1
    for (uint32_t u = 0; u < 16u / (uint32_t) G::K; ++u) {
      const uint64_t back = 16ull * w + (uint64_t) u * G::K;   /* p = n - back */
      const bool on = w < words && back < n;                    /* p >= 1: base p-1 exists */
      const uint64_t p = on ? n - back : 0;
      const uint32_t row = on ? isa[p] : 0u;
      const bool ok = on && row < ix.bwtsize;
      uint32_t c = 0;
      if (split) {   /* wave-uniform */
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (ok && grp == g) c = row_code<G>(ix, row);
      } else if (ok) {
        c = row_code<G>(ix, row);
      }
      if (p < (uint64_t) G::K) c &= (1u << (2u * (uint32_t) p)) - 1u;   /* only bases p-1 .. 0 are text */
      v |= c << (2u * (uint32_t) G::K * u);
    }
    if (w < words) out[w] = v;
  }
}

/* Text jump, the line table (DESIGN.md 5a''', IdxArgs::jsa): one thread per
 * output dword, streaming.  Dword t of line j is, for t < S, isa[n - e] at
 * e = S * j + t (SKIP_NONE where e > n), and for t >= S the stream slots
 * [16 * (j + t - 31), + 16): the line's text half starts on a word boundary
 * of jtext, so a text dword is a copy of one of its words, zero outside them. */
template <class G>
__global__ __launch_bounds__(256) void jump_lines_kernel(const uint32_t* __restrict__ isa, const uint32_t* __restrict__ text,
                                                         uint64_t n, uint64_t words, uint64_t lines,
                                                         uint32_t* __restrict__ out)
{
  const uint64_t total = lines * JUMP_LINE_DW;
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t) gridDim.x * 256) {
    const uint64_t j = i / JUMP_LINE_DW;
    const uint32_t t = (uint32_t) (i % JUMP_LINE_DW);
    uint32_t v;
    if (t < JUMP_LINE_TEXT) {
      const uint64_t e = j * JUMP_LINE_S + t;
      v = e <= n ? isa[n - e] : SKIP_NONE;
    } else {
      const uint64_t w = j + t;   /* word w - (DW - 1) of the stream */
      v = w >= JUMP_LINE_DW - 1 && w - (JUMP_LINE_DW - 1) < words ? text[w - (JUMP_LINE_DW - 1)] : 0u;
    }
    out[i] = v;
  }
}

/* Remainder table for reads with m % K = rem (1 <= rem < K): [L, R) of every
 * rem-base string x (base m-1 at bits 0-1, the code order of the K-steps).
 * A K-step from [0, n+1) gives the suffix-array range of a K-mer, so
 *   R(x) = R of x.T^(K-rem)  (the last K-mer range inside x's),
 *   L(x) = L of x.A^(K-rem) - #{j < K-rem : T ends with x.A^j}
 * (the suffixes x.A^j.$ sort below x.A^(K-rem) but inside x's range).  Whether
 * T ends with x.A^j is read from row 0 (suffix "$"), whose K-mer code holds
 * T[n-1-s] at bits 2s.  One thread per x (4^rem <= 64). */
template <class G>
__global__ __launch_bounds__(64) void rem_tab_kernel(IdxArgs ix, uint32_t rem, uint2* __restrict__ out)
{
  const uint32_t x = threadIdx.x;
  if (rem == 0 || rem >= (uint32_t) G::K || x >= (1u << (2 * rem))) return;
  const uint32_t pad = 2 * ((uint32_t) G::K - rem);
  const uint32_t cA = x << pad, cT = cA | ((1u << pad) - 1u);
  uint32_t sx[2 * G::K];
  plane_xor<G::K>(cA, sx);
  uint32_t L = lf_stream<G>(ix, 0u, cA, sx);
  plane_xor<G::K>(cT, sx);
  const uint32_t R = lf_stream<G>(ix, ix.bwtsize, cT, sx);
  const uint32_t n = ix.bwtsize - 1u;
  const uint32_t tail = row_code<G>(ix, 0u);
  for (uint32_t j = 0; j + rem < (uint32_t) G::K; ++j)
    if (j + rem <= n && (tail & ((1u << (2 * j)) - 1u)) == 0u && ((tail >> (2 * j)) & ((1u << (2 * rem)) - 1u)) == x)
      --L;
  out[x] = make_uint2(L, R);
}

/* distinct d-blocks touched per step (1 if L/d == R/d else 2): the
 * dedup-aware algorithmic traffic of SURVEY 8(d).  Same LF math as the
 * task kernel; a separate launch so the timed kernels carry no counters. */
template <class G>
__global__ __launch_bounds__(256) void count_blocks_kernel(IdxArgs ix, const uint32_t* __restrict__ qp, uint64_t num,
                                                           uint32_t steps, uint32_t nwords,
                                                           unsigned long long* __restrict__ total)
{
  const uint64_t q = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0;
  if (q < num) {
    uint32_t L = 0, R = ix.bwtsize;
    if (ix.rem) {   /* a table lookup, no index line */
      const uint2 lr = ix.rtab[qp[(uint64_t) nwords * num + q]];
      L = lr.x;
      R = lr.y;
    }
    for (uint32_t t = 0; t < steps; ++t) {
      const uint32_t word = qp[(uint64_t) (t / G::SPW) * num + q];
      const uint32_t c = (word >> (2 * G::K * (t % G::SPW))) & (uint32_t) (G::NC - 1);
      uint32_t sx[2 * G::K];
      plane_xor<G::K>(c, sx);
      cnt += (L / (uint32_t) G::D == R / (uint32_t) G::D) ? 1u : 2u;
      L = lf_stream<G>(ix, L, c, sx);
      R = lf_stream<G>(ix, R, c, sx);
    }
  }
  /* wave reduction, one atomic per wave */
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long) cnt);
}

/* Derivation of a 2K-step index from a K-step one (kfmi_derive_index_gpu):
 * row i's 2K-mer code is its own K-mer code (T[p-1-s], s < K, p = SA[i]) and,
 * above it, the K-mer code of row LF_K(i) -- the row of suffix p - K, whose
 * K-mer is T[p-1-K-s].  One thread per row (grid-stride).  The K rows whose
 * K-mer holds the '$' (D_s, s < K) have no valid LF: their upper half is
 * written by the host from the text's tail (row 0's code, see the caller);
 * a row whose LF lands on D_s is the row of suffix K + s, the new D_{K+s}
 * (isa[s]). */
/* The LF_K successor of every row for the walk check (check_lf_walks,
 * kfmi_search.hip): next[X] = LF_K(X) as a locate walk takes it (lf_row), a
 * '$' row D_s its own successor; an image past the last row sets *bad. */
template <class G>
__global__ __launch_bounds__(256) void lf_next_kernel(IdxArgs ix, uint64_t rows, uint32_t* __restrict__ next,
                                                      uint32_t* __restrict__ bad)
{
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256) {
    const uint32_t X = (uint32_t) i;
    bool dollar = false;
#pragma unroll
    for (int s = 0; s < G::K; ++s) dollar = dollar || ix.dl.dpos[s] == X;
    uint32_t j = X;
    if (!dollar) {
      j = lf_row<G>(ix, X);
      if ((uint64_t) j >= rows) {
        atomicOr(bad, 1u);
        j = X;
      }
    }
    next[i] = j;
  }
}

template <class G>
__global__ __launch_bounds__(256) void derive_codes_kernel(IdxArgs ix, uint64_t rows, uint8_t* __restrict__ codes,
                                                           uint32_t* __restrict__ isa)
{
  for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < rows; i += (uint64_t) gridDim.x * 256) {
    const uint32_t X = (uint32_t) i;
    const uint32_t c = row_code<G>(ix, X);
    bool dollar = false;
#pragma unroll
    for (int s = 0; s < G::K; ++s) dollar = dollar || ix.dl.dpos[s] == X;
    uint32_t up = 0;
    if (!dollar) {
      uint32_t sx[2 * G::K];
      plane_xor<G::K>(c, sx);
      const uint32_t j = lf_stream<G>(ix, X, c, sx);
      up = row_code<G>(ix, j);
#pragma unroll
      for (int s = 0; s < G::K; ++s)
        if (ix.dl.dpos[s] == j) isa[s] = X;
    }
    codes[i] = (uint8_t) (c | (up << (2 * G::K)));
  }
}

/* 128-B lines one LF end's task-kernel fetch touches (fetch_block: the
 * planes, the counter word and, when the
 * step is counted forward from block b-1 (line_local_prev), b-1's planes).
 * Returns how many ids it appended to ln; *extra = 1 when the counter lies
 * outside the planes' line(s), *prev = 1 for a line-local step. */
template <class G>
__device__ __forceinline__ int lf_lines(const IdxArgs& ix, uint32_t X, uint32_t c, uint64_t* ln, uint32_t* extra,
                                        uint32_t* prev)
{
  const uint32_t b = X / (uint32_t) G::D;
  Where<G> w = locate<G>(ix, b, c);
  line_local_prev<G>(ix, b, c, w);
  int n = 0;
  const uint64_t p0 = (uint64_t) (uintptr_t) w.planes >> 7, p1 = (uint64_t) (uintptr_t) (w.planes + G::BMW - 1) >> 7;
  ln[n++] = p0;
  if (p1 != p0) ln[n++] = p1;
  const uint64_t cl = (uint64_t) (uintptr_t) w.cnt >> 7;
  *extra = (cl != p0 && cl != p1) ? 1u : 0u;
  if (*extra) ln[n++] = cl;
  *prev = w.prev ? 1u : 0u;
  if (w.prev) {
    const uint64_t q0 = (uint64_t) (uintptr_t) w.pplanes >> 7, q1 = (uint64_t) (uintptr_t) (w.pplanes + G::BMW - 1) >> 7;
    if (q0 != p0 && q0 != p1) ln[n++] = q0;
    if (q1 != q0 && q1 != p0 && q1 != p1) ln[n++] = q1;
  }
  return n;
}

/* Statistics only (not timed): per batch, the distinct 128-B lines each
 * K-step's fetches touch (L's block, and R's when it is another block, as the
 * task kernel fetches them; lines shared by the two ends counted once) --
 * out[0]; the ends whose counter lies outside their planes' line -- out[1];
 * the ends fetched -- out[2]; the ends counted forward from block b-1
 * (line-local) -- out[3].  Compared with the PMC's fabric requests per read
 * this splits a layout's requests into the structural lines its fetches need
 * and what the caches absorb. */
template <class G>
__global__ __launch_bounds__(256) void count_lines_kernel(IdxArgs ix, const uint32_t* __restrict__ qp, uint64_t num,
                                                          uint32_t steps, uint32_t nwords,
                                                          unsigned long long* __restrict__ out)
{
  const uint64_t q = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  uint32_t lines = 0, extra = 0, ends = 0, prevs = 0;
  if (q < num) {
    uint32_t L = 0, R = ix.bwtsize;
    if (ix.rem) {
      const uint2 lr = ix.rtab[qp[(uint64_t) nwords * num + q]];
      L = lr.x;
      R = lr.y;
    }
    for (uint32_t t = 0; t < steps; ++t) {
      const uint32_t word = qp[(uint64_t) (t / G::SPW) * num + q];
      const uint32_t c = (word >> (2 * G::K * (t % G::SPW))) & (uint32_t) (G::NC - 1);
      uint64_t ln[10];
      uint32_t ex, pv;
      int n = lf_lines<G>(ix, L, c, ln, &ex, &pv);
      extra += ex;
      prevs += pv;
      ++ends;
      if (R / (uint32_t) G::D != L / (uint32_t) G::D) {
        n += lf_lines<G>(ix, R, c, ln + n, &ex, &pv);
        extra += ex;
        prevs += pv;
        ++ends;
      }
      for (int i = 0; i < n; ++i) {
        bool dup = false;
        for (int j = 0; j < i; ++j) dup = dup || ln[j] == ln[i];
        lines += dup ? 0u : 1u;
      }
      uint32_t sx[2 * G::K];
      plane_xor<G::K>(c, sx);
      L = lf_stream<G>(ix, L, c, sx);
      R = lf_stream<G>(ix, R, c, sx);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    lines += __shfl_xor(lines, off);
    extra += __shfl_xor(extra, off);
    ends += __shfl_xor(ends, off);
    prevs += __shfl_xor(prevs, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out + 0, (unsigned long long) lines);
    atomicAdd(out + 1, (unsigned long long) extra);
    atomicAdd(out + 2, (unsigned long long) ends);
    atomicAdd(out + 3, (unsigned long long) prevs);
  }
}

/* ------------------------------------------------------------------------ */
/* dispatch tables                                                          */
/* ------------------------------------------------------------------------ */

struct SearchLaunch {
  hipStream_t st;
  IdxArgs ix;
  const uint32_t* qp;
  const uint8_t* ascii;   /* fused packing: ASCII rows of m bases */
  uint32_t m;
  int maxw;               /* 0: packed words in qp; 8/16: fused packing */
  int words_maxw;         /* strand searches, maxw == 0: 8/16 = the words in qp fit that many registers and
                             the task backends walk them with the skip table when ix.skip is set
                             (task_words_skip_kernel); 0 = the plain walk of the words, as every other caller */
  uint32_t strands;       /* strand searches with fused packing (maxw != 0, task backends, K <= 2, m % K == 0):
                             2 / 3 = num reads run as 1 / 2 tasks each (task_strands_kernel); 0 = forward */
  uint64_t num;
  uint32_t steps, nwords;
  uint32_t* res;
  /* seed searches (launch_seeds): res holds the intervals and spans the {start, len} pairs, max_seeds slots
     per task in each; maxw / words_maxw / strands as for a strand search, strands 0 = forward */
  uint32_t* spans;
  uint32_t max_seeds;
  /* locate */
  const uint32_t* sa;
  uint32_t sa_log2;
  const uint64_t* off;
  const uint32_t* owner;
  uint64_t total;
  uint32_t* pos;
  unsigned long long* slot_ctr;   /* walk slot queue, zeroed before the launch */
  uint32_t slot_chunk;            /* slots per queue take (64 .. 4096) */
  /* ftab build */
  uint2* ftab_out;
  uint32_t ftab_steps;
  uint64_t ftab_n;
  /* remainder table build: rem bases -> ftab_out */
  uint32_t rem;
  /* skip table, level 0 (Op::Skip0): num rows -> skip_out */
  uint2* skip_out;
  /* index derivation: 2K-mer code per row (num rows), the rows of suffixes K..2K-1 */
  uint8_t* derive_codes;
  uint32_t* derive_isa;
  /* walk check (Op::PermCheck): every row's LF_K successor, and the flag of an image past the rows */
  uint32_t* perm_next;
  uint32_t* perm_bad;
  /* text jump, the code stream (Op::JumpText): num = n bases through jump_isa -> jump_words words of jump_text */
  const uint32_t* jump_isa;
  uint32_t* jump_text;
  uint64_t jump_words;
  uint32_t jump_split;
  /* text jump, the line table (Op::JumpLines): jump_isa and jump_words words of jump_text of a num-base text ->
     jump_line_count(num) lines at jump_lines */
  uint32_t* jump_lines;
  /* walk trace (trace_one, strands_trace_one, seeds_trace_one): one record per read or task; null in every
     other launch */
  uint4* trace;
};

/* The geometries that have seed, traced and traced strand kernels, and the text
 * jump: the plain-counter layouts at K <= 2 (KFMI_FOR_LANE_GEOMETRIES below). */
constexpr bool lane_kernels(uint32_t K, int lay) { return (lay == LAY_INTER || lay == LAY_MID) && K >= 1 && K <= 2; }

/* The fetch form (the SPLIT template value, fetch_ends_split) of the task, strand
 * and seed kernels of geometry G: `want` is the table-size class (IdxArgs::split,
 * split_for: 1, 2 or 4) and mw the MAXW of the kernel that will run, 0 for the
 * plain walk of packed words.  The split only exists for the one-line-per-block
 * path (SMALL: d <= 128 at K = 2): the asm fetch in one group below 2 GB and in
 * two groups above (X4 geometries); else the C++ fetch, in four groups at class
 * 4 and, for the 8-register kernels, at class 2.  The one rule: launch_task,
 * launch_seeds and the plan's test accessor (kfmi_launch_plan) all ask here. */
template <class G>
constexpr int fetch_form(uint32_t want, int mw)
{
  if constexpr (G::SMALL && X4<G>::OK) return want == 1 ? 8 : 7;
  else if constexpr (G::SMALL) return (want == 4 || (want == 2 && mw == 8)) ? 4 : 1;
  else return 1;
}

/* the statement with the constant NAME = V in scope (variadic: a launch arrives expanded, commas and all) */
#define KFMI_WITH_CONST(NAME, V, ...) \
  {                                   \
    constexpr int NAME = V;           \
    __VA_ARGS__;                      \
  }
/* CALL with FORM = fetch_form<G>(WANT, MW) as a constant; under if constexpr, so
 * that each geometry gets only the forms it can be launched with. */
#define KFMI_WITH_FETCH_FORM(G, WANT, MW, CALL)                                                 \
  do {                                                                                          \
    [[maybe_unused]] const int form_ = fetch_form<G>(WANT, MW);                                 \
    if constexpr (G::SMALL && X4<G>::OK) {                                                      \
      if (form_ == 8) KFMI_WITH_CONST(FORM, 8, CALL) else KFMI_WITH_CONST(FORM, 7, CALL)        \
    } else if constexpr (G::SMALL) {                                                            \
      if (form_ == 4) KFMI_WITH_CONST(FORM, 4, CALL) else KFMI_WITH_CONST(FORM, 1, CALL)        \
    } else KFMI_WITH_CONST(FORM, 1, CALL)                                                       \
  } while (0)
/* LAUNCH with MAXW = 8 or 16 as a constant, by the run-time register count MW */
#define KFMI_WITH_MAXW(MW, LAUNCH)                                                              \
  do {                                                                                          \
    if ((MW) == 8) KFMI_WITH_CONST(MAXW, 8, LAUNCH) else KFMI_WITH_CONST(MAXW, 16, LAUNCH)      \
  } while (0)

/* TR = Trace (kfmi_search_trace, trace_one below): the same choices with the
 * traced kernels, which exist for what the text jump serves -- the fused
 * forward walk on the plain layouts at K <= 2; there a search without any table
 * takes the tables' kernel too, so that skip_walk records its plain steps.
 * TR = StrandTrace (kfmi_search_strands_trace, strands_trace_one below): the
 * strand kernels' traced forms and nothing else -- the plain walk of packed
 * words has none.  The caller has refused everything else. */
template <class G, int SPLIT, class TR = NoTrace>
static void launch_task_split(const SearchLaunch& a)
{
  static_assert(!TR::ON || lane_kernels(G::K, G::LAY), "walk trace: fused forward task kernels, plain layouts, K <= 2");
  const typename TR::Out tr = TR::from(a.trace);
  const dim3 grid((uint32_t) ((a.num + 255) / 256)), block(256);
  if (a.maxw) {
    const size_t lds = 4 * (size_t) stage_slot_bytes(a.m);
    /* the walk with the tables, and the strand staging; LDS: the staging, then 64 x maxw code words per wave */
    const size_t lds_skip = std::max(lds, (size_t) 4 * 64 * 4 * (size_t) a.maxw);
    if constexpr (G::K <= 2 && (!TR::ON || TR::STRANDS)) {
      if (a.strands) {   /* strand-aware staging, then the fused kernel's own walk */
        const uint64_t tblocks = ((a.strands == 3u ? 2u : 1u) * a.num + 255) / 256;
        KFMI_WITH_MAXW(a.maxw, hipLaunchKernelGGL((task_strands_kernel<G, MAXW, SPLIT, TR>), dim3((uint32_t) tblocks), block,
                                                  lds_skip, a.st, a.ix, a.ascii, a.m, a.num, a.steps, a.strands, a.res, tr));
        return;
      }
    }
    if constexpr (!TR::STRANDS) {   /* that policy has the strand kernels only (the caller refused the rest) */
      if constexpr (G::K <= 2) {
        if (TR::ON || a.ix.skip || a.ix.jsa) {
          if constexpr (G::LAY == LAY_INTER || G::LAY == LAY_MID) {
            if (a.ix.jsa) {   /* with the text jump (DESIGN.md 5a'') */
              IdxArgs ix = a.ix;
              if ((ix.jump_split & JUMP_LINES_GROUPED) && a.m > JUMP_LINES_GROUPED_MAX_M)
                ix.jump_split &= ~(JUMP_LINES | JUMP_LINES_GROUPED);   /* long reads: the flat tables' form is faster */
              KFMI_WITH_MAXW(a.maxw, hipLaunchKernelGGL((task_kernel<G, 1, MAXW, SPLIT, true, true, TR>), grid, block, lds_skip,
                                                        a.st, ix, a.qp, a.ascii, a.m, a.num, a.steps, a.nwords, a.res, tr));
              return;
            }
          }
          KFMI_WITH_MAXW(a.maxw, hipLaunchKernelGGL((task_kernel<G, 1, MAXW, SPLIT, true, false, TR>), grid, block, lds_skip,
                                                    a.st, a.ix, a.qp, a.ascii, a.m, a.num, a.steps, a.nwords, a.res, tr));
          return;
        }
      }
      if constexpr (!TR::ON)
        KFMI_WITH_MAXW(a.maxw, hipLaunchKernelGGL((task_kernel<G, 1, MAXW, SPLIT>), grid, block, lds, a.st, a.ix, a.qp,
                                                  a.ascii, a.m, a.num, a.steps, a.nwords, a.res, tr));
    }
  } else if constexpr (!TR::ON || TR::STRANDS) {
    if constexpr (G::K <= 2) {
      if (a.ix.skip && a.words_maxw) {   /* strand searches: the skip-table walk on packed words */
        const size_t lds_skip = (size_t) 4 * 64 * 4 * (size_t) a.words_maxw;
        KFMI_WITH_MAXW(a.words_maxw, hipLaunchKernelGGL((task_words_skip_kernel<G, MAXW, SPLIT, TR>), grid, block, lds_skip,
                                                        a.st, a.ix, a.qp, a.num, a.steps, a.nwords, a.res, tr));
        return;
      }
    }
    if constexpr (!TR::ON)
      hipLaunchKernelGGL((task_kernel<G, 1, 0, SPLIT>), grid, block, 0, a.st, a.ix, a.qp, a.ascii, a.m, a.num, a.steps,
                         a.nwords, a.res, tr);
  }
}

/* mw: the words-skip kernel takes the fused skip kernel's form; the plain walk
 * of words keeps its own. */
template <class G, class TR = NoTrace>
static hipError_t launch_task(const SearchLaunch& a)
{
  const int mw = a.maxw ? a.maxw : (a.ix.skip ? a.words_maxw : 0);
  KFMI_WITH_FETCH_FORM(G, a.ix.split, mw, (launch_task_split<G, FORM, TR>(a)));
  if constexpr (G::SMALL && X4<G>::OK) {
    /* the C++ fetch forms of the asm geometries: never launched; named so that the
     * units hold the kernels they held before the rule moved to fetch_form */
    (void) &launch_task_split<G, 4, TR>;
    (void) &launch_task_split<G, 1, TR>;
  }
  return hipGetLastError();
}

/* Seed searches: the kernel by where the code words come from -- fused packing
 * (a.maxw; a.strands 2 / 3 the strand staging on a.num reads), else the
 * a.num task columns in a.qp (a.words_maxw registers). */
template <class G, int SPLIT, class TR = NoTrace>
static void launch_seeds_split(const SearchLaunch& a)
{
  const typename TR::Out tr = TR::from(a.trace);
  const dim3 grid((uint32_t) ((a.num + 255) / 256)), block(256);
  if (a.maxw) {   /* LDS: the staging, then 64 x maxw code words per wave */
    const size_t lds = std::max((size_t) 4 * stage_slot_bytes(a.m), (size_t) 4 * 64 * 4 * (size_t) a.maxw);
    if (a.strands) {
      const uint64_t tblocks = ((a.strands == 3u ? 2u : 1u) * a.num + 255) / 256;
      KFMI_WITH_MAXW(a.maxw, hipLaunchKernelGGL((seed_strands_kernel<G, MAXW, SPLIT, TR>), dim3((uint32_t) tblocks), block, lds,
                                                a.st, a.ix, a.ascii, a.m, a.num, a.steps, a.strands, a.max_seeds, a.res,
                                                a.spans, tr));
    } else {
      KFMI_WITH_MAXW(a.maxw, hipLaunchKernelGGL((seed_kernel<G, MAXW, SPLIT, TR>), grid, block, lds, a.st, a.ix, a.ascii, a.m,
                                                a.num, a.steps, a.max_seeds, a.res, a.spans, tr));
    }
  } else {
    const size_t lds = (size_t) 4 * 64 * 4 * (size_t) a.words_maxw;
    KFMI_WITH_MAXW(a.words_maxw, hipLaunchKernelGGL((seed_words_kernel<G, MAXW, SPLIT, TR>), grid, block, lds, a.st, a.ix,
                                                    a.qp, a.m, a.num, a.steps, a.nwords, a.max_seeds, a.res, a.spans, tr));
  }
}

/* The fetch form is fetch_form's for the kernel's registers, as for launch_task.
 * TR = Trace (kfmi_search_seeds_trace): the same choices with the traced kernels. */
template <class G, class TR = NoTrace>
static hipError_t launch_seeds(const SearchLaunch& a)
{
  if constexpr (lane_kernels(G::K, G::LAY)) {
    const int mw = a.maxw ? a.maxw : a.words_maxw;
    if (mw != 8 && mw != 16) return hipErrorInvalidValue;
    KFMI_WITH_FETCH_FORM(G, a.ix.split, mw, (launch_seeds_split<G, FORM, TR>(a)));
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <class G>
static hipError_t launch_coop(const SearchLaunch& a)
{
  return coop_launch<G>(a.st, a.ix, a.qp, a.ascii, a.m, a.maxw, a.num, a.steps, a.nwords, a.res);
}

template <class G>
static hipError_t launch_count(const SearchLaunch& a, unsigned long long* d_total)
{
  const uint64_t blocks = (a.num + 255) / 256;
  hipLaunchKernelGGL((count_blocks_kernel<G>), dim3((uint32_t) blocks), dim3(256), 0, a.st, a.ix, a.qp, a.num,
                     a.steps, a.nwords, d_total);
  return hipGetLastError();
}


/* K in {1,2}; d in {32,64,128,192,256,448,960} */
#define KFMI_FOR_NB(X, K, LAY) \
  X(K, 1, LAY) X(K, 2, LAY) X(K, 4, LAY) X(K, 6, LAY) X(K, 8, LAY) X(K, 14, LAY) X(K, 30, LAY)
/* the geometries of lane_kernels(): seeds_one, trace_one, strands_trace_one, seeds_trace_one */
#define KFMI_FOR_LANE_GEOMETRIES(X) \
  KFMI_FOR_NB(X, 1, LAY_INTER) KFMI_FOR_NB(X, 2, LAY_INTER) KFMI_FOR_NB(X, 1, LAY_MID) KFMI_FOR_NB(X, 2, LAY_MID)
/* every geometry dispatch_one is instantiated for (kfmi_inst_*.hip) */
#define KFMI_FOR_GEOMETRIES(X)                                                                             \
  KFMI_FOR_NB(X, 1, LAY_INTER) KFMI_FOR_NB(X, 2, LAY_INTER) KFMI_FOR_NB(X, 1, LAY_AC) KFMI_FOR_NB(X, 2, LAY_AC) \
  KFMI_FOR_NB(X, 1, LAY_MID) KFMI_FOR_NB(X, 2, LAY_MID) KFMI_FOR_NB(X, 1, LAY_MIDAC) KFMI_FOR_NB(X, 2, LAY_MIDAC) \
  X(4, 2, LAY_GRP) X(3, 2, LAY_GRP)


/* Locate: enough lanes to fill every CU (8 workgroups of 256 per CU), each
 * lane walking slot after slot (the cooperative walk: from its wave's share of
 * the slot queue). */
template <class G>
static hipError_t launch_locate(const SearchLaunch& a)
{
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    cus = 256;
  uint64_t blocks = (a.total + 255) / 256;
  if constexpr (locate_coop_ok<G>()) {   /* MID lines: one round trip per step (KFMI_LOCATE_COOP=0: per-lane walk) */
    static const bool coop = [] {   /* KFMI_LOCATE_COOP, read once */
      const char* e = getenv("KFMI_LOCATE_COOP");
      return !e || atoi(e) != 0;
    }();
    if (coop) {
      /* 32 KB of LDS per workgroup: 5 fit a CU (4 measured the same within 2 %,
       * profiles/r02/locate_r2ba.jsonl: the walk is not short of lines in flight) */
      hipLaunchKernelGGL((locate_coop_kernel<G>), dim3(grid_blocks(blocks, (uint64_t) cus * 5)), dim3(256), 0, a.st, a.ix,
                         a.sa, a.sa_log2,
                         a.owner, a.total, a.pos, a.slot_ctr, a.slot_chunk);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((locate_kernel<G>), dim3(grid_blocks(blocks, (uint64_t) cus * 8)), dim3(256), 0, a.st, a.ix, a.sa,
                     a.sa_log2, a.owner, a.total, a.pos);
  return hipGetLastError();
}

template <class G>
static hipError_t launch_ftab(const SearchLaunch& a)
{
  /* one launch per level, in stream order: level t reads what level t-1 wrote */
  uint64_t parents = 1;
  for (uint32_t t = 0; t < a.ftab_steps; ++t, parents <<= 2 * G::K) {
    if ((parents << (2 * G::K)) > a.ftab_n) return hipErrorInvalidValue;   /* the children stay inside the table */
    const uint64_t blocks = (parents + 255) / 256;
    hipLaunchKernelGGL((ftab_level_kernel<G>), dim3(grid_blocks(blocks, 1u << 20)), dim3(256), 0, a.st, a.ix, t,
                       parents, a.ftab_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <class G>
static hipError_t launch_rem_tab(const SearchLaunch& a)
{
  hipLaunchKernelGGL((rem_tab_kernel<G>), dim3(1), dim3(64), 0, a.st, a.ix, a.rem, a.ftab_out);
  return hipGetLastError();
}

template <class G>
static hipError_t launch_skip0(const SearchLaunch& a)
{
  if constexpr (G::K <= 2 && G::LAY != LAY_GRP) {
    hipLaunchKernelGGL((skip_level0_kernel<G>), dim3(grid_blocks((a.num + 255) / 256, 1u << 20)), dim3(256), 0, a.st,
                       a.ix, a.num, a.skip_out);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

template <class G>
static hipError_t launch_count_lines(const SearchLaunch& a, unsigned long long* d_out)
{
  const uint64_t blocks = (a.num + 255) / 256;
  hipLaunchKernelGGL((count_lines_kernel<G>), dim3((uint32_t) blocks), dim3(256), 0, a.st, a.ix, a.qp, a.num,
                     a.steps, a.nwords, d_out);
  return hipGetLastError();
}

template <class G>
static hipError_t launch_derive(const SearchLaunch& a)
{
  if constexpr (G::LAY == LAY_INTER && G::K <= 2) {
    hipLaunchKernelGGL((derive_codes_kernel<G>), dim3(grid_blocks((a.num + 255) / 256, 65536)), dim3(256), 0, a.st,
                       a.ix, a.num, a.derive_codes, a.derive_isa);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

template <class G>
static hipError_t launch_perm(const SearchLaunch& a)
{
  hipLaunchKernelGGL((lf_next_kernel<G>), dim3(grid_blocks((a.num + 255) / 256, 65536)), dim3(256), 0, a.st, a.ix,
                     a.num, a.perm_next, a.perm_bad);
  return hipGetLastError();
}

template <class G>
static hipError_t launch_jump_text(const SearchLaunch& a)
{
  if constexpr (G::K <= 2 && (G::LAY == LAY_INTER || G::LAY == LAY_MID)) {
    hipLaunchKernelGGL((jump_text_kernel<G>), dim3(grid_blocks((a.jump_words + 255) / 256, 1u << 20)), dim3(256), 0, a.st,
                       a.ix, a.jump_isa, a.num, a.jump_words, a.jump_split, a.jump_text);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

template <class G>
static hipError_t launch_jump_lines(const SearchLaunch& a)
{
  if constexpr (G::K <= 2 && (G::LAY == LAY_INTER || G::LAY == LAY_MID)) {
    const uint64_t lines = jump_line_count(a.num);
    hipLaunchKernelGGL((jump_lines_kernel<G>), dim3(grid_blocks((lines * JUMP_LINE_DW + 255) / 256, 1u << 20)), dim3(256), 0,
                       a.st, a.jump_isa, a.jump_text, a.num, a.jump_words, lines, a.jump_lines);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

/* Trace: the traced task kernels; dispatch() sends it to trace_one (below), not through dispatch_one */
enum class Op { Task, Coop, Count, Locate, Ftab, RemTab, CountLines, Derive, PermCheck, Skip0, JumpText, JumpLines, Trace };

/* Defined here, instantiated once per (K, NB, LAY) in kfmi_inst_*.hip. */
template <int K, int NB, int LAY>
hipError_t dispatch_one(Op op, const SearchLaunch& a, unsigned long long* d_total)
{
  using G = Geo<K, NB, LAY>;
  switch (op) {
    case Op::Task: return launch_task<G>(a);
    case Op::Coop: return launch_coop<G>(a);
    case Op::Locate: return launch_locate<G>(a);
    case Op::Ftab: return launch_ftab<G>(a);
    case Op::RemTab: return launch_rem_tab<G>(a);
    case Op::CountLines: return launch_count_lines<G>(a, d_total);
    case Op::Derive: return launch_derive<G>(a);
    case Op::PermCheck: return launch_perm<G>(a);
    case Op::Skip0: return launch_skip0<G>(a);
    case Op::JumpText: return launch_jump_text<G>(a);
    case Op::JumpLines: return launch_jump_lines<G>(a);
    case Op::Trace: return hipErrorInvalidValue;   /* trace_one */
    default: return launch_count<G>(a, d_total);
  }
}

#define KFMI_INSTANTIATE(KK, NBV, LAYV) \
  template hipError_t dispatch_one<KK, NBV, LAYV>(Op, const SearchLaunch&, unsigned long long*);
#define KFMI_EXTERN(KK, NBV, LAYV) \
  extern template hipError_t dispatch_one<KK, NBV, LAYV>(Op, const SearchLaunch&, unsigned long long*);

/* The seed kernels' launch, apart from dispatch_one so that the units above
 * stay as they are: instantiated per (K, NB, LAY) in kfmi_inst_seeds_*.hip for
 * K <= 2 on the task and task-mid layouts, called from kfmi_seeds.hip. */
template <int K, int NB, int LAY>
hipError_t seeds_one(const SearchLaunch& a)
{
  return launch_seeds<Geo<K, NB, LAY>>(a);
}

#define KFMI_SEEDS_INSTANTIATE(KK, NBV, LAYV) template hipError_t seeds_one<KK, NBV, LAYV>(const SearchLaunch&);
#define KFMI_SEEDS_EXTERN(KK, NBV, LAYV) extern template hipError_t seeds_one<KK, NBV, LAYV>(const SearchLaunch&);

/* The traced task kernels' launch (Op::Trace), apart from dispatch_one like the
 * seed kernels' and for the same reason: launch_task with the traced kernels,
 * instantiated per (K, NB, LAY) in kfmi_inst_trace_*.hip for K <= 2 on the task
 * and task-mid layouts, called from dispatch (kfmi_search.hip). */
template <int K, int NB, int LAY>
hipError_t trace_one(const SearchLaunch& a)
{
  if (!a.trace || !a.maxw || a.strands) return hipErrorInvalidValue;
  return launch_task<Geo<K, NB, LAY>, Trace>(a);
}

#define KFMI_TRACE_INSTANTIATE(KK, NBV, LAYV) template hipError_t trace_one<KK, NBV, LAYV>(const SearchLaunch&);
#define KFMI_TRACE_EXTERN(KK, NBV, LAYV) extern template hipError_t trace_one<KK, NBV, LAYV>(const SearchLaunch&);

/* The traced strand and seed kernels' launches (kfmi_search_strands_trace,
 * kfmi_search_seeds_trace): launch_task / launch_seeds with the traced kernels,
 * instantiated per (K, NB, LAY) in kfmi_inst_trace_seeds_*.hip for K <= 2 on the
 * task and task-mid layouts, called from kfmi_strands.hip and kfmi_seeds.hip. */
template <int K, int NB, int LAY>
hipError_t strands_trace_one(const SearchLaunch& a)
{
  if (!a.trace || (a.maxw ? !a.strands : !(a.ix.skip && a.words_maxw))) return hipErrorInvalidValue;
  return launch_task<Geo<K, NB, LAY>, StrandTrace>(a);
}

template <int K, int NB, int LAY>
hipError_t seeds_trace_one(const SearchLaunch& a)
{
  if (!a.trace) return hipErrorInvalidValue;
  return launch_seeds<Geo<K, NB, LAY>, Trace>(a);
}

#define KFMI_SEEDS_TRACE_INSTANTIATE(KK, NBV, LAYV)                             \
  template hipError_t strands_trace_one<KK, NBV, LAYV>(const SearchLaunch&); \
  template hipError_t seeds_trace_one<KK, NBV, LAYV>(const SearchLaunch&);
#define KFMI_SEEDS_TRACE_EXTERN(KK, NBV, LAYV)                                         \
  extern template hipError_t strands_trace_one<KK, NBV, LAYV>(const SearchLaunch&); \
  extern template hipError_t seeds_trace_one<KK, NBV, LAYV>(const SearchLaunch&);

}  // namespace kfmi

#endif  // KFMI_KERNELS_H_
