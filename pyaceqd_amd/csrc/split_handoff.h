// split_handoff.h — the hand-off of the split-group kernels, once: the device code by which the workgroups of one group
// pass a step's rows to each other in pt_split.hip (one trajectory per group) and pt_msplit.hip (several). Only these
// two files include it. Every function is inlined into its caller; the callers keep their exchange layouts, their
// gathers, their stamps and the epilogue of a failed wait (they differ: see poll_group).
// Four pieces have one caller and a written-out twin in the other kernel, because the call moved that kernel's
// registers or spills: st_keep, poll_group and sched_chunk / sched_pick are written out in
// pt_split.hip, xcd_slot in pt_msplit.hip. A change to one of them goes to its twin as well.
//
// Protocol (MI355X_MICROARCH.md § visibility, "Valid forms" table row 1), per step n and workgroup g of a group:
//   publish   the workgroup's rows of the step go to the exchange slot of parity n & 1: 8-B sc1 relaxed atomic stores
//             (st_sc1), or plain 16-B stores that keep their lines in the XCD's L2 (st_keep, "l2keep" below)
//   arrive    every storing wave drains (s_waitcnt vmcnt(0)), a workgroup barrier, then ONE lane stores the workgroup's
//             arrival word ct[g] = n + 1 (arrive_word): one word per producer, two 128-B lines per group, so no
//             serialised atomics at the L2 and one load per poll
//   poll      wave 0 reads all G words with one relaxed sc1 load per poll, lane l the word of workgroup l (poll_group);
//             the other waves wait at a barrier. No fences: every payload load that follows is an sc1 load too (16-B
//             buffer loads, unpack_c128)
// The slots are double-buffered by step parity: a workgroup cannot publish step n + 2 before every peer has gathered
// step n, because its own step n + 1 rows depend on that gather.
// Residency: one workgroup per CU (each kernel's LDS request forces it) and at most n_cu workgroups (host check), so
// every workgroup of a launch is resident. Every spin is bounded by spin_limit polls (PQD_SPLIT_SPIN); a wait that runs
// out ends the kernel with an error word and the host re-runs the step range another way.
// XCD-grouped grid (xcd_slot): block b sits in XCD slot b % 8 under the observed round-robin dealing, and slot xs holds
// the groups xs, xs + 8, ..., so all G workgroups of a group share one L2 when the dealing holds. Placement is speed
// only: the exchange is the same at any placement, unless
// l2keep: on that grid the payload and, from step 1 on, the arrival words are plain stores whose lines stay in the
// group's L2, where the peers' sc1 loads find them without a fabric round trip (an sc1 store drops the line, and the
// same-XCD readers then fetch it at the cross-XCD rate). That is coherent only if the whole group runs on one XCD: each
// arrival word carries its writer's XCD id in bits 28..30 (xcd_tag), step 0's word is still an sc1 store, and the first
// poll compares the ids (check_placement). A spread group ends the launch before its first gather. PQD_ABLATE bit 512
// fakes one (workgroup 0 reports the next XCD) for the tests of that path.
#pragma once
#include "pqd_common.h"

typedef unsigned long long __attribute__((address_space(1))) gu64;
typedef unsigned int __attribute__((address_space(1))) gu32;
typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));

constexpr unsigned HO_STEP_MASK = 0x0FFFFFFFu;  // arrival word: step n + 1 in bits 0..27, the writer's XCD id above
// s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 4): register id 20, offset 0, size 4 (simm16 = (size - 1) << 11 | offset << 6 | id)
constexpr int HO_HWREG_XCC_ID = (3 << 11) | (0 << 6) | 20;

__device__ __forceinline__ void st_sc1(double2* p, double2 v) {
    __hip_atomic_store((gu64*)&p->x, (unsigned long long)__double_as_longlong(v.x), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64*)&p->y, (unsigned long long)__double_as_longlong(v.y), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
// plain 16-B global store: the line stays in the XCD's L2. Used only under l2keep
__device__ __forceinline__ void st_keep(double2* p, double2 v) {
    typedef double v2f64 __attribute__((ext_vector_type(2)));
    v2f64 w = {v.x, v.y};
    *(__attribute__((address_space(1))) v2f64*)p = w;
}
// plain global load (a generic pointer would become flat_load, which also counts in lgkmcnt: every LDS wait would then
// wait for the register prefetches too)
__device__ __forceinline__ double2 gld(const double2* p) {
    const __attribute__((address_space(1))) double* q = (const __attribute__((address_space(1))) double*)p;
    return make_double2(q[0], q[1]);
}
// the complex number a 16-B buffer load returned
__device__ __forceinline__ double2 unpack_c128(v4u32 r) {
    return make_double2(__hiloint2double((int)r.y, (int)r.x), __hiloint2double((int)r.w, (int)r.z));
}

// XCD-grouped grid: the group of block b and the workgroup's index g in it, G workgroups per group
struct XcdSlot {
    int group, g;
};
__device__ __forceinline__ XcdSlot xcd_slot(unsigned b, int G) {
    const int xs = b & 7, loc = b >> 3;
    return {xs + 8 * (loc / G), loc - (loc / G) * G};
}

// this workgroup's XCD id where the arrival word carries it (or, faked: the next XCD's, from workgroup 0)
__device__ __forceinline__ unsigned xcd_tag(int g, int ablate) {
    unsigned xid = (unsigned)__builtin_amdgcn_s_getreg(HO_HWREG_XCC_ID) & 7u;
    if ((ablate & 512) && g == 0) xid = (xid + 1u) & 7u;
    return xid << 28;
}

// one lane, after the drain and the barrier: workgroup g has published step n (xtag: xcd_tag under l2keep, else 0)
__device__ __forceinline__ void arrive_word(unsigned* ct, int g, int n, unsigned xtag, bool l2keep) {
    const unsigned av = ((unsigned)n + 1u) | xtag;
    if (l2keep && n >= 1) *(__attribute__((address_space(1))) unsigned*)(ct + g) = av;
    else __hip_atomic_store((gu32*)(ct + g), av, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave 0 waits until all G workgroups have published step want - 1. Returns whether they did within spin_limit polls;
// placed (set only with check_placement, the first poll under l2keep; the caller starts it at true): their words carry
// one XCD id. The same words reach every workgroup of the group, so all of them take the same decision. The caller
// turns a failure into its own error words: pt_split.hip sets err[0] for either, pt_msplit.hip err[1] as well for a
// placement miss (its host re-runs with sc1). (The two results are a return value and a reference, not one struct: a
// struct moved pt_msplit's SGPR spills.)
template <int G>
__device__ __forceinline__ bool poll_group(const unsigned* ct, int lane, unsigned want, unsigned spin_limit,
                                           bool check_placement, bool& placed) {
    unsigned spins = 0;
    bool ok = true;
    for (;;) {
        const unsigned v =
            lane < G ? __hip_atomic_load((gu32*)(ct + lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
        if (__all((v & HO_STEP_MASK) >= want)) {
            if (check_placement) {
                const unsigned x0 = __builtin_amdgcn_readfirstlane(v) >> 28;
                placed = __all(lane >= G || (v >> 28) == x0);
            }
            break;
        }
        __builtin_amdgcn_s_sleep(1);
        if (++spins > spin_limit) { ok = false; break; }
    }
    return ok;
}

// the schedule, 64 entries at a time in a VGPR (lane i holds sched[64 c + i], -1 from n_end on), picked with v_readlane:
// a uniform sched[n] load in the step loop compiles to a vector load + readfirstlane that waits (s_waitcnt vmcnt(0))
// for every outstanding vector memory op where it is issued, on every workgroup's critical path each step. The callers
// load a chunk ahead and keep their own rotation
__device__ __forceinline__ int sched_chunk(const int* sched, int c, int lane, int n_end) {
    const int i = 64 * c + lane;
    return i < n_end ? *(const __attribute__((address_space(1))) int*)(sched + i) : -1;
}
__device__ __forceinline__ int sched_pick(int chunk, int m) { return __builtin_amdgcn_readlane(chunk, m & 63); }
