// group_kernel.h -- part of the single translation unit msx.hip (included there, after logprob_kernel.h).
// TARGET GROUPS (msx_group_*): one launch evaluates the walkers of several staged problems, one workgroup per walker,
// each against its own member's problem -- the fused kernel's body (logprob_body) once more, behind a member lookup.
#ifndef MSX_GROUP_KERNEL_H
#define MSX_GROUP_KERNEL_H

namespace {

// What the fused launch of one member passes as its leading (preloaded) arguments, kept per member in the group's
// device array beside the member's DevProblem.  The mode is the launch's: ng_fast holds ng | fast << 16 | dist_fit << 18 |
// use_av << 19 and the kernel adds mode << 8 (logprob_kernel's packed word, without the sampler / probe / linked bits).
struct GroupMember {
    const unsigned char *rblk;
    int32_t niso_nt, ng_fast;
    double tmin, tmax;
};

// The walkers' partition, by value in the kernel arguments (a launch's counts change; nothing is uploaded): member m
// owns walkers [start[m], start[m + 1]); start[k] = the launch's walker count.  Empty members repeat a start.
struct GroupStarts {
    int32_t k;
    int32_t start[MSX_MAX_GROUP + 1];
};

// The group's arrays are read through the CONSTANT address space: the member index is wave-uniform (blockIdx and kernel
// arguments only), so every field load is a scalar load, as the by-value struct's are in logprob_kernel.  (Through a
// generic pointer the compiler could not prove that the kernel's own stores -- through pointers it loads from the very
// same structs -- leave them alone, and would fetch them with vector loads.)
typedef __attribute__((address_space(4))) const DevProblem ConstDevProblem;
typedef __attribute__((address_space(4))) const GroupMember ConstGroupMember;

// The member of walker wk: the last m with start[m] <= wk -- a binary search over the kernel arguments, in scalar
// registers (readfirstlane: the compiler is told, not left to prove, that the index is the same in every lane)
__device__ __forceinline__ int group_member_of(const GroupStarts &st, int32_t wk) {
    int lo = 0, hi = st.k;  // start[lo] <= wk < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (st.start[mid] <= wk) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// One workgroup per walker of the whole group, the fused kernel's launch shape and launch bounds, and its body
// (logprob_body.h) over the walker's member.  No probe, GM, linked or in-path bits: the group's snapshots have those
// fields cleared (msx_group_create) and the packed word carries none of them.  (The names the body declares are its own:
// what this kernel adds is prefixed g_.)
// SMP = a half-step of the group's device-resident sampler (msx_group_sampler_*): the packed word gets the sampler bit,
// `theta` is the group's resident ensemble and g_smp_rec the half-step's records, whose si / ci are GROUP-level ensemble
// indices (member offset + local index); g_probs is the set of member snapshots built for this (slot, step, half) at
// msx_group_sampler_begin, whose sampler fields point at the group's arrays.  The plain instances (SMP = false) ignore
// g_smp_rec: their body is compiled with the sampler path off, as before.
template <int NS, int MAXT, bool SH = false, bool PF = false, int FULL = 0, bool SMP = false>
__global__ void __launch_bounds__(MAXT, MAXT == 256 ? (SH ? 2 : 3) : (MAXT == 512 && SH) ? 4 : 1)
logprob_group_kernel(const double *theta, ConstGroupMember *__restrict__ g_members, ConstDevProblem *__restrict__ g_probs,
                     int g_mode, int64_t n, GroupStarts g_st, double *__restrict__ logp, int32_t *__restrict__ status,
                     const SmpRec *__restrict__ g_smp_rec) {
    constexpr bool GM = false, LK = false, R32 = false, GIVEN = false;
    const int g_m = group_member_of(g_st, (int32_t)blockIdx.x);
    ConstGroupMember *const g_rec = g_members + g_m;
    // what logprob_kernel receives as its leading arguments, from the member's launch record
    const unsigned char *const rblk = g_rec->rblk;
    // (the sampler's instances: ng, fast, dist_fit and use_av of the record only -- no overlap or probe bits, whose paths the
    // compiler then drops -- and the sampler bit)
    const int niso_nt = g_rec->niso_nt;
    const int ng_mode_fast = SMP ? (g_rec->ng_fast & 0xd00ff) | (g_mode << 8) | (1 << 17) : g_rec->ng_fast | (g_mode << 8);
    const double gate_tmin = g_rec->tmin, gate_tmax = g_rec->tmax;
    const SmpRec *const smp_rec = SMP ? g_smp_rec : nullptr;
    const DevProblem &P = *(const DevProblem *)(g_probs + g_m);
#include "logprob_body.h"
}

}  // namespace

#endif  // MSX_GROUP_KERNEL_H
