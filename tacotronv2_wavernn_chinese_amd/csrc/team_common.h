// The XCD-team protocol, in one place.  Six kernels run as teams of the 32 workgroups of one XCD -- loop_team2.hip, loop_batch.hip,
// loop_batch_cs.hip, loop_dm_team.hip, loop_teamg.hip and the two GRU kernels of train_team.hip -- and all of them form their teams,
// publish and take granules and reduce over lanes with the helpers below; none of them carries a copy.
//
//   * Team = the workgroups that RUN on one XCD (HW_REG_XCC_ID, never blockIdx), numbered in order of first arrival (join_team).
//   * Exchange = 8-byte {tag (hi), payload (lo)} granules through the XCD's L2: plain store, L1-bypassing load, the data is the flag;
//     regions are double-buffered by step parity and the tag is the step's epoch.  Same-XCD only.
//   * Every wait is bounded: a spin that gives up writes its code to the device error word and sets the caller's `dead`, with which
//     all waves run on to the kernel's next bail-out check instead of hanging.
#pragma once
#include "device_util.h"
#include "wrnn_internal.h"

#define TEAM_WGS 32
#define TEAM_SPIN_MAX 300000u
// polls a workgroup waits at the start of a team kernel for the other 31 of its XCD (~1.5 ms; a resident launch needs ~10 us)
#define WRNN_ARRIVE_POLLS 200000u
// Control words of a launch (zeroed by the host inside the launch gate, wrnn_gated_launch):
//   ctl[0..15]     arrivals per physical XCC id (the id is read as 4 bits)
//   ctl[8]         team slots handed out
//   ctl[16 + xcc]  slot + 1 of that XCC id, 0 = none yet
// ctl[8] is also the arrival counter of an XCC id 8.  This part numbers its XCDs 0..7 in every partition mode, so the two never
// meet; on a part that did report an id of 8 the counts would mix, the formation would come out short or overfull, and the launch
// would end in WRNN_ERR_BUSY or a bounded exchange timeout -- wrong, but not a hang.
#define TEAM_CTL_WORDS 32

typedef unsigned long long u64;

namespace {

// slots of a kernel's `misc` words in LDS: team, rank inside the team, bail-out flag
constexpr int M_TEAM = 0, M_RANK = 1, M_DEAD = 2;

__device__ __forceinline__ unsigned xcc_id() {
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 0xf;
}

// Team formation + co-residency check.  Teams are numbered in order of first arrival of their XCD, so any set of XCC ids (SPX, or a
// partition exposing a subset of the XCDs) maps onto team slots 0..n_teams-1.  Returns false when this workgroup is not in a team.
// Co-residency is checked instead of assumed: the 32 workgroups of an XCD spin on each other for the whole launch, so all of them must
// be running NOW.  One bounded wait for the team slot AND the arrival counter; if the counter does not fill -- the GPU is shared with
// another process's kernel -- report WRNN_ERR_BUSY and leave instead of timing out inside the loop.
// LEAVE_SPARE: a workgroup whose XCD holds a slot beyond n_teams is not in a team, and leaves as soon as it sees the slot: no arrival
// wait, no error word.  loop_dm_team.hip needs it (its grid covers every XCD and the first one works); the batch kernels take it
// too.  In a grid of n_teams * 32 workgroups such a slot only occurs in an uneven launch, and the team that is short reports that as
// WRNN_ERR_BUSY either way.  loop_team2.hip, loop_teamg.hip and train_team.hip leave it off, which keeps the code generated for
// them what it was before they shared this header (profiles/team_common.txt).
template <bool LEAVE_SPARE = false>
__device__ __forceinline__ bool join_team(unsigned *ctl, unsigned *err, int *misc_i, int n_teams, int &team, int &g) {
    if (threadIdx.x == 0) {
        const unsigned x = xcc_id();
        misc_i[M_DEAD] = 0;
        const unsigned rank = atomicAdd(&ctl[x], 1u);
        unsigned slot1 = 0, arrived = 0;
        if (rank == 0) {
            slot1 = atomicAdd(&ctl[8], 1u) + 1u;
            __hip_atomic_store(&ctl[16 + x], slot1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        bool spare = false;
        for (unsigned spins = 0; spins < WRNN_ARRIVE_POLLS; ++spins) {
            slot1 = __hip_atomic_load(&ctl[16 + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            arrived = __hip_atomic_load(&ctl[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            spare = LEAVE_SPARE && slot1 > (unsigned)n_teams;
            if (spare || (slot1 && arrived >= TEAM_WGS)) break;
        }
        if (spare) slot1 = 0;
        else if (arrived < TEAM_WGS) { slot1 = 0; if (rank < TEAM_WGS) atomicCAS(err, 0u, WRNN_DEVERR_BUSY); }
        misc_i[M_TEAM] = slot1 ? (int)slot1 - 1 : 1 << 20;   // no slot: "not in a team" below
        misc_i[M_RANK] = (int)rank;
    }
    __syncthreads();
    team = __builtin_amdgcn_readfirstlane(misc_i[M_TEAM]);
    g = __builtin_amdgcn_readfirstlane(misc_i[M_RANK]);
    __syncthreads();
    return g < TEAM_WGS && team < n_teams;
}

// publish one granule; float callers pass __float_as_uint
__device__ __forceinline__ void st_granule(u64 *base, unsigned idx, unsigned tag, unsigned payload) {
    const u64 v = ((u64)tag << 32) | payload;
    const unsigned off = idx * 8u;
    asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"(off), "v"(v), "s"(base) : "memory");
}
// st_granule for a kernel so short of scalar registers that `base` may come back from a spill: it is then restored with v_readlane
// right in front of the store, and a VALU write of an SGPR needs five wait states before a VMEM instruction reads it as its address.
// The compiler inserts them for its own instructions, not for inline assembly, so they are part of the statement here.
__device__ __forceinline__ void st_granule_ws(u64 *base, unsigned idx, unsigned tag, unsigned payload) {
    const u64 v = ((u64)tag << 32) | payload;
    const unsigned off = idx * 8u;
    asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %2" ::"v"(off), "v"(v), "s"(base) : "memory");
}
__device__ __forceinline__ u64 peek(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// One granule per lane, wave-uniform completion, two staggered first looks, then the bounded re-read loop (loop_dm_team.hip,
// loop_teamg.hip).  loop_team2.hip measured this form against a single look and keeps its own take_granule.
__device__ __forceinline__ float take_staggered(const u64 *base, unsigned idx, unsigned tag, bool &dead, unsigned *err, unsigned code) {
    u64 ga = peek(base + idx);
    __builtin_amdgcn_s_sleep(3);
    u64 gb = peek(base + idx);
    if (__all((unsigned)(ga >> 32) == tag)) return __uint_as_float((unsigned)ga);
    unsigned spins = 0;
    while (!dead && !__all((unsigned)(gb >> 32) == tag)) {
        if (++spins > TEAM_SPIN_MAX) { dead = true; if ((threadIdx.x & 63) == 0) atomicExch(err, code); break; }
        gb = peek(base + idx);
    }
    return __uint_as_float((unsigned)gb);
}

template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum(float v) {   // sum over the 16 lanes of a DPP row, result in every lane
    v += dppf<0xB1>(v);
    v += dppf<0x4E>(v);
    v += dppf<0x141>(v);
    v += dppf<0x140>(v);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {   // max over 64 lanes, valid in lane 63
    // One v_max_f32_dpp per step (the compiler's fmaxf + update_dpp form costs 4 VALU per step: copy, DPP move, two
    // canonicalising maxes).  s_nop 1 = the two wait states a DPP read of a just-written VGPR needs.
    asm volatile(
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}

__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f); }

}  // namespace

// The older two-loop form of the same formation, for loop_batch_cs.hip alone: a bounded wait for the slot, then a bounded, sleeping wait
// for the arrivals; it defines `team` and `g` and leaves the "in a team" test to the caller.  A MACRO, because that kernel sits at its
// register limit and its allocation follows the text of its prologue: with join_team a scratch reload enters the shadow waves' 8-row
// step loop and configs[2] loses 1.7 %, and the same two loops as an inlined function spill more still (profiles/team_common.txt).
// Expanded in place the kernel is generated as before.  Whoever finds a form of join_team that kernel tolerates can drop this.
#define JOIN_TEAM_TWO_LOOP(a, misc_i, tid, team, g)                                                                         \
    if ((tid) == 0) {                                                                                                       \
        const unsigned x = xcc_id();                                                                                        \
        (misc_i)[M_DEAD] = 0;                                                                                               \
        const unsigned rank = atomicAdd(&(a).ctl[x], 1u);                                                                   \
        unsigned slot1 = 0;                                                                                                 \
        if (rank == 0) {                                                                                                    \
            slot1 = atomicAdd(&(a).ctl[8], 1u) + 1u;                                                                        \
            __hip_atomic_store(&(a).ctl[16 + x], slot1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                        \
        } else {                                                                                                            \
            for (unsigned spins = 0; spins < 4000000u; ++spins) {                                                           \
                slot1 = __hip_atomic_load(&(a).ctl[16 + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                    \
                if (slot1) break;                                                                                           \
            }                                                                                                               \
        }                                                                                                                   \
        if (slot1 && rank < TEAM_WGS) {                                                                                     \
            unsigned arrived = 0;                                                                                           \
            for (unsigned spins = 0; spins < WRNN_ARRIVE_POLLS; ++spins) {                                                  \
                arrived = __hip_atomic_load(&(a).ctl[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                       \
                if (arrived >= TEAM_WGS) break;                                                                             \
                __builtin_amdgcn_s_sleep(8);                                                                                \
            }                                                                                                               \
            if (arrived < TEAM_WGS) { atomicCAS((a).err, 0u, WRNN_DEVERR_BUSY); slot1 = 0; }                                \
        }                                                                                                                   \
        (misc_i)[M_TEAM] = slot1 ? (int)slot1 - 1 : 1 << 20;                                                                \
        (misc_i)[M_RANK] = (int)rank;                                                                                       \
    }                                                                                                                       \
    __syncthreads();                                                                                                        \
    const int team = __builtin_amdgcn_readfirstlane((misc_i)[M_TEAM]);                                                      \
    const int g = __builtin_amdgcn_readfirstlane((misc_i)[M_RANK]);                                                         \
    __syncthreads()
