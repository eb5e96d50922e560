// lg_lane_ints.h -- the INTEGER constants of a lane of the component-per-lane kernels (lg_quad.h): which env, leg and component it works
// on, its foot link and foot slot, and the byte offsets of its element in each index pattern of the state arrays.  Plain C, no HIP: the
// kernel includes it (through lg_shared.h), the host packs the per-leg foot constants with it, and tests/test_lane_constants.py compiles it
// on its own and compares every value with a derivation from the model description.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LG_LANE_FN __host__ __device__ static inline
#else
#define LG_LANE_FN static inline
#endif

// The foot link of each leg and its foot slot (the rank of that link among the foot links: the order of the (N, feet, ...) arrays), one byte
// per leg: bits 0-5 the link (LG_MAX_LINKS = 24), bits 6-7 the slot.  Packed by the host once per launch plan (KParams.k.foot_pack); a lane
// extracts its leg's byte with a shift and two masks instead of a select tree over the four links and four compares (go2's foot links
// do NOT ascend with the leg: 8, 4, 16, 12).
LG_LANE_FN uint32_t lg_foot_pack(const int32_t *foot_link, int legs) {
    uint32_t pack = 0;
    for (int l = 0; l < legs; l++) {
        uint32_t slot = 0;
        for (int k = 0; k < legs; k++) slot += foot_link[k] < foot_link[l] ? 1u : 0u;
        pack |= (((uint32_t)foot_link[l] & 63u) | (slot << 6)) << (8 * l);
    }
    return pack;
}

typedef struct LgLaneInts {
    int32_t c, cj, cjj;          // lane of the quad; its vector component (lane 3 shadows lane 2); its joint (four-joint legs: lane 3 has its own)
    int32_t leg, e, alive;       // leg of the env, env (dead lanes shadow the last env), whether the lane's own env exists
    int32_t ei;                  // 4 leg + c: the lane's type (lane-table row, episode-sum rows ei, ei + 16 | ei + 8 k)
    int32_t foot_link, foot_slot;
    int32_t ja;                  // this lane's joint in the (N, A) arrays
    // byte offsets: (N, A) f32 | (N) f32 | (N, 3) f32 | (N, 4) f32 | (N, feet) f32 | (N, feet, 3) f32 | (A) f32 | row ei of a (term, N) f32 array
    uint32_t o_ja, o_e, o_e3, o_q4, o_fs, o_ft, o_dj, o_es;
} LgLaneInts;

// tid: global lane index (workgroup * 64 + lane of the wave); legs / jpl: legs of the robot, joints per leg (compile-time in the kernel)
LG_LANE_FN LgLaneInts lg_lane_ints(int32_t tid, int32_t n_envs, int32_t legs, int32_t jpl, uint32_t foot_pack) {
    LgLaneInts r;
    r.c = tid & 3; r.cj = r.c < 2 ? r.c : 2; r.cjj = jpl == 4 ? r.c : r.cj;
    const int32_t quad = tid >> 2;
    r.leg = quad % legs; r.e = quad / legs;
    r.alive = r.e < n_envs ? 1 : 0;
    if (!r.alive) r.e = n_envs - 1;
    r.ei = (r.leg << 2) | r.c;
    const uint32_t fb = foot_pack >> (8 * r.leg);
    r.foot_link = (int32_t)(fb & 63u); r.foot_slot = (int32_t)((fb >> 6) & 3u);
    const int32_t d0 = jpl * r.leg;
    r.ja = r.e * (jpl * legs) + d0 + r.cjj;
    r.o_ja = 4u * (uint32_t)r.ja; r.o_e = 4u * (uint32_t)r.e; r.o_e3 = 4u * (uint32_t)(3 * r.e + r.cj); r.o_q4 = 4u * (uint32_t)(4 * r.e + r.c);
    r.o_fs = 4u * (uint32_t)(r.e * legs + r.foot_slot); r.o_ft = 3u * r.o_fs + 4u * (uint32_t)r.cj; r.o_dj = 4u * (uint32_t)(d0 + r.cj);
    r.o_es = 4u * ((uint32_t)r.ei * (uint32_t)n_envs + (uint32_t)r.e);
    return r;
}
