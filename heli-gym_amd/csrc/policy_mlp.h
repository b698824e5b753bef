// policy_mlp.h — the handle's MLP policy, evaluated by one wave for its 64 envs (included by
// heligym_amd.hip after its Philox / u01 device functions).
//
// Model (include/heligym_amd.h, hg_set_policy):
//   x = (obs - obs_mean) * obs_scale                                  [17]
//   a = W3 tanh(W2 tanh(W1 x + b1) + b2) + b3 + exp(log_std) * z       [4]
// W1 [64,17], W2 [64,64], W3 [4,64] row-major [out,in], fp32.  The three products run on the exact
// fp32 matrix instruction v_mfma_f32_32x32x2_f32 (D = A B + C, an fp32 fma chain over k, one rounding
// per product) with the envs as the N dimension: H^T [64 hidden x 64 envs] = W X^T, four 32x32 tiles
// (mt = hidden half, nt = env half).  Operand maps of the instruction (lane l, h = l >> 5):
//   A[i = l & 31][k = h]      B[k = h][j = l & 31]      one k pair {k0, k1} per instruction
//   C/D: column j = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h        (reg = 0 .. 15)
// Layer 1: k pair ks = {2 ks, 2 ks + 1} of the 17 inputs and, as input 17, the constant 1 whose
// weight column is b1.  A lane holds its own env's x; v_permlane32_swap of (x[2 ks], x[2 ks + 1]) gives
// both env halves' B operands at once.
// Layers 2 and 3: the k order is chosen so that the previous layer's accumulator registers are the B
// operands as they stand: register r of hidden tile mt holds rows 32 mt + (r & 3) + 8 (r >> 2) (+ 4 in
// the upper half-wave) of H^T for this lane's column, which is B[k = h][j] of the k pair
// {that row, that row + 4}.  The weights are packed to match (policy_pack_kernel), so no lane moves
// and no LDS; a last k pair {1, 0} carries the bias.  Layer 3's A operand holds W3's four rows twice
// (tile rows 0-3 and 4-7, the rest zero), so both half-waves find their env's action in registers 0-3:
// lanes 0-31 in env tile 0's, lanes 32-63 in env tile 1's.
//
// Packed device image (floats; kPolicyFloats in all), written by policy_pack_kernel:
//   [0..3] exp(log_std) (0 when deterministic)   [4] 1.0 when stochastic, else 0.0
//   [5] log_std[0] + log_std[1] + log_std[2] + log_std[3], summed left to right (0 when deterministic)
//   [8..24] obs_mean (0 when absent)   [25..41] obs_scale (1 when absent)
//   [64 + 64 s + l]  A operand of lane l for slot s: s in [0,18) layer 1 (mt * 9 + ks),
//                    [18,84) layer 2 (mt * 33 + kp), [84,117) layer 3 (kp)
//
// Value head (hg_set_value_head, policy_eval): v = w_v . tanh(h2) + b_v shares the trunk and rides in
// layer 3's tile: w_v is one more row of the A operand, at tile rows 8 and 12, which acc_row() puts in
// accumulator register 4 of the lower and of the upper half-wave -- no further matrix instruction.  The
// rows of D are independent, so the actions are bitwise the same with or without it.  Its elements of
// the image (lanes 8, 12, 40, 44 of the layer-3 slots) are value_pack_kernel's and no one else's:
// policy_pack_kernel skips them, so hg_set_policy and hg_set_value_head commute and neither undoes the
// other.  They are zero (hg_create) until a head is set.
#pragma once

namespace hgp {

constexpr int kL1Steps = 9;                 // k pairs of layer 1 (17 inputs + the bias input)
constexpr int kL2Steps = 33;                // k pairs of layers 2 and 3 (64 hidden + the bias pair)
constexpr int kL1Slots = 2 * kL1Steps;      // x 2 hidden tiles
constexpr int kL2Slots = 2 * kL2Steps;
constexpr int kL3Slots = kL2Steps;
constexpr int kSlots = kL1Slots + kL2Slots + kL3Slots;
constexpr int kHeadFloats = 64;
constexpr int kStdOff = 0, kStochOff = 4, kMeanOff = 8, kScaleOff = 25;
constexpr int kLogStdSumOff = 5;            // sum of log_std (the log-probability's constant)
constexpr int kValueRowLo = 8, kValueRowHi = 12;   // the value head's rows of layer 3's tile
constexpr int kValueReg = 4;                // acc_row(0, 4, 0) == 8, acc_row(0, 4, 1) == 12
constexpr int kPolicyFloats = kHeadFloats + 64 * kSlots;
// key words of the action noise: the turbulence key (seed lo, seed hi) with these constants XORed in
constexpr uint32_t kNoiseKey0 = 0x706F6C69u, kNoiseKey1 = 0x63795F7Au;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the hidden row a lane of half-wave h holds in accumulator register r of hidden tile mt
__host__ __device__ constexpr int acc_row(int mt, int r, int h) { return 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h; }

// the A operands of one lane, kept in registers across the steps of a rollout
struct Weights {
    float l1[kL1Slots], l2[kL2Slots], l3[kL3Slots];
};

__device__ __forceinline__ void load_weights(const float* __restrict__ pk, int lane, Weights& w) {
    const float* p = pk + kHeadFloats + lane;
#pragma unroll
    for (int s = 0; s < kL1Slots; ++s) w.l1[s] = p[64 * s];
#pragma unroll
    for (int s = 0; s < kL2Slots; ++s) w.l2[s] = p[64 * (kL1Slots + s)];
#pragma unroll
    for (int s = 0; s < kL3Slots; ++s) w.l3[s] = p[64 * (kL1Slots + kL2Slots + s)];
}

// tanh(x) = sign(x) (1 - t) / (1 + t), t = exp(-2 |x|) = exp2(|x| * (-2 log2 e)) on the hardware exp2.
// One formula for every x: t underflows to 0 for large |x| (-> +-1), 1 - t is exact for t >= 1/2, and a
// NaN stays a NaN.
__device__ __forceinline__ float tanh_exp(float x) {
    const float t = __builtin_amdgcn_exp2f(fabsf(x) * -2.88539008177792681f);
    const float num = 1.0f - t;
    const float den = 1.0f + t;
    const float q = num / den;
    return copysignf(q, x);
}

// The action of this lane's env from its observation row.  Every lane of the wave must call it (the
// matrix instructions take all 64 columns); the lanes of a ragged tile's padding pass finite rows.
// gid = env_offset + env index; step, epi: the env's raw counters (as draw_eta keys the turbulence).
__device__ __forceinline__ float4 policy_action(const Weights& w, const float* __restrict__ pk, const float obs[17],
                                                int lane, uint64_t seed, uint64_t gid, int32_t step, int32_t epi) {
    const bool upper = lane >= 32;
    float x[18];
#pragma unroll
    for (int c = 0; c < 17; ++c) {
        const float d = obs[c] - pk[kMeanOff + c];
        x[c] = d * pk[kScaleOff + c];
    }
    x[17] = 1.0f;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // layer 1: h1[mt][nt]
    f32x16 h1[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
    for (int ks = 0; ks < kL1Steps; ++ks) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[2 * ks]), __float_as_uint(x[2 * ks + 1]),
                                                         false, false);
        const float b0 = __uint_as_float(sw[0]), b1 = __uint_as_float(sw[1]);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            h1[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l1[mt * kL1Steps + ks], b0, h1[mt][0], 0, 0, 0);
            h1[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l1[mt * kL1Steps + ks], b1, h1[mt][1], 0, 0, 0);
        }
    }
    // (each hidden value's tanh is taken where it becomes an operand, between the matrix instructions:
    // they run in the matrix pipe while the vector pipe computes the next operand)
    const float one_lo = upper ? 0.0f : 1.0f;   // the bias pair's B operand: k0 = 1, k1 = 0
    // layer 2: h2[mt2][nt], its k pairs the registers of h1
    f32x16 h2[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
    for (int kp = 0; kp < kL2Steps; ++kp) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float b = kp < 32 ? tanh_exp(h1[kp >> 4][nt][kp & 15]) : one_lo;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                h2[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l2[mt * kL2Steps + kp], b, h2[mt][nt], 0, 0, 0);
        }
    }
    // layer 3: o[nt], rows 0-3 (lower half-wave) and 4-7 (upper) both W3's four
    f32x16 o[2] = {zero, zero};
#pragma unroll
    for (int kp = 0; kp < kL2Steps; ++kp) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float b = kp < 32 ? tanh_exp(h2[kp >> 4][nt][kp & 15]) : one_lo;
            o[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l3[kp], b, o[nt], 0, 0, 0);
        }
    }
    float4 a;
    a.x = upper ? o[1][0] : o[0][0];
    a.y = upper ? o[1][1] : o[0][1];
    a.z = upper ? o[1][2] : o[0][2];
    a.w = upper ? o[1][3] : o[0][3];
    if (pk[kStochOff] != 0.0f) {   // (uniform) stochastic: four normals of one Philox call, Box-Muller as draw_eta's
        const U4 r = philox(U4{(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)step, (uint32_t)epi},
                            (uint32_t)seed ^ kNoiseKey0, (uint32_t)(seed >> 32) ^ kNoiseKey1);
        const float r0 = sqrtf(__log2f(u01(r.x)) * -1.38629436111989061f);   // sqrt(-2 ln u)
        const float r1 = sqrtf(__log2f(u01(r.z)) * -1.38629436111989061f);
        const float a1 = __uint_as_float((r.y >> 9) | 0x3f800000u), a3 = __uint_as_float((r.w >> 9) | 0x3f800000u);
        const float z0 = r0 * __builtin_amdgcn_cosf(a1);
        const float z1 = r0 * __builtin_amdgcn_sinf(a1);
        const float z2 = r1 * __builtin_amdgcn_cosf(a3);
        const float z3 = r1 * __builtin_amdgcn_sinf(a3);
        a.x = a.x + pk[kStdOff + 0] * z0;
        a.y = a.y + pk[kStdOff + 1] * z1;
        a.z = a.z + pk[kStdOff + 2] * z2;
        a.w = a.w + pk[kStdOff + 3] * z3;
    }
    return a;
}

// What policy_eval returns beside the action.
struct Eval {
    float4 a;     // the sampled action (the mean when nothing is drawn)
    float logp;   // log pi(a | obs) from the z drawn; 0 when nothing is drawn
    float v;      // w_v . tanh(h2) + b_v (0 while no value head is set)
};

// policy_action with the log-probability of the action and the value head's output.  The action is
// bitwise policy_action's (the same instructions on the same operands; the value row is another row of
// layer 3's D).  sample (wave-uniform): false computes the mean action and the value only and draws
// nothing -- the rollout's value of a terminal observation.  logp = -1/2 sum z_i^2 - sum log_std_i -
// 2 ln 2 pi with the z the noise was built from, not (a - mean) / std.
__device__ __forceinline__ Eval policy_eval(const Weights& w, const float* __restrict__ pk, const float obs[17], int lane,
                                            uint64_t seed, uint64_t gid, int32_t step, int32_t epi, bool sample) {
    const bool upper = lane >= 32;
    float x[18];
#pragma unroll
    for (int c = 0; c < 17; ++c) {
        const float d = obs[c] - pk[kMeanOff + c];
        x[c] = d * pk[kScaleOff + c];
    }
    x[17] = 1.0f;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 h1[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
    for (int ks = 0; ks < kL1Steps; ++ks) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[2 * ks]), __float_as_uint(x[2 * ks + 1]),
                                                         false, false);
        const float b0 = __uint_as_float(sw[0]), b1 = __uint_as_float(sw[1]);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            h1[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l1[mt * kL1Steps + ks], b0, h1[mt][0], 0, 0, 0);
            h1[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l1[mt * kL1Steps + ks], b1, h1[mt][1], 0, 0, 0);
        }
    }
    const float one_lo = upper ? 0.0f : 1.0f;
    f32x16 h2[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
    for (int kp = 0; kp < kL2Steps; ++kp) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float b = kp < 32 ? tanh_exp(h1[kp >> 4][nt][kp & 15]) : one_lo;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                h2[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l2[mt * kL2Steps + kp], b, h2[mt][nt], 0, 0, 0);
        }
    }
    f32x16 o[2] = {zero, zero};
#pragma unroll
    for (int kp = 0; kp < kL2Steps; ++kp) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float b = kp < 32 ? tanh_exp(h2[kp >> 4][nt][kp & 15]) : one_lo;
            o[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.l3[kp], b, o[nt], 0, 0, 0);
        }
    }
    Eval e;
    e.a.x = upper ? o[1][0] : o[0][0];
    e.a.y = upper ? o[1][1] : o[0][1];
    e.a.z = upper ? o[1][2] : o[0][2];
    e.a.w = upper ? o[1][3] : o[0][3];
    e.v = upper ? o[1][kValueReg] : o[0][kValueReg];
    e.logp = 0.0f;
    if (sample && pk[kStochOff] != 0.0f) {   // (uniform) the noise exactly as policy_action draws and adds it
        const U4 r = philox(U4{(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)step, (uint32_t)epi},
                            (uint32_t)seed ^ kNoiseKey0, (uint32_t)(seed >> 32) ^ kNoiseKey1);
        const float r0 = sqrtf(__log2f(u01(r.x)) * -1.38629436111989061f);   // sqrt(-2 ln u)
        const float r1 = sqrtf(__log2f(u01(r.z)) * -1.38629436111989061f);
        const float a1 = __uint_as_float((r.y >> 9) | 0x3f800000u), a3 = __uint_as_float((r.w >> 9) | 0x3f800000u);
        const float z0 = r0 * __builtin_amdgcn_cosf(a1);
        const float z1 = r0 * __builtin_amdgcn_sinf(a1);
        const float z2 = r1 * __builtin_amdgcn_cosf(a3);
        const float z3 = r1 * __builtin_amdgcn_sinf(a3);
        e.a.x = e.a.x + pk[kStdOff + 0] * z0;
        e.a.y = e.a.y + pk[kStdOff + 1] * z1;
        e.a.z = e.a.z + pk[kStdOff + 2] * z2;
        e.a.w = e.a.w + pk[kStdOff + 3] * z3;
        const float q = fmaf(z3, z3, fmaf(z2, z2, fmaf(z1, z1, z0 * z0)));
        e.logp = fmaf(-0.5f, q, -pk[kLogStdSumOff]) - 3.67575413281869070f;   // 2 ln 2 pi
    }
    return e;
}

// The applied-action bounds of hg_policy_act_mean / hg_rollout_branch_policy, by value in the kernel
// arguments (clamp == 0: no bounds).
struct ActBox {
    float lo[4], hi[4];
    int32_t clamp;
};

// The action of a policy-guided branch: the policy's mean `mu` (policy_eval(..., sample = false).a) plus the
// row's residual `res` -- one fp32 add per component, none at all without a residual (has_res,
// wave-uniform) -- clamped as hg_mppi_sample clamps its candidates.  hg_policy_act_mean's kernel and the
// branch kernel both call it.
__device__ __forceinline__ float4 residual_action(float4 mu, float4 res, bool has_res, const ActBox& box) {
    float v[4] = {mu.x, mu.y, mu.z, mu.w};
    if (has_res) {
        v[0] = v[0] + res.x;
        v[1] = v[1] + res.y;
        v[2] = v[2] + res.z;
        v[3] = v[3] + res.w;
    }
    if (box.clamp) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fminf(fmaxf(v[c], box.lo[c]), box.hi[c]);
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace hgp
