// ppo_grad.hip — the clipped PPO loss's gradient for the fixed 17-64-64-4 tanh actor with its value head
// (include/heligym_amd.h, hg_ppo_grad): forward, back-propagation and the 5641 parameter-gradient sums of
// a minibatch in one kernel, no per-sample intermediate leaving the CU, then a fixed-order reduction.
//
// Tiles.  One wave owns a tile of 64 samples at a time (grid-stride over the tiles by wave); a block is
// four waves, one per SIMD, sharing one LDS image of the weights.  Every product runs on
// v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain over k).  Operand maps (lane l, i = l & 31, h = l >> 5):
//   A[i][k = h]    B[k = h][j = i]    C/D: column j = i, row acc_row(reg, h) = (reg & 3) + 8 (reg >> 2) + 4 h
// Forward (policy_mlp.h's scheme): samples are the N dimension, H^T [64 hidden x 64 samples] = W X^T in
// four 32x32 tiles [mt = hidden half][nt = sample half]; a layer's accumulator registers are the next
// layer's B operands as they stand (k pair {row, row + 4}), the bias a last k pair {1, 0}.  Layer 3's A
// holds W3's rows at tile rows 0-3 and 4-7 and w_v at rows 8 and 12: lane l finds its own sample's mean
// in registers 0-3 and its value in register 4 of o[h].
// Backward through the layers keeps that layout: dH2 = [W3; w_v]^T d3 (k = 5 outputs, padded to 6; the
// per-sample d3 reaches both sample halves by v_permlane32_swap as layer 1's input does), D2 = dH2 (1 -
// H2^2), dH1 = W2^T D2 with D2's registers as B operands, D1 = dH1 (1 - H1^2).
// Weight gradients contract over the samples, the lane dimension of that layout, so each operand goes
// through a per-wave LDS transpose, 32 samples at a time: rows [hidden][36] (stride 36 = 4 mod 32: the
// stores of a half-wave hit 32 banks, the 16-byte loads of a 16-lane group 16 distinct 4-bank slots).
// A lane of half h reads samples 8 q + 4 h + {0 .. 3} of its row as one 16-byte load and uses them as
// the k values of four instructions: A and B agree on that k order, which is all a contraction needs.
//   dW2 [out][in]      = D2 (A) x H1 (B)            four accumulator tiles [mt][n2]
//   dW1 [out][18]      = D1 (A) x [x; 1] (B)         two tiles; column 17, the constant input, is db1
//   d[W3; w_v] [5][in] = d3 (A, rows 0-4) x H2 (B)   two tiles
// Rows / columns past an operand's extent read finite filler: a row of D depends on that row of A only.
// db2 is the lane sum of D2's A operands as they are read; db3, db_v, dlog_std and the statistics are
// per-lane sums.  All of it stays in registers across the wave's tiles.
// End of block: the four waves' sums are added in wave order through LDS and written as the block's
// partial to the workspace; ppo_reduce_kernel adds the partials in a fixed order.  No atomics: the launch
// shape is a function of M, so the bits are too.
// The weighted imitation loss (hg_bc_grad) is a second head on the same body: grad_body<LOSS> below holds
// everything, ppo_grad_kernel and bc_grad_kernel are its two instantiations.
#include "ppo_grad.h"

namespace hgk {
namespace {

constexpr int kWaves = 4, kThreads = 64 * kWaves;
// weight image slots, 64 floats (one per lane) each
constexpr int kS1 = 0;      // layer 1 forward   [mt * 9 + ks]
constexpr int kS2 = 18;     // layer 2 forward   [mt * 33 + kp]
constexpr int kS3 = 84;     // layer 3 forward   [kp]
constexpr int kSB3 = 117;   // [W3; w_v]^T       [mt * 3 + kk]
constexpr int kSB2 = 123;   // W2^T              [mt * 32 + kp]
constexpr int kSlots = 187;
constexpr int kTS = 36;     // transposed half tile: floats per hidden row (32 samples + 4)
constexpr int kXS = 68;     // x / d3 rows: floats per row (64 samples + 4)
constexpr int kRA = 0, kRB = 64 * kTS, kRX = 2 * 64 * kTS, kR3 = kRX + 18 * kXS, kWaveFloats = kR3 + 8 * kXS;
static_assert(kSlots * 64 >= kPpoPartialFloats, "the block sum reuses the weight image's LDS");
static_assert((kSlots * 64 + kWaves * kWaveFloats) * 4 <= 160 * 1024, "LDS of one CU");

typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

#define HG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// policy_mlp.h's tanh: sign(x) (1 - t) / (1 + t), t = exp2(|x| * (-2 log2 e))
__device__ __forceinline__ float tanh_exp(float x) {
    const float t = __builtin_amdgcn_exp2f(fabsf(x) * -2.88539008177792681f);
    const float num = 1.0f - t;
    const float den = 1.0f + t;
    const float q = num / den;
    return copysignf(q, x);
}

// the flat parameter index of element `lane` of weight image slot `slot`, or -1 where the image holds 0
__device__ __forceinline__ int image_index(int slot, int lane) {
    const int i = lane & 31, h = lane >> 5;
    if (slot < kS2) {
        const int mt = slot / 9, ks = slot % 9, row = 32 * mt + i, c = 2 * ks + h;
        return c < 17 ? kPpoW1 + row * 17 + c : kPpoB1 + row;
    }
    if (slot < kS3) {
        const int s = slot - kS2, mt = s / 33, kp = s % 33, o = 32 * mt + i;
        if (kp == 32) return h ? -1 : kPpoB2 + o;
        return kPpoW2 + o * 64 + 32 * (kp >> 4) + acc_row(kp & 15, h);
    }
    if (slot < kSB3) {
        const int kp = slot - kS3;
        const bool act = i < 8, val = i == 8 || i == 12;
        if (!act && !val) return -1;
        if (kp == 32) return h ? -1 : (act ? kPpoB3 + (i & 3) : kPpoBv);
        const int col = 32 * (kp >> 4) + acc_row(kp & 15, h);
        return act ? kPpoW3 + (i & 3) * 64 + col : kPpoWv + col;
    }
    if (slot < kSB2) {
        const int s = slot - kSB3, mt = s / 3, kk = s % 3, k = 2 * kk + h, hid = 32 * mt + i;
        return k < 4 ? kPpoW3 + k * 64 + hid : (k == 4 ? kPpoWv + hid : -1);
    }
    const int s = slot - kSB2, mt = s >> 5, kp = s & 31;
    return kPpoW2 + (32 * (kp >> 4) + acc_row(kp & 15, h)) * 64 + 32 * mt + i;
}

// A wave's LDS stores are visible to its later loads (the LDS serves a wave's requests in order); this
// keeps the compiler from moving either across the other.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sample half nt of a [64 hidden x 64 samples] register tile pair -> R[hidden][kTS]
__device__ __forceinline__ void put_half(float* __restrict__ R, const f32x16& t0, const f32x16& t1, int i, int h) {
    float* p = R + (4 * h) * kTS + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        p[acc_row(r, 0) * kTS] = t0[r];
        p[(32 + acc_row(r, 0)) * kTS] = t1[r];
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// The loss heads.  Everything but the head -- the forward pass, the back-propagation, the parameter sums and
// the block's partial -- is the same code for each; the head forms d3[0..4], the log_std sums and the six
// statistic sums of its loss from the sample's mean, value and labels.
//   kLossPpo: the clipped surrogate (hg_ppo_grad).
//   kLossBc:  the weighted imitation loss (hg_bc_grad); `mode` (HG_BC_NLL / HG_BC_MSE, wave-uniform) selects
//             between the two regressions inside the head.  The argument struct's adv slot carries the
//             weights (or nullptr: 1), ret the value targets (or nullptr: no value term), logp_old nothing.
constexpr int kLossPpo = 0, kLossBc = 1;
constexpr int kBcNll = 0, kBcMse = 1;   // include/heligym_amd.h's HG_BC_NLL, HG_BC_MSE

template <int LOSS>
__device__ __forceinline__ void grad_body(const PpoGradArgs& a, const int64_t tiles, const int mode) {
    __shared__ __attribute__((aligned(16))) float s_img[kSlots * 64];
    __shared__ __attribute__((aligned(16))) float s_wave[kWaves][kWaveFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const float* __restrict__ th = a.theta;
    // the weight image, twelve loads in flight per thread (the index arithmetic first, then the loads)
    constexpr int kImgBatch = 12;
    for (int e0 = tid; e0 < kSlots * 64; e0 += kThreads * kImgBatch) {
        int idx[kImgBatch];
        float v[kImgBatch];
#pragma unroll
        for (int u = 0; u < kImgBatch; ++u) {
            const int e = e0 + u * kThreads;
            idx[u] = e < kSlots * 64 ? image_index(e >> 6, e & 63) : -1;
        }
#pragma unroll
        for (int u = 0; u < kImgBatch; ++u) v[u] = th[idx[u] < 0 ? 0 : idx[u]];
#pragma unroll
        for (int u = 0; u < kImgBatch; ++u) {
            const int e = e0 + u * kThreads;
            if (e < kSlots * 64) s_img[e] = idx[u] < 0 ? 0.0f : v[u];
        }
    }
    float* const RA = s_wave[wave] + kRA;
    float* const RB = s_wave[wave] + kRB;
    float* const RX = s_wave[wave] + kRX;
    float* const R3 = s_wave[wave] + kR3;
    for (int e = lane; e < 8 * kXS; e += 64) R3[e] = 0.0f;
    __syncthreads();
    const float* const img = s_img + lane;

    float ls[4], inv_std[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ls[c] = th[kPpoLogStd + c];
        inv_std[c] = expf(-ls[c]);
    }
    const float ls_sum = ((ls[0] + ls[1]) + ls[2]) + ls[3];
    const float one_lo = h ? 0.0f : 1.0f;
    const float clip_lo = 1.0f - a.clip, clip_hi = 1.0f + a.clip;

    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 accW2[2][2] = {{zero, zero}, {zero, zero}};
    f32x16 accW1[2] = {zero, zero};
    f32x16 acc3[2] = {zero, zero};
    float sb2[2] = {0.f, 0.f};
    float sb3[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // db3[0..3], db_v
    float sls[4] = {0.f, 0.f, 0.f, 0.f};
    float st[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // policy term, value term, kl, clip fraction, ratio, skipped

    const int64_t stride = (int64_t)gridDim.x * kWaves;
#pragma unroll 1
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < tiles; tile += stride) {
        // ---- this lane's sample
        const int64_t t = tile * 64 + lane;
        const bool valid = t < a.M;
        int64_t row = valid ? t : 0;
        bool skipped = false;
        if (a.index) {
            const int32_t ix = valid ? a.index[t] : 0;
            skipped = valid && (ix < 0 || (int64_t)ix >= a.B);
            row = (valid && !skipped) ? (int64_t)ix : 0;
        }
        const bool active = valid && !skipped;
        float x[18];
        {
            const float* __restrict__ o = a.obs + row * 17;
#pragma unroll
            for (int c = 0; c < 17; ++c) {
                const float d = o[c] - (a.mean ? a.mean[c] : 0.0f);
                x[c] = d * (a.scale ? a.scale[c] : 1.0f);
            }
            x[17] = 1.0f;
        }
        const float4 av = *reinterpret_cast<const float4*>(a.act + row * 4);
        const float act[4] = {av.x, av.y, av.z, av.w};
        float lp_old = 0.0f, adv = 1.0f, ret = 0.0f;   // (kLossBc: adv is the weight, ret the value target)
        if constexpr (LOSS == kLossPpo) {
            lp_old = a.logp_old[row];
            adv = a.adv[row];
            ret = a.ret[row];
        } else {
            if (a.adv) adv = a.adv[row];
            if (a.ret) ret = a.ret[row];
        }
#pragma unroll
        for (int c = 0; c < 18; ++c) RX[c * kXS + lane] = x[c];

        // ---- forward
        f32x16 h1[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
        for (int ks = 0; ks < 9; ++ks) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[2 * ks]), __float_as_uint(x[2 * ks + 1]),
                                                             false, false);
            const float b0 = __uint_as_float(sw[0]), b1 = __uint_as_float(sw[1]);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float w = img[(kS1 + mt * 9 + ks) * 64];
                h1[mt][0] = HG_MFMA(w, b0, h1[mt][0]);
                h1[mt][1] = HG_MFMA(w, b1, h1[mt][1]);
            }
        }
        // (each hidden value's tanh is taken where it becomes an operand, between the matrix instructions,
        // and kept in place of the pre-activation: h1, h2 hold tanh values from here on)
        f32x16 h2[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
        for (int kp = 0; kp < 33; ++kp) {
            float b[2] = {one_lo, one_lo};
            if (kp < 32) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    b[nt] = tanh_exp(h1[kp >> 4][nt][kp & 15]);
                    h1[kp >> 4][nt][kp & 15] = b[nt];
                }
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float w = img[(kS2 + mt * 33 + kp) * 64];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) h2[mt][nt] = HG_MFMA(w, b[nt], h2[mt][nt]);
            }
        }
        f32x16 o3[2] = {zero, zero};
#pragma unroll
        for (int kp = 0; kp < 33; ++kp) {
            float b[2] = {one_lo, one_lo};
            if (kp < 32) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    b[nt] = tanh_exp(h2[kp >> 4][nt][kp & 15]);
                    h2[kp >> 4][nt][kp & 15] = b[nt];
                }
            }
            const float w = img[(kS3 + kp) * 64];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) o3[nt] = HG_MFMA(w, b[nt], o3[nt]);
        }

        // ---- the loss's derivative with respect to this sample's mean, value and log_std
        float d3[6];
        if constexpr (LOSS == kLossPpo) {
            float z[4], q = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float mu = h ? o3[1][c] : o3[0][c];
                const float diff = act[c] - mu;
                z[c] = diff * inv_std[c];
                q = fmaf(z[c], z[c], q);
            }
            const float v = h ? o3[1][4] : o3[0][4];
            const float logp = fmaf(-0.5f, q, -ls_sum) - 3.67575413281869070f;   // 2 ln 2 pi
            const float dl = logp - lp_old;
            const float ratio = expf(dl);
            const float rc = fminf(fmaxf(ratio, clip_lo), clip_hi);
            const float ra = ratio * adv, ca = rc * adv;
            const float pol = -fminf(ra, ca);
            const bool clipped_out = (adv > 0.0f && ratio > clip_hi) || (adv < 0.0f && ratio < clip_lo);
            const float nra = -ra;
            const float g = (active && !clipped_out) ? nra * a.inv_m : 0.0f;   // dL / dlogp
            const float verr = v - ret;
            const float vg = a.vf_coef * verr;
            const float gv = active ? vg * a.inv_m : 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float gz = g * z[c];
                d3[c] = gz * inv_std[c];
                sb3[c] = sb3[c] + d3[c];
                const float zz = fmaf(z[c], z[c], -1.0f);
                sls[c] = fmaf(g, zz, sls[c]);
            }
            d3[4] = gv;
            d3[5] = 0.0f;
            sb3[4] = sb3[4] + gv;
            const float hv = 0.5f * verr;
            st[0] = st[0] + (active ? pol : 0.0f);
            st[1] = st[1] + (active ? hv * verr : 0.0f);
            st[2] = st[2] + (active ? -dl : 0.0f);
            st[3] = st[3] + ((active && (ratio < clip_lo || ratio > clip_hi)) ? 1.0f : 0.0f);
            st[4] = st[4] + (active ? ratio : 0.0f);
            st[5] = st[5] + (skipped ? 1.0f : 0.0f);
        } else {
            // the imitation head: st = {w l, 1/2 (v - y)^2, sum (a* - mu)^2, w, logp(a*), skipped}
            const bool nll = mode == kBcNll;   // (uniform)
            float diff[4], z[4], q = 0.0f, sq = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float mu = h ? o3[1][c] : o3[0][c];
                diff[c] = act[c] - mu;
                z[c] = diff[c] * inv_std[c];
                q = fmaf(z[c], z[c], q);
                sq = fmaf(diff[c], diff[c], sq);
            }
            const float v = h ? o3[1][4] : o3[0][4];
            const float logp = fmaf(-0.5f, q, -ls_sum) - 3.67575413281869070f;   // 2 ln 2 pi
            const float w = adv;
            const float wm = active ? w * a.inv_m : 0.0f;
            const float g = -wm;   // NLL: dL / dlogp
            const float verr = a.ret ? v - ret : 0.0f;
            const float vg = a.vf_coef * verr;
            const float gv = active ? vg * a.inv_m : 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float gz = g * z[c];
                const float nd = -diff[c];
                d3[c] = nll ? gz * inv_std[c] : nd * wm;
                sb3[c] = sb3[c] + d3[c];
                const float zz = fmaf(z[c], z[c], -1.0f);
                sls[c] = nll ? fmaf(g, zz, sls[c]) : sls[c];
            }
            d3[4] = gv;
            d3[5] = 0.0f;
            sb3[4] = sb3[4] + gv;
            const float hv = 0.5f * verr;
            const float hq = 0.5f * sq;
            const float l = nll ? -logp : hq;
            st[0] = st[0] + (active ? w * l : 0.0f);
            st[1] = st[1] + (active ? hv * verr : 0.0f);
            st[2] = st[2] + (active ? sq : 0.0f);
            st[3] = st[3] + (active ? w : 0.0f);
            st[4] = st[4] + (active ? logp : 0.0f);
            st[5] = st[5] + (skipped ? 1.0f : 0.0f);
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) R3[c * kXS + lane] = d3[c];

        // ---- d[W3; w_v] = d3 x H2
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            put_half(RB, h2[0][nt], h2[1][nt], i, h);
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 A4 = *reinterpret_cast<const float4*>(R3 + (i & 7) * kXS + 32 * nt + 8 * q + 4 * h);
                const float4 B0 = *reinterpret_cast<const float4*>(RB + i * kTS + 8 * q + 4 * h);
                const float4 B1 = *reinterpret_cast<const float4*>(RB + (32 + i) * kTS + 8 * q + 4 * h);
                const float Ae[4] = {A4.x, A4.y, A4.z, A4.w};
                const float B0e[4] = {B0.x, B0.y, B0.z, B0.w}, B1e[4] = {B1.x, B1.y, B1.z, B1.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc3[0] = HG_MFMA(Ae[e], B0e[e], acc3[0]);
                    acc3[1] = HG_MFMA(Ae[e], B1e[e], acc3[1]);
                }
            }
            wave_lds_sync();
        }

        // ---- dH2 = [W3; w_v]^T d3, D2 = dH2 (1 - H2^2)  (h2 becomes D2)
        f32x16 g1[2][2] = {{zero, zero}, {zero, zero}};
        {
            f32x16 g2[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(d3[2 * kk]), __float_as_uint(d3[2 * kk + 1]),
                                                                 false, false);
                const float b0 = __uint_as_float(sw[0]), b1 = __uint_as_float(sw[1]);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const float w = img[(kSB3 + mt * 3 + kk) * 64];
                    g2[mt][0] = HG_MFMA(w, b0, g2[mt][0]);
                    g2[mt][1] = HG_MFMA(w, b1, g2[mt][1]);
                }
            }
        // ---- dH1 = W2^T D2, each D2 formed where it becomes an operand
#pragma unroll
            for (int kp = 0; kp < 32; ++kp) {
                float b[2];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float hh = h2[kp >> 4][nt][kp & 15];
                    const float dt = 1.0f - hh * hh;
                    b[nt] = g2[kp >> 4][nt][kp & 15] * dt;
                    h2[kp >> 4][nt][kp & 15] = b[nt];
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const float w = img[(kSB2 + mt * 32 + kp) * 64];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) g1[mt][nt] = HG_MFMA(w, b[nt], g1[mt][nt]);
                }
            }
        }
        // ---- dW2 = D2 x H1, db2 = D2's row sums
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            put_half(RA, h2[0][nt], h2[1][nt], i, h);
            put_half(RB, h1[0][nt], h1[1][nt], i, h);
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 A0 = *reinterpret_cast<const float4*>(RA + i * kTS + 8 * q + 4 * h);
                const float4 A1 = *reinterpret_cast<const float4*>(RA + (32 + i) * kTS + 8 * q + 4 * h);
                const float4 B0 = *reinterpret_cast<const float4*>(RB + i * kTS + 8 * q + 4 * h);
                const float4 B1 = *reinterpret_cast<const float4*>(RB + (32 + i) * kTS + 8 * q + 4 * h);
                const float A0e[4] = {A0.x, A0.y, A0.z, A0.w}, A1e[4] = {A1.x, A1.y, A1.z, A1.w};
                const float B0e[4] = {B0.x, B0.y, B0.z, B0.w}, B1e[4] = {B1.x, B1.y, B1.z, B1.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sb2[0] = sb2[0] + A0e[e];
                    sb2[1] = sb2[1] + A1e[e];
                    accW2[0][0] = HG_MFMA(A0e[e], B0e[e], accW2[0][0]);
                    accW2[0][1] = HG_MFMA(A0e[e], B1e[e], accW2[0][1]);
                    accW2[1][0] = HG_MFMA(A1e[e], B0e[e], accW2[1][0]);
                    accW2[1][1] = HG_MFMA(A1e[e], B1e[e], accW2[1][1]);
                }
            }
            wave_lds_sync();
        }
        // ---- D1 = dH1 (1 - H1^2), dW1 (and db1, its column 17) = D1 x [x; 1]
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float hh = h1[mt][nt][r];
                    const float dt = 1.0f - hh * hh;
                    g1[mt][nt][r] = g1[mt][nt][r] * dt;
                }
        const int xr = i < 17 ? i : 17;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            put_half(RA, g1[0][nt], g1[1][nt], i, h);
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 A0 = *reinterpret_cast<const float4*>(RA + i * kTS + 8 * q + 4 * h);
                const float4 A1 = *reinterpret_cast<const float4*>(RA + (32 + i) * kTS + 8 * q + 4 * h);
                const float4 B4 = *reinterpret_cast<const float4*>(RX + xr * kXS + 32 * nt + 8 * q + 4 * h);
                const float A0e[4] = {A0.x, A0.y, A0.z, A0.w}, A1e[4] = {A1.x, A1.y, A1.z, A1.w};
                const float Be[4] = {B4.x, B4.y, B4.z, B4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    accW1[0] = HG_MFMA(A0e[e], Be[e], accW1[0]);
                    accW1[1] = HG_MFMA(A1e[e], Be[e], accW1[1]);
                }
            }
            wave_lds_sync();
        }
    }

    // ---- the block's sum: the waves add their registers in wave order, at each parameter's flat index
    sb2[0] = sb2[0] + __shfl_xor(sb2[0], 32, 64);
    sb2[1] = sb2[1] + __shfl_xor(sb2[1], 32, 64);
#pragma unroll
    for (int c = 0; c < 5; ++c) sb3[c] = wave_sum(sb3[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) sls[c] = wave_sum(sls[c]);
#pragma unroll
    for (int c = 0; c < 6; ++c) st[c] = wave_sum(st[c]);
    __syncthreads();   // every wave is done with the weight image
    float* const sum = s_img;
#pragma unroll 1
    for (int w = 0; w < kWaves; ++w) {
        if (wave == w) {
            const bool first = w == 0;
            auto add = [&](int idx, float v) { sum[idx] = first ? v : sum[idx] + v; };
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int out = 32 * mt + acc_row(r, h);
                    add(kPpoW2 + out * 64 + i, accW2[mt][0][r]);
                    add(kPpoW2 + out * 64 + 32 + i, accW2[mt][1][r]);
                    if (i < 17) add(kPpoW1 + out * 17 + i, accW1[mt][r]);
                    if (i == 17) add(kPpoB1 + out, accW1[mt][r]);
                }
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2) {
                if (!h) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) add(kPpoW3 + c * 64 + 32 * n2 + i, acc3[n2][c]);
                    add(kPpoB2 + 32 * n2 + i, sb2[n2]);
                } else {
                    add(kPpoWv + 32 * n2 + i, acc3[n2][0]);
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    add(kPpoB3 + c, sb3[c]);
                    add(kPpoLogStd + c, sls[c]);
                }
                add(kPpoBv, sb3[4]);
#pragma unroll
                for (int c = 0; c < 6; ++c) add(kPpoStatsOff + c, st[c]);
            }
            if (lane >= 1 && lane < 8) {   // the partial's padding
                if (first) sum[kPpoParams + lane - 1] = 0.0f;
                if (first && lane < 3) sum[kPpoStatsOff + 5 + lane] = 0.0f;
            }
        }
        __syncthreads();
    }
    float* __restrict__ dst = a.ws + (int64_t)blockIdx.x * kPpoPartialFloats;
    for (int e = tid; e < kPpoPartialFloats; e += kThreads) dst[e] = sum[e];
}

__global__ __launch_bounds__(kThreads) void ppo_grad_kernel(const PpoGradArgs a, const int64_t tiles) {
    grad_body<kLossPpo>(a, tiles, 0);
}

__global__ __launch_bounds__(kThreads) void bc_grad_kernel(const PpoGradArgs a, const int64_t tiles, const int mode) {
    grad_body<kLossBc>(a, tiles, mode);
}

// grad[p] = the partials' sum: chain c = 0 .. 3 adds the blocks b = c, c + 4, .. in ascending order (one
// thread per parameter and chain, 64 parameters per block, the loads sixteen deep), then
// ((chain 0 + chain 1) + (chain 2 + chain 3)); the entropy term's constant -ent_coef on log_std.  The
// statistics, entries 5648 .. 5653 of the partials, are summed the same way and finished by one thread.
constexpr int kRedParams = 64;
constexpr int kRedItems = kPpoStatsOff + 6;   // parameters, padding, six statistic sums

__global__ __launch_bounds__(256) void ppo_reduce_kernel(const float* __restrict__ ws, int nb, const float* __restrict__ theta,
                                                         float vf_coef, float ent_coef, float inv_m,
                                                         float* __restrict__ grad, float* __restrict__ stats) {
    __shared__ float s_part[4][kRedParams];
    const int j = threadIdx.x & (kRedParams - 1), c = threadIdx.x >> 6;
    const int idx = blockIdx.x * kRedParams + j;
    float s = 0.0f;
    if (idx < kRedItems) {
        const float* __restrict__ src = ws + idx;
        int b = c;
        for (; b + 60 < nb; b += 64) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = src[(int64_t)(b + 4 * u) * kPpoPartialFloats];
#pragma unroll
            for (int u = 0; u < 16; ++u) s = s + v[u];
        }
        for (; b < nb; b += 4) s = s + src[(int64_t)b * kPpoPartialFloats];
    }
    s_part[c][j] = s;
    __syncthreads();
    if (c != 0 || idx >= kRedItems) return;
    float g = (s_part[0][j] + s_part[1][j]) + (s_part[2][j] + s_part[3][j]);
    if (idx < kPpoParams) {
        if (idx >= kPpoLogStd && idx < kPpoLogStd + 4) g = g - ent_coef;
        grad[idx] = g;
    }
    // the six statistic sums sit in one block (5648 = 88 * 64 + 16): its lane 16 finishes them
    static_assert(kPpoStatsOff / kRedParams == (kPpoStatsOff + 5) / kRedParams, "the statistics' sums share a block");
    if (stats != nullptr && idx == kPpoStatsOff) {
        float q[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k] = (s_part[0][j + k] + s_part[1][j + k]) + (s_part[2][j + k] + s_part[3][j + k]);
        const float ls = ((theta[kPpoLogStd] + theta[kPpoLogStd + 1]) + theta[kPpoLogStd + 2]) + theta[kPpoLogStd + 3];
        const float H = ls + 5.67575413281869070f;   // 2 (1 + ln 2 pi)
        const float pol = q[0] * inv_m, val = q[1] * inv_m;
        stats[0] = pol;
        stats[1] = val;
        stats[2] = q[2] * inv_m;
        stats[3] = q[3] * inv_m;
        stats[4] = H;
        const float pv = fmaf(vf_coef, val, pol);
        stats[5] = fmaf(-ent_coef, H, pv);
        stats[6] = q[4] * inv_m;
        stats[7] = q[5];
    }
}

}  // namespace

// the gradient kernel `launch` enqueues, then the reduction: the grid is a function of M alone
template <typename Launch>
static hipError_t launch_grad(const PpoGradArgs& a, hipStream_t stream, Launch launch) {
    const int64_t tiles = (a.M + 63) / 64;
    const int64_t want = (tiles + kWaves - 1) / kWaves;
    const int nb = (int)(want < kPpoMaxBlocks ? want : kPpoMaxBlocks);
    launch(nb, tiles);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((kRedItems + kRedParams - 1) / kRedParams), dim3(256), 0, stream, (const float*)a.ws, nb,
                       a.theta, a.vf_coef, a.ent_coef, a.inv_m, a.grad, a.stats);
    return hipGetLastError();
}

hipError_t launch_ppo_grad(const PpoGradArgs& a, hipStream_t stream) {
    return launch_grad(a, stream, [&](int nb, int64_t tiles) {
        hipLaunchKernelGGL(ppo_grad_kernel, dim3(nb), dim3(kThreads), 0, stream, a, tiles);
    });
}

hipError_t launch_bc_grad(const PpoGradArgs& a, int mode, hipStream_t stream) {
    return launch_grad(a, stream, [&](int nb, int64_t tiles) {
        hipLaunchKernelGGL(bc_grad_kernel, dim3(nb), dim3(kThreads), 0, stream, a, tiles, mode);
    });
}

}  // namespace hgk
