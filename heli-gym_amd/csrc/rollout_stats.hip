// rollout_stats.hip — running observation / return normalisation and episode statistics of a rollout on the
// device (include/heligym_amd.h, hg_rollout_stats): one pass over what hg_rollout_ac wrote.
//
// Three launches on the caller's stream, the shape of each a function of (K, N) and the constants below only:
//
//  1. stats_pass_kernel, two kinds of blocks side by side in one grid (they share no data):
//     a. the scan blocks, first in the grid.  One lane per env walks its K rewards and flags in step order
//        (each row a coalesced access, eight steps' loads issued ahead of the dependent chain, as gae_kernel
//        does with four): the discounted return G, the episode return and length, the return moments'
//        shifted fp64 sums and the episode aggregates.  At most kStatsScanBlocksMax blocks; past
//        kStatsScanBlocksMax * 256 envs a lane takes several envs, its sums running on.
//     b. the observation blocks: the moments and the shifted copy.  Neither cares which step or env a row
//        belongs to: obs [K,N,17] is K N rows of 17 floats, and obs_in is the same floats N rows further on,
//        behind obs0's N rows.  So the pass is tiled over the FLAT rows, kStatsTileRows = 1024 rows (17 408
//        floats, a multiple of both 17 and 4) per tile: a thread issues the tile's 17 16-byte loads, stores
//        the same registers to obs_in (16-byte stores when N is a multiple of 4, so that the shifted rows
//        keep the alignment; 4-byte stores otherwise) and to LDS, and requests its next tile; then a thread
//        per row overwrites the LDS rows that hold a non-finite value with NaNs (such a row leaves all 17
//        sums; the copy has its bits already), and 255 threads as 15 groups of 17 columns read the
//        tile back column-wise (consecutive lanes, consecutive words: no bank conflict) and add x - c and
//        (x - c)^2 in fp64 while the next tile's loads are in flight.  At most kStatsObsBlocksMax blocks, two
//        per CU by their LDS; past that many tiles a block takes several, its sums running on.
//  2. stats_finalise_kernel.  One block: wave w adds the blocks' partials of quantities w, w + 16, .. (lane l
//     the blocks l, l + 64, .. in ascending order, then the xor butterfly 32, 16, .. 1), and one thread per
//     column / part does the Chan merge into the fp64 head and forms the outputs.
//  3. stats_scale_kernel, only with reward_out: reward * scale, clamped, the scale read from the device.
//
// Determinism: no atomics; every sum above is in an order fixed by (K, N) and the constants.
#include "rollout_stats.h"

#include "../../include/heligym_amd.h"

namespace hgk {
namespace {

constexpr int kStatsThreads = 256, kStatsWaves = kStatsThreads / 64;
constexpr int kScanUnroll = 8;
constexpr int kStatsTileRows = 1024, kTileFloats = kStatsTileRows * kStatsCols;
constexpr int kTileVecs = kTileFloats / 4 / kStatsThreads;       // 16-byte loads per thread and tile: 17
constexpr int kColGroups = kStatsThreads / kStatsCols;           // 15 groups of 17 column threads
constexpr int kColRowsPerThread = (kStatsTileRows + kColGroups - 1) / kColGroups;   // 69 rows of a tile per column thread
constexpr int kFinalThreads = 1024, kFinalWaves = kFinalThreads / 64;
constexpr int kFinalRounds = (kStatsObsQ + kStatsScanQ + kFinalWaves - 1) / kFinalWaves;   // quantities per wave: 4
constexpr int kFinalPerLane = kStatsObsBlocksMax / 64;                                      // blocks per lane: 8
static_assert(kStatsObsBlocksMax % 64 == 0 && kStatsScanBlocksMax <= kStatsObsBlocksMax, "finalise shape");
static_assert(kTileFloats % (4 * kStatsThreads) == 0 && kStatsTileRows % kStatsThreads == 0, "tile shape");

// the scan's per-block partials
enum { kQRetN = 0, kQRetS1, kQRetS2, kQRetSkipped, kQRewSum, kQRewN, kQEpisodes, kQTerminated, kQTruncated,
       kQSuccess, kQEpNonfinite, kQEpRetSum, kQEpRetSq, kQEpLenSum, kQEpRetMin, kQEpRetMax };
static_assert(kQEpRetMax + 1 == kStatsScanQ, "scan partials");

struct Views {
    double* head;
    float* G;
    float* ep_ret;
    int32_t* ep_len;
    double* ws_obs;
    double* ws_scan;
    float* ws_scale;
};

__host__ __device__ __forceinline__ Views views_of(void* state, int64_t n) {
    Views v;
    char* const base = static_cast<char*>(state);
    v.head = reinterpret_cast<double*>(base);
    v.G = reinterpret_cast<float*>(base + kStatsHeadBytes);
    v.ep_ret = v.G + n;
    v.ep_len = reinterpret_cast<int32_t*>(v.ep_ret + n);
    v.ws_obs = reinterpret_cast<double*>(base + kStatsHeadBytes + stats_env_bytes(n));
    v.ws_scan = v.ws_obs + (int64_t)kStatsObsQ * kStatsObsBlocksMax;
    v.ws_scale = reinterpret_cast<float*>(v.ws_scan + (int64_t)kStatsScanQ * kStatsScanBlocksMax);
    return v;
}

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ the scans
struct ScanAcc {
    double ret_s1 = 0.0, ret_s2 = 0.0, rew_sum = 0.0, ep_sum = 0.0, ep_sq = 0.0, ep_len_sum = 0.0;
    uint32_t ret_n = 0, ret_skipped = 0, rew_n = 0, episodes = 0, terminated = 0, truncated = 0, success = 0,
             ep_nonfinite = 0;
    float ep_min = __builtin_inff(), ep_max = -__builtin_inff();
};

// one env-step, in the header's order.  fl: bit 0 terminated, bit 1 truncated, bit 2 success
// Selections, no branches: what does not enter a sum enters it as +0.0, which changes no bit of it (x + 0.0 = x,
// fma(0, 0, x) = x), and the steps of a batch are one basic block whose independent fp64 chains interleave on
// the one wave a SIMD has here.
__device__ __forceinline__ void scan_step(ScanAcc& s, float& G, float& er, int32_t& el, float r, uint32_t fl,
                                          float gamma, double c) {
    G = fmaf(gamma, G, r);
    const bool g_ok = finite32(G);
    const double d = g_ok ? (double)G - c : 0.0;
    s.ret_s1 = s.ret_s1 + d;
    s.ret_s2 = fma(d, d, s.ret_s2);
    s.ret_n += g_ok ? 1u : 0u;
    s.ret_skipped += g_ok ? 0u : 1u;
    er = er + r;
    el = el + 1;
    const bool r_ok = finite32(r);
    s.rew_sum = s.rew_sum + (r_ok ? (double)r : 0.0);
    s.rew_n += r_ok ? 1u : 0u;
    const bool done = (fl & 3u) != 0u, e_ok = done && finite32(er);
    const double e = e_ok ? (double)er : 0.0;
    s.ep_sum = s.ep_sum + e;
    s.ep_sq = fma(e, e, s.ep_sq);
    s.ep_min = fminf(s.ep_min, e_ok ? er : __builtin_inff());
    s.ep_max = fmaxf(s.ep_max, e_ok ? er : -__builtin_inff());
    s.episodes += done ? 1u : 0u;
    s.terminated += fl & 1u;
    s.truncated += (fl & 3u) == 2u ? 1u : 0u;
    s.success += (done && (fl & 4u)) ? 1u : 0u;
    s.ep_nonfinite += (done && !e_ok) ? 1u : 0u;
    s.ep_len_sum = s.ep_len_sum + (done ? (double)el : 0.0);
    G = done ? 0.0f : G;
    er = done ? 0.0f : er;
    el = done ? 0 : el;
}

__device__ __forceinline__ uint32_t scan_flags(const RolloutStatsArgs& a, int64_t r) {
    uint32_t fl = (a.terminated[r] != 0 ? 1u : 0u) | (a.truncated[r] != 0 ? 2u : 0u);
    if (a.info) fl |= (a.info[r] & HG_INFO_SUCCESSED) ? 4u : 0u;
    return fl;
}

// block `block` of the `nblocks` scan blocks of the pass
__device__ __forceinline__ void scan_block(const RolloutStatsArgs& a, int block, int nblocks) {
    __shared__ double s_part[kStatsWaves][kStatsScanQ];
    const Views v = views_of(a.state, a.n);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double c = v.head[kStatsRetCount] > 0.0 ? v.head[kStatsRetMean] : 0.0;
    const int32_t K = a.nsteps;
    const int64_t n = a.n;
    ScanAcc s;
    for (int64_t i = (int64_t)block * kStatsThreads + tid; i < n; i += (int64_t)nblocks * kStatsThreads) {
        float G = v.G[i], er = v.ep_ret[i];
        int32_t el = v.ep_len[i];
        int32_t k = 0;
        for (; k + kScanUnroll <= K; k += kScanUnroll) {
            float r[kScanUnroll];
            uint32_t fl[kScanUnroll];
#pragma unroll
            for (int j = 0; j < kScanUnroll; ++j) {
                const int64_t row = (int64_t)(k + j) * n + i;
                r[j] = a.reward[row];
                fl[j] = scan_flags(a, row);
            }
#pragma unroll
            for (int j = 0; j < kScanUnroll; ++j) scan_step(s, G, er, el, r[j], fl[j], a.gamma, c);
        }
        if (k < K) {   // the last K % kScanUnroll steps: one more batch, its loads issued together as well
            float r[kScanUnroll];
            uint32_t fl[kScanUnroll];
#pragma unroll
            for (int j = 0; j < kScanUnroll - 1; ++j) {
                const int64_t row = (int64_t)(k + j < K ? k + j : K - 1) * n + i;
                r[j] = a.reward[row];
                fl[j] = scan_flags(a, row);
            }
#pragma unroll
            for (int j = 0; j < kScanUnroll - 1; ++j)
                if (k + j < K) scan_step(s, G, er, el, r[j], fl[j], a.gamma, c);
        }
        v.G[i] = G;
        v.ep_ret[i] = er;
        v.ep_len[i] = el;
    }
    double q[kStatsScanQ];
    q[kQRetN] = (double)s.ret_n;
    q[kQRetS1] = s.ret_s1;
    q[kQRetS2] = s.ret_s2;
    q[kQRetSkipped] = (double)s.ret_skipped;
    q[kQRewSum] = s.rew_sum;
    q[kQRewN] = (double)s.rew_n;
    q[kQEpisodes] = (double)s.episodes;
    q[kQTerminated] = (double)s.terminated;
    q[kQTruncated] = (double)s.truncated;
    q[kQSuccess] = (double)s.success;
    q[kQEpNonfinite] = (double)s.ep_nonfinite;
    q[kQEpRetSum] = s.ep_sum;
    q[kQEpRetSq] = s.ep_sq;
    q[kQEpLenSum] = s.ep_len_sum;
    q[kQEpRetMin] = (double)s.ep_min;
    q[kQEpRetMax] = (double)s.ep_max;
#pragma unroll
    for (int j = 0; j < kStatsScanQ; ++j) {
        double x = q[j];
        if (j == kQEpRetMin) {
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) x = fmin(x, __shfl_xor(x, k, 64));
        } else if (j == kQEpRetMax) {
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) x = fmax(x, __shfl_xor(x, k, 64));
        } else {
            x = wave_sum(x);
        }
        if (lane == 0) s_part[wave][j] = x;
    }
    __syncthreads();
    if (tid < kStatsScanQ) {
        double x = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < kStatsWaves; ++w) {
            const double y = s_part[w][tid];
            x = tid == kQEpRetMin ? fmin(x, y) : tid == kQEpRetMax ? fmax(x, y) : x + y;
        }
        v.ws_scan[(int64_t)tid * kStatsScanBlocksMax + block] = x;
    }
}

// --------------------------------------------------------------------------------------- the observation pass
typedef float f4 __attribute__((ext_vector_type(4)));

// floats f .. f + 3 of p, those below `total` (f a multiple of 4, p 16-byte aligned); the others 0
__device__ __forceinline__ f4 load4_guard(const float* __restrict__ p, int64_t f, int64_t total) {
    f4 x = {0.0f, 0.0f, 0.0f, 0.0f};
    if (f + 3 < total) {
        x = *reinterpret_cast<const f4*>(p + f);
    } else {
        if (f < total) x.x = p[f];
        if (f + 1 < total) x.y = p[f + 1];
        if (f + 2 < total) x.z = p[f + 2];
    }
    return x;
}

// x to floats f .. f + 3 of p, those below `lim`; one 16-byte store when `vec` (p + f is then 16-byte aligned)
__device__ __forceinline__ void store4_guard(float* __restrict__ p, int64_t f, f4 x, int64_t lim, bool vec) {
    if (vec && f + 3 < lim) {
        *reinterpret_cast<f4*>(p + f) = x;
    } else {
        if (f < lim) p[f] = x.x;
        if (f + 1 < lim) p[f + 1] = x.y;
        if (f + 2 < lim) p[f + 2] = x.z;
        if (f + 3 < lim) p[f + 3] = x.w;
    }
}

// the shift of the observation sums: the state's mean, or the batch's first row (its finite values) for a fresh state
__device__ __forceinline__ double obs_shift(const double* head, const float* obs, int col) {
    if (head[kStatsObsCount] > 0.0) return head[kStatsObsMean + col];
    const float x = obs[col];
    return finite32(x) ? (double)x : 0.0;
}

// thread tid's 17 16-byte pieces of tile `tile` of obs (zeros past the end)
__device__ __forceinline__ void load_tile(f4 (&x)[kTileVecs], const float* __restrict__ obs, int64_t tile, int64_t total,
                                          int tid) {
    const int64_t f0 = tile * kTileFloats;
    if (f0 + kTileFloats <= total) {
#pragma unroll
        for (int u = 0; u < kTileVecs; ++u)
            x[u] = *reinterpret_cast<const f4*>(obs + f0 + (int64_t)(u * kStatsThreads + tid) * 4);
    } else {
#pragma unroll
        for (int u = 0; u < kTileVecs; ++u) x[u] = load4_guard(obs, f0 + (int64_t)(u * kStatsThreads + tid) * 4, total);
    }
}

// block `block` of the `nblocks` observation blocks of the pass
__device__ __forceinline__ void obs_block(const RolloutStatsArgs& a, int64_t ntiles, int block, int nblocks) {
    __shared__ __attribute__((aligned(16))) float s_tile[kTileFloats];
    __shared__ double s_sum[2][kColGroups][kStatsCols];
    __shared__ uint32_t s_cnt[2][kStatsWaves];
    const Views v = views_of(a.state, a.n);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = tid % kStatsCols, grp = tid / kStatsCols;
    const bool col_thread = grp < kColGroups;
    const double c = col_thread ? obs_shift(v.head, a.obs, col) : 0.0;
    const int64_t rows = (int64_t)a.nsteps * a.n, total = rows * kStatsCols;
    const int64_t shift = a.n * kStatsCols;        // obs_in is obs, `shift` floats further on, behind obs0
    const int64_t copy_lim = total - shift;        // the last step's rows are not copied
    const bool vec_shift = (a.n & 3) == 0;
    double s1 = 0.0, s2 = 0.0;
    uint32_t valid = 0, skipped = 0;
    f4 x[kTileVecs];
    if (block < ntiles) load_tile(x, a.obs, block, total, tid);
    for (int64_t tile = block; tile < ntiles; tile += nblocks) {
        const int64_t f0 = tile * kTileFloats;
#pragma unroll
        for (int u = 0; u < kTileVecs; ++u) reinterpret_cast<f4*>(s_tile)[u * kStatsThreads + tid] = x[u];
        if (a.obs_in_out) {
            float* const dst = a.obs_in_out + shift;
            if (vec_shift && f0 + kTileFloats <= copy_lim) {
#pragma unroll
                for (int u = 0; u < kTileVecs; ++u)
                    *reinterpret_cast<f4*>(dst + f0 + (int64_t)(u * kStatsThreads + tid) * 4) = x[u];
            } else if (f0 < copy_lim) {
#pragma unroll
                for (int u = 0; u < kTileVecs; ++u)
                    store4_guard(dst, f0 + (int64_t)(u * kStatsThreads + tid) * 4, x[u], copy_lim, vec_shift);
            }
            if (f0 < shift) {   // the tiles over the first N rows also carry obs0 to them: all loads, then all stores
                f4 w[kTileVecs];
                load_tile(w, a.obs0, tile, shift, tid);
                if (f0 + kTileFloats <= shift) {
#pragma unroll
                    for (int u = 0; u < kTileVecs; ++u)
                        *reinterpret_cast<f4*>(a.obs_in_out + f0 + (int64_t)(u * kStatsThreads + tid) * 4) = w[u];
                } else {
#pragma unroll
                    for (int u = 0; u < kTileVecs; ++u)
                        store4_guard(a.obs_in_out, f0 + (int64_t)(u * kStatsThreads + tid) * 4, w[u], shift, true);
                }
            }
        }
        __syncthreads();
        // the block's next tile is requested now: its loads are in flight while this one is summed from the LDS
        if (tile + nblocks < ntiles) load_tile(x, a.obs, tile + nblocks, total, tid);
#pragma unroll
        for (int j = 0; j < kStatsTileRows / kStatsThreads; ++j) {
            const int row = j * kStatsThreads + tid;
            const bool in = tile * kStatsTileRows + row < rows;
            float y[kStatsCols];
#pragma unroll
            for (int cc = 0; cc < kStatsCols; ++cc) y[cc] = s_tile[row * kStatsCols + cc];   // (all 17 reads, then the test)
            uint32_t bad = 0u;
#pragma unroll
            for (int cc = 0; cc < kStatsCols; ++cc) bad |= finite32(y[cc]) ? 0u : 1u;
            if (bad != 0u || !in) {   // the row leaves the sums: the column threads skip what is not finite
#pragma unroll
                for (int cc = 0; cc < kStatsCols; ++cc) s_tile[row * kStatsCols + cc] = __builtin_nanf("");
            }
            valid += (in && bad == 0u) ? 1u : 0u;
            skipped += (in && bad != 0u) ? 1u : 0u;
        }
        __syncthreads();
        if (col_thread) {
            // rows grp, grp + 15, ..: selections, no branches, so that the LDS reads of several rows are in flight
#pragma unroll 8
            for (int i = 0; i < kColRowsPerThread; ++i) {
                const int row = grp + i * kColGroups;
                const float xv = s_tile[(row < kStatsTileRows ? row : kStatsTileRows - 1) * kStatsCols + col];
                const bool ok = row < kStatsTileRows && finite32(xv);
                const double d = ok ? (double)xv - c : 0.0;
                s1 = s1 + d;
                s2 = fma(d, d, s2);
            }
        }
        __syncthreads();   // (the next tile overwrites the LDS)
    }
    if (col_thread) {
        s_sum[0][grp][col] = s1;
        s_sum[1][grp][col] = s2;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        valid += __shfl_xor(valid, k, 64);
        skipped += __shfl_xor(skipped, k, 64);
    }
    if (lane == 0) {
        s_cnt[0][wave] = valid;
        s_cnt[1][wave] = skipped;
    }
    __syncthreads();
    if (tid < 2 * kStatsCols) {
        const int which = tid / kStatsCols, cc = tid % kStatsCols;
        double t = s_sum[which][0][cc];
#pragma unroll
        for (int g = 1; g < kColGroups; ++g) t = t + s_sum[which][g][cc];
        v.ws_obs[(int64_t)(1 + which * kStatsCols + cc) * kStatsObsBlocksMax + block] = t;
    } else if (tid < 2 * kStatsCols + 2) {
        const int which = tid - 2 * kStatsCols;
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kStatsWaves; ++w) t += s_cnt[which][w];
        v.ws_obs[(int64_t)(which ? kStatsObsQ - 1 : 0) * kStatsObsBlocksMax + block] = (double)t;
    }
}

// The pass: the first nb_scan blocks are the scans (the longest dependent chains start first), the others the
// observation blocks; the two kinds share no data, so they simply run side by side.
__global__ __launch_bounds__(kStatsThreads) void stats_pass_kernel(const RolloutStatsArgs a, int nb_scan, int64_t ntiles) {
    const int b = (int)blockIdx.x;
    if (b < nb_scan) scan_block(a, b, nb_scan);
    else obs_block(a, ntiles, b - nb_scan, (int)gridDim.x - nb_scan);
}

// ----------------------------------------------------------------------------------------- merge and finalise
struct Moments {
    double n, mean, m2;
};

// Chan's update of `a` by a batch of nb samples with the shifted sums s1 = sum (x - c), s2 = sum (x - c)^2
__device__ __forceinline__ Moments chan_merge(Moments a, double nb, double c, double s1, double s2) {
    if (!(nb > 0.0)) return a;
    const double mean_b = c + s1 / nb;
    const double m2_b = fmax(0.0, s2 - s1 * (s1 / nb));
    if (!(a.n > 0.0)) return Moments{nb, mean_b, m2_b};
    const double n = a.n + nb, delta = mean_b - a.mean;
    Moments r;
    r.n = n;
    r.mean = a.mean + delta * (nb / n);
    r.m2 = a.m2 + m2_b + delta * delta * (a.n * (nb / n));
    return r;
}

__global__ __launch_bounds__(kFinalThreads) void stats_finalise_kernel(const RolloutStatsArgs a, int nb_obs, int nb_scan) {
    __shared__ double s_tot[kStatsObsQ + kStatsScanQ];
    const Views v = views_of(a.state, a.n);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // a wave's quantities (at most kFinalRounds) and a lane's blocks of each (at most kFinalPerLane): every load is
    // issued before the first sum; a slot without a block holds the operation's identity
    double y[kFinalRounds][kFinalPerLane];
#pragma unroll
    for (int r = 0; r < kFinalRounds; ++r) {
        const int q = wave + r * kFinalWaves, sq = q - kStatsObsQ;
        const bool is_obs = q < kStatsObsQ, live = q < kStatsObsQ + kStatsScanQ;
        const double* const p = !live    ? v.ws_scan
                                : is_obs ? v.ws_obs + (int64_t)q * kStatsObsBlocksMax
                                         : v.ws_scan + (int64_t)sq * kStatsScanBlocksMax;
        const int nb = !live ? 0 : is_obs ? nb_obs : nb_scan;
        const double id = sq == kQEpRetMin ? (double)__builtin_inff() : sq == kQEpRetMax ? -(double)__builtin_inff() : 0.0;
#pragma unroll
        for (int j = 0; j < kFinalPerLane; ++j) y[r][j] = lane + 64 * j < nb ? p[lane + 64 * j] : id;
    }
#pragma unroll
    for (int r = 0; r < kFinalRounds; ++r) {
        const int q = wave + r * kFinalWaves, sq = q - kStatsObsQ;
        const bool is_min = sq == kQEpRetMin, is_max = sq == kQEpRetMax;
        double x = y[r][0];
#pragma unroll
        for (int j = 1; j < kFinalPerLane; ++j) x = is_min ? fmin(x, y[r][j]) : is_max ? fmax(x, y[r][j]) : x + y[r][j];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            const double z = __shfl_xor(x, k, 64);
            x = is_min ? fmin(x, z) : is_max ? fmax(x, z) : x + z;
        }
        if (lane == 0 && q < kStatsObsQ + kStatsScanQ) s_tot[q] = x;
    }
    // every thread reads what it needs of the head before any thread rewrites it
    const bool col_thread = tid < kStatsCols, ret_thread = tid == 64, ep_thread = tid == 128;
    Moments m = {0.0, 0.0, 0.0};
    double c = 0.0, life[4] = {0.0, 0.0, 0.0, 0.0};
    if (col_thread) {
        m = Moments{v.head[kStatsObsCount], v.head[kStatsObsMean + tid], v.head[kStatsObsM2 + tid]};
        c = obs_shift(v.head, a.obs, tid);
    } else if (ret_thread) {
        m = Moments{v.head[kStatsRetCount], v.head[kStatsRetMean], v.head[kStatsRetM2]};
        c = m.n > 0.0 ? m.mean : 0.0;
    } else if (ep_thread) {
#pragma unroll
        for (int j = 0; j < 4; ++j) life[j] = v.head[kStatsEpisodes + j];
    }
    __syncthreads();
    const double* const sc = s_tot + kStatsObsQ;
    if (col_thread) {
        if (a.update & HG_STATS_UPDATE_OBS) {
            m = chan_merge(m, s_tot[0], c, s_tot[1 + tid], s_tot[1 + kStatsCols + tid]);
            if (tid == 0) v.head[kStatsObsCount] = m.n;
            v.head[kStatsObsMean + tid] = m.mean;
            v.head[kStatsObsM2 + tid] = m.m2;
        }
        const bool any = m.n > 0.0;
        if (a.obs_mean_out) a.obs_mean_out[tid] = any ? (float)m.mean : 0.0f;
        if (a.obs_scale_out)
            a.obs_scale_out[tid] = any ? fminf((float)(1.0 / sqrt(m.m2 / m.n + a.obs_eps)), a.max_obs_scale) : 1.0f;
    } else if (ret_thread) {
        if (a.update & HG_STATS_UPDATE_RET) {
            m = chan_merge(m, sc[kQRetN], c, sc[kQRetS1], sc[kQRetS2]);
            v.head[kStatsRetCount] = m.n;
            v.head[kStatsRetMean] = m.mean;
            v.head[kStatsRetM2] = m.m2;
        }
        const float scale = m.n > 0.0 ? (float)(1.0 / sqrt(m.m2 / m.n + a.ret_eps)) : 1.0f;
        v.ws_scale[0] = scale;
        if (a.reward_scale_out) a.reward_scale_out[0] = scale;
    } else if (ep_thread) {
        if (a.update != 0u) {
            v.head[kStatsEpisodes] = life[0] + sc[kQEpisodes];
            v.head[kStatsEnvSteps] = life[1] + (double)a.nsteps * (double)a.n;
        }
        if (a.update & HG_STATS_UPDATE_OBS) v.head[kStatsSkippedRows] = life[2] + s_tot[kStatsObsQ - 1];
        if (a.update & HG_STATS_UPDATE_RET) v.head[kStatsSkippedReturns] = life[3] + sc[kQRetSkipped];
        if (a.episode_out) {
            const double nan = __builtin_nan("");
            const double episodes = sc[kQEpisodes], counted = episodes - sc[kQEpNonfinite];
            const bool some = counted > 0.0;
            const double mean = sc[kQEpRetSum] / counted;
            float* const o = a.episode_out;
            o[0] = (float)episodes;
            o[1] = (float)(some ? mean : nan);
            o[2] = (float)(some ? sqrt(fmax(0.0, sc[kQEpRetSq] / counted - mean * mean)) : nan);
            o[3] = (float)(some ? sc[kQEpRetMin] : nan);
            o[4] = (float)(some ? sc[kQEpRetMax] : nan);
            o[5] = (float)(episodes > 0.0 ? sc[kQEpLenSum] / episodes : nan);
            o[6] = (float)sc[kQTerminated];
            o[7] = (float)sc[kQTruncated];
            o[8] = (float)sc[kQSuccess];
            o[9] = (float)(sc[kQRewN] > 0.0 ? sc[kQRewSum] / sc[kQRewN] : nan);
            o[10] = (float)s_tot[kStatsObsQ - 1];
            o[11] = (float)sc[kQRetSkipped];
            o[12] = (float)sc[kQEpNonfinite];
            o[13] = 0.0f;
            o[14] = 0.0f;
            o[15] = 0.0f;
        }
    }
}

// -------------------------------------------------------------------------------------------------- scaling
// reward_out = clamp(reward * scale, +-clip): one multiply, then two selections (a NaN stays a NaN)
__device__ __forceinline__ float scale_clip(float r, float s, float clip) {
    float x = r * s;
    x = x > clip ? clip : x;
    x = x < -clip ? -clip : x;
    return x;
}

__global__ __launch_bounds__(kStatsThreads) void stats_scale_kernel(const RolloutStatsArgs a, int64_t count, int vec) {
    const Views v = views_of(a.state, a.n);
    const float s = v.ws_scale[0], clip = a.clip_reward;
    const int64_t f = ((int64_t)blockIdx.x * kStatsThreads + threadIdx.x) * 4;
    if (f >= count) return;
    if (vec && f + 3 < count) {
        const f4 r = *reinterpret_cast<const f4*>(a.reward + f);
        f4 o;
        o.x = scale_clip(r.x, s, clip);
        o.y = scale_clip(r.y, s, clip);
        o.z = scale_clip(r.z, s, clip);
        o.w = scale_clip(r.w, s, clip);
        *reinterpret_cast<f4*>(a.reward_out + f) = o;
    } else {
        for (int64_t e = f; e < f + 4 && e < count; ++e) a.reward_out[e] = scale_clip(a.reward[e], s, clip);
    }
}

// hg_rollout_stats_init: a kernel rather than a memset, so that a captured call is a kernel node like the rest
__global__ __launch_bounds__(kStatsThreads) void stats_zero_kernel(uint32_t* __restrict__ state, int64_t words) {
    for (int64_t e = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; e < words; e += (int64_t)gridDim.x * kStatsThreads)
        state[e] = 0u;
}

int64_t blocks_for(int64_t items, int64_t per_block, int64_t cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return b < cap ? b : cap;
}

}  // namespace

hipError_t launch_rollout_stats_zero(void* state, int64_t n, hipStream_t stream) {
    const int64_t words = stats_state_bytes(n) / 4;
    hipLaunchKernelGGL(stats_zero_kernel, dim3((unsigned)blocks_for(words, kStatsThreads, 256)), dim3(kStatsThreads), 0,
                       stream, static_cast<uint32_t*>(state), words);
    return hipGetLastError();
}

hipError_t launch_rollout_stats(const RolloutStatsArgs& a, hipStream_t stream) {
    const int64_t rows = (int64_t)a.nsteps * a.n;
    const int64_t ntiles = (rows + kStatsTileRows - 1) / kStatsTileRows;
    const int nb_scan = (int)blocks_for(a.n, kStatsThreads, kStatsScanBlocksMax);
    const int nb_obs = (int)blocks_for(rows, kStatsTileRows, kStatsObsBlocksMax);
    hipLaunchKernelGGL(stats_pass_kernel, dim3(nb_scan + nb_obs), dim3(kStatsThreads), 0, stream, a, nb_scan, ntiles);
    hipLaunchKernelGGL(stats_finalise_kernel, dim3(1), dim3(kFinalThreads), 0, stream, a, nb_obs, nb_scan);
    if (a.reward_out) {
        const int vec = ((((uintptr_t)a.reward | (uintptr_t)a.reward_out) & 15) == 0) ? 1 : 0;
        hipLaunchKernelGGL(stats_scale_kernel, dim3((unsigned)((rows + 4 * kStatsThreads - 1) / (4 * kStatsThreads))),
                           dim3(kStatsThreads), 0, stream, a, rows, vec);
    }
    return hipGetLastError();
}

}  // namespace hgk
