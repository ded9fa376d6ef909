// Prefill attention for a block of up to 256 queries over the compact f16 KV cache, the query heads of a GQA group sharing each K / V
// tile: attention_flash16_kernel's arithmetic PER HEAD (attention_flash16.hip, whose header describes the lane maps, the hi / lo split,
// the pre-scales and the softmax) with a geometry of its own.
//
//   out[r] = softmax(q[r] . K[t] / sqrt(headDim)) . V[t],  t = 0 .. pos0 + r,  r = 0 .. rows - 1, per head (head h reads KV head h / R)
//
// attention_flash16_kernel's workgroup is one query head and 16 queries: the R = numHeads / numHeadsKV heads of a group fetch the same K
// and V tiles, stage and transpose the same V tile and compute the same causal mask, once each.  Here a workgroup is one KV head, 16
// query positions and HPW of that group's query heads, HPW = min(R, 512 / HD); where R > HPW the R / HPW head groups are part of the
// grid: grid (numHeadsKV * R / HPW, ceil(rows / 16)), kFaWaves waves.  Workgroup x serves heads x HPW .. x HPW + HPW - 1.
//
// Tile ownership is attention_flash16_kernel's: 32 keys on absolute multiples of 32, tile t on wave t % kFaWaves, ascending.  The wave
// that owns a tile
//   * loads its K fragments once from global memory straight into the A operand (the same rows kRow, hf),
//   * stages its V tile once (16-byte stores) and reads every transposed fragment once (ds_read_b64_tr_b16, the wave-local wait only),
//   * computes the mask live[i] once (it depends on the position alone),
// and uses them for all HPW heads.  It owns HPW independent online-softmax states (m, l) and HPW accumulators.  No workgroup barrier
// inside the key loop.
//
// Operand placement.
//   q parts   (qh, ql per head and k-step, sc per head and row) are built ONCE per workgroup -- head j by wave j % kFaWaves, with the
//             per-row, per-head exponent -- and kept in LDS in B-operand order [head][k-step][part][lane]: the lane that needs a
//             fragment reads the 16 bytes at its own lane index, a wave's read is 1024 contiguous bytes, no two lanes of a quarter wave
//             share a bank.  HPW * HD * 64 bytes: 32 KB where HPW * HD = 512.  In registers they would be 128 VGPRs at headDim 128.
//   first product   head by head: four chains (sh, sl x the two halves) of NS steps, then that head's softmax step, which leaves the
//             probabilities' parts ph[j], pl[j] (8 VGPRs per head) and has rescaled acc[j].  The sums of a head are not kept: 16
//             VGPRs of them are live at a time.  Once the last head's first product is issued kf is free and the next tile's K is asked
//             for.
//   second product  d tile by d tile: ONE transposed V^T fragment (two reads, 4 VGPRs) feeds the two matrix instructions of every
//             head, acc[j][dt] += V^T . ph[j], += V^T . pl[j].  Each fragment is read once per tile and none is held across d tiles (the
//             whole tile's fragments would be 32 VGPRs at headDim 128, 64 at 256); the HPW heads' instructions are independent chains.
//   accumulators    HPW * HD / 4 = 128 f32 registers where HPW * HD = 512.  __launch_bounds__(256): one workgroup's waves have the
//             whole register file, the compiler places what does not fit 256 VGPRs in AGPRs.
//   LDS       q parts + kFaWaves V tiles (36 KB at headDim 128); after the key loop the merged accumulators ob [head][query][d] take
//             the place of both.
//
// Merge, per head: attention_flash16_kernel's -- a query's four lanes add their l in the order g = 0 .. 3, M is the max over all waves,
// the waves' states are added in the order w = 0, 1, ..., invL carries the probabilities' 2^-14.
//
// Guarantees:
//   * Output row r, head h has BIT FOR BIT the bits effort_attention_flash_f16 writes for the same q row, position and cache.  Per head
//     the order of every sum, the tile-to-wave map, the selection of masked keys and the merge order are that kernel's; only where an
//     operand comes from differs (tests/test_gpu_attention_flash_group.py compares the bits on every case).
//   * Hence an output row's bits are a function of the query, its absolute position and cache rows 0 .. pos0 + r alone.
//   * No cache row at or past pos0 + rows and no q row at or past rows is read: a key or V index there is CLAMPED to the last live row
//     and selected out, a q row there is a zero operand.  Nothing outside out[0 .. rows) is written.
//   * No scratch segment and no spills at any instantiation.  The compiler's resource report for gfx950 (-Rpass-analysis=kernel-
//     resource-usage), VGPRs / AGPRs / LDS bytes / waves per SIMD:
//         <HD, HPW> VGPR  AGPR    LDS   waves per SIMD
//         < 64, 1>  108    16  25216   4
//         < 64, 2>  118    48  29952   3
//         < 64, 4>  160    80  39424   2
//         < 64, 8>  238   144  58368   1
//         <128, 1>  154    32  45696   2
//         <128, 2>  184    80  54528   1
//         <128, 4>  255   144  72192   1
//         <256, 1>  237    80  86656   1
//         <256, 2>  256   196 103680   1
#include "attention_flash_device.h"
#include "attention_split.h"
#include "effort_internal.h"

namespace effort {

template <int HD, int HPW>
__global__ __launch_bounds__(64 * kFaWaves) void attention_flash_group_kernel(const float* __restrict__ qAll, const _Float16* __restrict__ kCache,
                                                                              const _Float16* __restrict__ vCache, uint32_t pos0, uint32_t rows,
                                                                              float* __restrict__ outAll, uint32_t numHeads, uint32_t kvRep) {
    constexpr int NS = HD / 32;                         // k-steps of the first product
    constexpr int ND = HD / 16;                         // d tiles of the second
    constexpr int kVPitch = HD + 16;                    // halves per staged V row
    constexpr int PR = HD / 8, RP = 64 / PR, NP = kFaTile / RP;   // staging: 16-byte pieces per row, rows per pass, passes per tile
    constexpr int kObPitch = HD + 4;                    // floats per merged row
    constexpr int kQBytes = HPW * NS * 2 * 64 * 16;     // the q parts [head][k-step][hi / lo][lane], one fa_f16x8 each
    constexpr int kStageBytes = kFaWaves * kFaTile * kVPitch * 2;
    static_assert(HPW * 16 * kObPitch * 4 <= kQBytes + kStageBytes, "the merged accumulators take the q parts' and the staging buffers' place");
    __shared__ alignas(16) unsigned char lds[kQBytes + kStageBytes];    // q parts, the waves' V tiles; after the key loop, ob [head][query][d]
    __shared__ float scs[HPW][16], ms[kFaWaves][HPW][16], ls[kFaWaves][HPW][16], invL[HPW][16];
    const uint32_t head0 = blockIdx.x * HPW, qt = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, c = lane & 15u;
    const uint32_t limit = pos0 + rows;                 // no cache row at or past it is read
    const uint32_t r = qt * 16u + c, qpos = pos0 + r;   // this lane's query: row of the block, absolute position
    const size_t rowStride = (size_t)numHeads * HD;
    const uint32_t cHeads = numHeads / kvRep, cHead = head0 / kvRep;    // the cache's heads per row, this workgroup's among them
    const uint32_t lastTile = (pos0 + min(qt * 16u + 15u, rows - 1u)) / kFaTile;
    fa_f16x8* qParts = reinterpret_cast<fa_f16x8*>(lds);
    _Float16* stage = reinterpret_cast<_Float16*>(lds + kQBytes) + (size_t)wave * kFaTile * kVPitch;

    // the queries' parts, head j by wave j % kFaWaves: row r times 2^e, its largest |q| in [2^13, 2^14)
    for (uint32_t j = wave; j < (uint32_t)HPW; j += kFaWaves) {
        const float* qp = qAll + (size_t)min(r, rows - 1u) * rowStride + (head0 + j) * HD + 16u * g;
        fa_f32x4 x[NS][2];
        float amax = 0.0f;
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const fa_f32x4 y = *reinterpret_cast<const fa_f32x4*>(qp + 64 * (s >> 1) + 8 * (s & 1) + 4 * hh);
                x[s][hh] = r < rows ? y : fa_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int e = 0; e < 4; e++) amax = fmaxf(amax, fabsf(x[s][hh][e]));
            }
        amax = fmaxf(amax, __shfl_xor(amax, 16));
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        // (a zero or non-finite row keeps e = 0; e is held to +-100 so that 2^e and 2^-e are normal floats)
        int e = amax > 0.0f && amax < INFINITY ? 13 - ilogbf(amax) : 0;
        e = max(-100, min(100, e));
        const float up = ldexpf(1.0f, e);
        if (g == 0) scs[j][c] = ldexpf(1.0f / sqrtf((float)HD), -e);   // 2^-e / sqrt(HD): a sum of the first product times it is a score
#pragma unroll
        for (int s = 0; s < NS; s++) {
            fa_f16x8 qh, ql;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                _Float16 hi, lo;
                fa_split(x[s][i >> 2][i & 3] * up, hi, lo);
                qh[i] = hi;
                ql[i] = lo;
            }
            qParts[((j * NS + s) * 2 + 0) * 64 + lane] = qh;
            qParts[((j * NS + s) * 2 + 1) * 64 + lane] = ql;
        }
    }
    __syncthreads();
    float sc[HPW];
#pragma unroll
    for (int j = 0; j < HPW; j++) sc[j] = scs[j][c];

    // this lane's two key rows of tile t (A rows c of the halves 0 / 1), clamped
    const uint32_t kRow = 8u * (c >> 2) + (c & 3u);
    auto ask_k = [&](uint32_t t, fa_f16x8 (&k)[2][NS]) {
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            const _Float16* kp = kCache + ((size_t)min(t * kFaTile + kRow + 4u * hf, limit - 1u) * cHeads + cHead) * HD + 16u * g;
#pragma unroll
            for (int s = 0; s < NS; s++) k[hf][s] = *reinterpret_cast<const fa_f16x8*>(kp + 64 * (s >> 1) + 8 * (s & 1));
        }
    };
    // the V tile, row-contiguous: pass u takes rows u RP .. u RP + RP - 1, a lane one 16-byte piece
    const uint32_t vPiece = lane % PR, vRow = lane / PR;
    auto ask_v = [&](uint32_t t, fa_f16x8 (&v)[NP]) {
#pragma unroll
        for (int u = 0; u < NP; u++)
            v[u] = *reinterpret_cast<const fa_f16x8*>(vCache + ((size_t)min(t * kFaTile + u * RP + vRow, limit - 1u) * cHeads + cHead) * HD + 8u * vPiece);
    };
    auto stage_v = [&](const fa_f16x8 (&v)[NP]) {
#pragma unroll
        for (int u = 0; u < NP; u++) {
            const uint32_t kl = u * RP + vRow, row = 16u * ((kl >> 2) & 1u) + 4u * (kl >> 3) + (kl & 3u);
            *reinterpret_cast<fa_f16x8*>(stage + row * kVPitch + 8u * vPiece) = v[u];
        }
    };
    // the transposed read's address of this lane: row 4 g + c / 4 (+ 16 hf), d = 4 (c % 4) (+ 16 dt)
    const _Float16* trBase = stage + (4u * g + (c >> 2)) * kVPitch + 4u * (c & 3u);

    float m[HPW], l[HPW];                               // per head.  m: of query c, in units of the sums; l: this lane's keys only
    fa_f32x4 acc[HPW][ND];
#pragma unroll
    for (int j = 0; j < HPW; j++) {
        m[j] = -INFINITY;
        l[j] = 0.0f;
#pragma unroll
        for (int a = 0; a < ND; a++) acc[j][a] = fa_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    fa_f16x8 kf[2][NS], vf[NP];
    if (wave <= lastTile) ask_k(wave, kf);
    for (uint32_t t = wave; t <= lastTile; t += kFaWaves) {                        // (uniform in the wave)
        ask_v(t, vf);                                                              // in flight under the first products
        bool live[8];                                                              // key 8 g + i of the tile, the same for every head
#pragma unroll
        for (int i = 0; i < 8; i++) live[i] = t * kFaTile + 8u * g + i <= qpos;
        fa_f16x8 ph[HPW], pl[HPW];
#pragma unroll
        for (int j = 0; j < HPW; j++) {
            fa_f32x4 sh[2], sl[2];                                                 // four chains: the hi and lo parts of both halves
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                sh[hf] = fa_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                sl[hf] = sh[hf];
            }
#pragma unroll
            for (int s = 0; s < NS; s++) {
                const fa_f16x8 qh = qParts[((j * NS + s) * 2 + 0) * 64 + lane], ql = qParts[((j * NS + s) * 2 + 1) * 64 + lane];
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    sh[hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[hf][s], qh, sh[hf], 0, 0, 0);
                    sl[hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[hf][s], ql, sl[hf], 0, 0, 0);
                }
            }
            // attention_flash16_kernel's softmax step on this head's state (the max in the units of the SUMS, masked by selection)
            float p[8];
            float tm = -INFINITY;
#pragma unroll
            for (int i = 0; i < 8; i++) tm = fmaxf(tm, live[i] ? sh[i >> 2][i & 3] + sl[i >> 2][i & 3] : -INFINITY);
            tm = fmaxf(tm, __shfl_xor(tm, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float mn = fmaxf(m[j], tm);
            const float alpha = mn == -INFINITY ? 1.0f : expf((m[j] - mn) * sc[j]);      // (no live key yet: the state is zeros, keep it)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                p[i] = live[i] ? expf(((sh[i >> 2][i & 3] - mn) + sl[i >> 2][i & 3]) * sc[j]) : 0.0f;
                _Float16 hi, lo;
                fa_split(p[i] * kFaPScale, hi, lo);
                ph[j][i] = hi;
                pl[j][i] = lo;
            }
            l[j] = l[j] * alpha + (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
            m[j] = mn;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {                      // (x * 1 is x: skipping it where no query's max moved changes no bit)
#pragma unroll
                for (int a = 0; a < ND; a++) acc[j][a] *= alpha;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t + kFaWaves <= lastTile) ask_k(t + kFaWaves, kf);                     // the next tile's keys, under the second products
        __builtin_amdgcn_sched_barrier(0);
        stage_v(vf);
        as_wave_sync();                                                            // the wave's own stores, before its transposed reads
#pragma unroll
        for (int dt = 0; dt < ND; dt++) {                                          // one fragment, every head
            const fa_f16x4 v0 = fa_read_tr(trBase + 16 * dt), v1 = fa_read_tr(trBase + 16 * kVPitch + 16 * dt);
            const fa_f16x8 vt = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int j = 0; j < HPW; j++) {
                acc[j][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vt, ph[j], acc[j][dt], 0, 0, 0);
                acc[j][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vt, pl[j], acc[j][dt], 0, 0, 0);
            }
        }
        as_wave_sync();                                                            // the tile is rewritten by the next one
    }

    // merge, per head: the four lanes of a query add their l in the order g = 0 .. 3, then the waves' states in the order w = 0, 1, ...
#pragma unroll
    for (int j = 0; j < HPW; j++) {
        const float lq = ((__shfl(l[j], (int)c) + __shfl(l[j], (int)c + 16)) + __shfl(l[j], (int)c + 32)) + __shfl(l[j], (int)c + 48);
        if (g == 0) { ms[wave][j][c] = m[j]; ls[wave][j][c] = lq; }
    }
    __syncthreads();                                     // (every wave is past its key loop: the q parts and the staging buffers are free)
    float (*ob)[16][kObPitch] = reinterpret_cast<float (*)[16][kObPitch]>(lds);
    float mine[HPW];
#pragma unroll
    for (int j = 0; j < HPW; j++) {
        float M = ms[0][j][c];                           // (wave 0 owns tile 0 and key 0 is live for every query: M is finite)
#pragma unroll
        for (int w = 1; w < kFaWaves; w++) M = fmaxf(M, ms[w][j][c]);
        mine[j] = m[j] == -INFINITY ? 0.0f : expf((m[j] - M) * sc[j]);                   // a wave with no live key: an exact zero
        if (wave == 0 && g == 0) {
            float L = 0.0f;
#pragma unroll
            for (int w = 0; w < kFaWaves; w++) L += ls[w][j][c] * (ms[w][j][c] == -INFINITY ? 0.0f : expf((ms[w][j][c] - M) * sc[j]));
            invL[j][c] = (1.0f / L) * (1.0f / kFaPScale);                               // (the probabilities' 2^14 leaves here)
        }
    }
    for (int w = 0; w < kFaWaves; w++) {
        if ((int)wave == w) {
#pragma unroll
            for (int j = 0; j < HPW; j++)
#pragma unroll
                for (int dt = 0; dt < ND; dt++) {
                    fa_f32x4* o = reinterpret_cast<fa_f32x4*>(&ob[j][c][16 * dt + 4 * g]);
                    const fa_f32x4 x = acc[j][dt] * mine[j];
                    *o = w == 0 ? x : *o + x;
                }
        }
        __syncthreads();
    }
    // a row's HPW heads are HPW * HD neighbouring floats of out
    float* out = outAll + (size_t)(qt * 16u) * rowStride + (size_t)head0 * HD;
    for (uint32_t idx = tid; idx < 16u * HPW * HD; idx += 64u * kFaWaves) {
        const uint32_t qi = idx / (HPW * HD), j = idx / HD % HPW, d = idx % HD;
        if (qt * 16u + qi < rows) out[(size_t)qi * rowStride + j * HD + d] = ob[j][qi][d] * invL[j][qi];
    }
}

template <int HD, int HPW>
static void launch_group(const float* q, const _Float16* kCache, const _Float16* vCache, uint32_t pos0, uint32_t rows, float* out, uint32_t numHeads,
                         uint32_t kvRep, hipStream_t st) {
    const dim3 grid(numHeads / HPW, (rows + 15u) / 16u), block(64 * kFaWaves);
    hipLaunchKernelGGL((attention_flash_group_kernel<HD, HPW>), grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads, kvRep);
}

// the caller checked: 1 <= rows <= 256, pos0 + rows <= maxTokens <= 32768, kv16_shape_ok (headDim 64 / 128 / 256, R 1 / 2 / 4 / 8)
hipError_t launch_attention_flash_group_f16(const float* q, const _Float16* kCache, const _Float16* vCache, uint32_t pos0, uint32_t rows, float* out,
                                            uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, hipStream_t st) {
    const uint32_t kvRep = numHeads / numHeadsKV, hpw = min(kvRep, 512u / headDim);
#define EFFORT_GROUP_CASE(HD, HPW) \
    case HD * 16 + HPW: launch_group<HD, HPW>(q, kCache, vCache, pos0, rows, out, numHeads, kvRep, st); break;
    switch (headDim * 16u + hpw) {
        EFFORT_GROUP_CASE(64, 1) EFFORT_GROUP_CASE(64, 2) EFFORT_GROUP_CASE(64, 4) EFFORT_GROUP_CASE(64, 8)
        EFFORT_GROUP_CASE(128, 1) EFFORT_GROUP_CASE(128, 2) EFFORT_GROUP_CASE(128, 4)
        EFFORT_GROUP_CASE(256, 1) EFFORT_GROUP_CASE(256, 2)
        default: return hipErrorInvalidValue;
    }
#undef EFFORT_GROUP_CASE
    return hipGetLastError();
}

}  // namespace effort
