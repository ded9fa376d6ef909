// Prefill attention for a block of queries over the compact f16 KV cache, both products on the f16 matrix instruction.
//
//   out[r] = softmax(q[r] . K[t] / sqrt(headDim)) . V[t],  t = 0 .. pos0 + r,  r = 0 .. rows - 1, per head (head h reads KV head h / R)
//
// attention_block_kernel<HD, _Float16> (attention_block.hip) widens every half and runs both products on v_mfma_f32_16x16x4_f32: 64
// matrix instructions per 16 keys and query tile at headDim 128.  The cache already holds what v_mfma_f32_16x16x32_f16 takes -- eight
// times the k depth per issue -- but q and the probabilities are f32, and rounding them to half once misses the f32 bar by a factor
// of 18.  So each f32 operand x is SPLIT, hi = f16(x), lo = f16(x - hi), x ~ hi + lo to 2^-22, and every product is issued twice, once
// per part: K and V are exact halves, every half x half product is exact in f32 and the sums are f32.  16 matrix instructions per 16
// keys at headDim 128.  The same bar as the f32 kernel (tests/test_gpu_attention_flash.py: within_bar against float64).
//
// Geometry: grid (numHeads, ceil(rows / 16)), kFaWaves waves per workgroup, a workgroup is one head and 16 queries.  Key tiles are 32
// keys on ABSOLUTE multiples of 32 from token 0; tile t belongs to wave t % kFaWaves, a wave takes its tiles in ascending order with
// its own (m, l, acc), the states merge through LDS in the order w = 0, 1, ...  No workgroup barrier inside the key loop.
//
// Lane l = 16 g + c.  v_mfma_f32_16x16x32_f16: A lane = row c, k = 8 g .. 8 g + 7; B lane = column c, the same k; D lane = rows
// 4 g + i (registers i = 0 .. 3) of column c.
//   S^T = K . Q^T   A = K straight from global memory: row c of the tile's half hf (0 / 1) is key 8 (c / 4) + 4 hf + (c % 4), so D
//                   register i of half hf is key 8 g + 4 hf + i of query c: the two result tiles leave a lane holding keys 8 g ..
//                   8 g + 7 of ONE query, which is the B operand of the second product as it stands -- no lane movement, no LDS.
//                   The sum over d runs in a permuted order (k-step s, lane group g, j = 0 .. 7: d = 64 (s / 2) + 16 g + 8 (s % 2) +
//                   j), K and q alike: a lane's halves of a step are ONE 16-byte load, of two steps 32 contiguous bytes.
//                   B = the query's hi and lo parts, built once per workgroup and held in registers: 2 MFMAs per k-step of 32.
//   out^T += V^T . P^T   B = P's hi and lo parts.  A = V^T (lane: d = 16 dt + c, keys 8 g .. 8 g + 7) -- eight KEYS of one d, while a
//                   cache row is contiguous in d.  So each wave stages its own V tile in LDS with 16-byte stores and reads it back
//                   TRANSPOSED with ds_read_b64_tr_b16 (of the 16 lanes of a group, lane j hands in the address of four halves, lane
//                   i receives element i % 4 of lanes i / 4, 4 + i / 4, 8 + i / 4, 12 + i / 4): lane j points at key 8 g + 4 hf + j /
//                   4, d = 16 dt + 4 (j % 4), lane c gets keys 8 g + 4 hf + 0 .. 3 of d = 16 dt + c; two reads make an operand.
//                   Key kl of the tile sits in LDS row 16 hf + 4 (kl / 8) + kl % 4, hf = (kl / 4) % 2, at a pitch of HD + 16 halves:
//                   the 16 rows one read touches are neighbours and fall on different banks.  D register i of d tile dt is
//                   d = 16 dt + 4 g + i of query c.  Only a wave-local wait stands between the stores and the reads.
// (A wrong lane map moves every element by O(1): the marker test puts a query's whole weight on one key, at each of the eight places
// of a lane's group and in both halves of a tile.)
//
// Pre-scales, exact powers of two, so that no part that matters is a subnormal half (nothing here relies on how the matrix unit
// treats those).  q: row r times 2^e(r), its largest |q| in [2^13, 2^14); undone in f32, in the one factor sc = 2^-e / sqrt(HD).
// The exponent is PER QUERY ROW (and head): a wider one would make a row's bits depend on its neighbours.  p: times 2^14 before the
// split, undone in the final 1 / l.
//
// Softmax: f32, attention_block.hip's rules.  A key that a query may not see is SELECTED out (score -inf, probability an exact 0);
// alpha = 1 while nothing is live; the accumulator's rescale is skipped where no query's max moved (x * 1 is x).
//
// Guarantees, those of the f32 kernel:
//   * An output row's bits are a function of the query, its absolute position and cache rows 0 .. position only -- not of pos0, rows
//     or the row's place in the block (tiles, their waves, the order inside a tile and the merge follow the absolute position; a
//     tile wholly masked for a query leaves its state as it was, bit for bit; a wave that saw no live key merges as an exact zero).
//   * No cache row at or past pos0 + rows and no q row at or past rows is read: a key index there is CLAMPED to the last live row, its
//     score selected out, its probability an exact 0 on a finite V row; a q row there is a zero operand.
//   * No scratch segment and no spills at headDim 64 / 128 / 256.
// The bits are NOT those of effort_attention_block_f16: another order of the sums.
#include "attention_flash_device.h"
#include "attention_split.h"
#include "effort_internal.h"

namespace effort {

template <int HD>
__global__ __launch_bounds__(64 * kFaWaves) void attention_flash16_kernel(const float* __restrict__ qAll, const _Float16* __restrict__ kCache,
                                                                          const _Float16* __restrict__ vCache, uint32_t pos0, uint32_t rows,
                                                                          float* __restrict__ outAll, uint32_t numHeads, uint32_t kvRep) {
    constexpr int NS = HD / 32;                         // k-steps of the first product
    constexpr int ND = HD / 16;                         // d tiles of the second
    constexpr int kVPitch = HD + 16;                    // halves per staged V row
    constexpr int PR = HD / 8, RP = 64 / PR, NP = kFaTile / RP;   // staging: 16-byte pieces per row, rows per pass, passes per tile
    constexpr int kObPitch = HD + 4;                    // floats per merged row (a pitch of HD puts the 16 queries on the same banks)
    constexpr int kStageBytes = kFaWaves * kFaTile * kVPitch * 2;
    static_assert(16 * kObPitch * 4 <= kStageBytes, "the merged accumulator takes the staging buffers' place");
    __shared__ alignas(16) unsigned char lds[kStageBytes];              // the waves' V tiles; after the key loop, ob [query][d]
    __shared__ float ms[kFaWaves][16], ls[kFaWaves][16], invL[16];
    const uint32_t head = blockIdx.x, qt = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, c = lane & 15u;
    const uint32_t limit = pos0 + rows;                 // no cache row at or past it is read
    const uint32_t r = qt * 16u + c, qpos = pos0 + r;   // this lane's query: row of the block, absolute position
    const size_t rowStride = (size_t)numHeads * HD;
    const uint32_t cHeads = numHeads / kvRep, cHead = head / kvRep;     // the cache's heads per row, this head's among them
    const uint32_t lastTile = (pos0 + min(qt * 16u + 15u, rows - 1u)) / kFaTile;
    _Float16* stage = reinterpret_cast<_Float16*>(lds) + (size_t)wave * kFaTile * kVPitch;

    // the query's parts: row r times 2^e, its largest |q| in [2^13, 2^14)
    fa_f16x8 qh[NS], ql[NS];
    float sc;                                           // 2^-e / sqrt(HD): a sum of the first product times sc is a score
    {
        const float* qp = qAll + (size_t)min(r, rows - 1u) * rowStride + head * HD + 16u * g;
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
        sc = ldexpf(1.0f / sqrtf((float)HD), -e);
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                _Float16 hi, lo;
                fa_split(x[s][j >> 2][j & 3] * up, hi, lo);
                qh[s][j] = hi;
                ql[s][j] = lo;
            }
    }
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

    float m = -INFINITY, l = 0.0f;                      // m: of query c, in units of the sums (the same in its four lanes); l: this lane's keys only
    fa_f32x4 acc[ND];
#pragma unroll
    for (int a = 0; a < ND; a++) acc[a] = fa_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    fa_f16x8 kf[2][NS], vf[NP];
    if (wave <= lastTile) ask_k(wave, kf);
    for (uint32_t t = wave; t <= lastTile; t += kFaWaves) {                        // (uniform in the wave)
        ask_v(t, vf);                                                              // in flight under the first product
        fa_f32x4 sh[2], sl[2];                                                     // four chains: the hi and lo parts of both halves
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            sh[hf] = fa_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            sl[hf] = sh[hf];
        }
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                sh[hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[hf][s], qh[s], sh[hf], 0, 0, 0);
                sl[hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[hf][s], ql[s], sl[hf], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
        if (t + kFaWaves <= lastTile) ask_k(t + kFaWaves, kf);                     // the next tile's keys, under the second product
        __builtin_amdgcn_sched_barrier(0);
        // The max is kept in the units of the SUMS (m times sc is the score): a key near the max then loses nothing to the rounding of
        // hi + lo or of the product with sc -- (hi - max) is exact there, and only the small difference meets sc.
        float p[8];
        bool live[8];
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; i++) {                                              // key 8 g + i of the tile: half i / 4, register i % 4
            live[i] = t * kFaTile + 8u * g + i <= qpos;
            tm = fmaxf(tm, live[i] ? sh[i >> 2][i & 3] + sl[i >> 2][i & 3] : -INFINITY);                  // masked by selection
        }
        tm = fmaxf(tm, __shfl_xor(tm, 16));
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        const float mn = fmaxf(m, tm);
        const float alpha = mn == -INFINITY ? 1.0f : expf((m - mn) * sc);         // (no live key yet: the state is zeros, keep it)
        fa_f16x8 ph, pl;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            p[i] = live[i] ? expf(((sh[i >> 2][i & 3] - mn) + sl[i >> 2][i & 3]) * sc) : 0.0f;
            _Float16 hi, lo;
            fa_split(p[i] * kFaPScale, hi, lo);
            ph[i] = hi;
            pl[i] = lo;
        }
        l = l * alpha + (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
        m = mn;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {                          // (x * 1 is x: skipping it where no query's max moved changes no bit)
#pragma unroll
            for (int a = 0; a < ND; a++) acc[a] *= alpha;
        }
        stage_v(vf);
        as_wave_sync();                                                            // the wave's own stores, before its transposed reads
#pragma unroll
        for (int dt = 0; dt < ND; dt++) {
            const fa_f16x4 v0 = fa_read_tr(trBase + 16 * dt), v1 = fa_read_tr(trBase + 16 * kVPitch + 16 * dt);
            const fa_f16x8 vt = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vt, ph, acc[dt], 0, 0, 0);
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vt, pl, acc[dt], 0, 0, 0);
        }
        as_wave_sync();                                                            // the tile is rewritten by the next one
    }

    // merge: the four lanes of a query add their l in the order g = 0 .. 3, then the waves' states in the order w = 0, 1, ...
    const float lq = ((__shfl(l, (int)c) + __shfl(l, (int)c + 16)) + __shfl(l, (int)c + 32)) + __shfl(l, (int)c + 48);
    if (g == 0) { ms[wave][c] = m; ls[wave][c] = lq; }
    __syncthreads();                                     // (every wave is past its key loop: the staging buffers are free)
    float (*ob)[kObPitch] = reinterpret_cast<float (*)[kObPitch]>(lds);
    float M = ms[0][c];                                  // (wave 0 owns tile 0 and key 0 is live for every query: M is finite)
#pragma unroll
    for (int w = 1; w < kFaWaves; w++) M = fmaxf(M, ms[w][c]);
    const float mine = m == -INFINITY ? 0.0f : expf((m - M) * sc);                       // a wave with no live key: an exact zero
    if (wave == 0 && g == 0) {
        float L = 0.0f;
#pragma unroll
        for (int w = 0; w < kFaWaves; w++) L += ls[w][c] * (ms[w][c] == -INFINITY ? 0.0f : expf((ms[w][c] - M) * sc));
        invL[c] = (1.0f / L) * (1.0f / kFaPScale);       // (the probabilities' 2^14 leaves here)
    }
    for (int w = 0; w < kFaWaves; w++) {
        if ((int)wave == w) {
#pragma unroll
            for (int dt = 0; dt < ND; dt++) {
                fa_f32x4* o = reinterpret_cast<fa_f32x4*>(&ob[c][16 * dt + 4 * g]);
                const fa_f32x4 x = acc[dt] * mine;
                *o = w == 0 ? x : *o + x;
            }
        }
        __syncthreads();
    }
    float* out = outAll + (size_t)(qt * 16u) * rowStride + head * HD;
    for (uint32_t idx = tid; idx < 16u * HD; idx += 64u * kFaWaves) {
        const uint32_t qi = idx / HD, d = idx % HD;
        if (qt * 16u + qi < rows) out[(size_t)qi * rowStride + d] = ob[qi][d] * invL[qi];
    }
}

// the caller checked: 1 <= rows <= 64, pos0 + rows <= maxTokens <= 32768, kv16_shape_ok
hipError_t launch_attention_flash_f16(const float* q, const _Float16* kCache, const _Float16* vCache, uint32_t pos0, uint32_t rows, float* out,
                                      uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, hipStream_t st) {
    const dim3 grid(numHeads, (rows + 15u) / 16u), block(64 * kFaWaves);
    const uint32_t kvRep = numHeads / numHeadsKV;
    switch (headDim) {
        case 64: hipLaunchKernelGGL((attention_flash16_kernel<64>), grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads, kvRep); break;
        case 128: hipLaunchKernelGGL((attention_flash16_kernel<128>), grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads, kvRep); break;
        case 256: hipLaunchKernelGGL((attention_flash16_kernel<256>), grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads, kvRep); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace effort
