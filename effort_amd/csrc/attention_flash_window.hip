// Prefill attention for a block of queries over the ROLLING f16 KV cache with a sliding window, both products on the f16 matrix
// instruction: attention_flash16_kernel's arithmetic (attention_flash16.hip) on attention_block_window_kernel's operands (kv_window.hip).
//
//   out[r] = softmax(q[r] . K[t] / sqrt(headDim)) . V[t],  t = lo(pos0 + r) .. pos0 + r,  lo(p) = max(0, p + 1 - window),  r = 0 .. rows - 1,
//   per head (head h reads KV head h / R); K, V: _Float16 [ringRows][numHeadsKV][headDim], token t in row t % ringRows.
//
// Arithmetic, lane maps, pre-scales and softmax are those of attention_flash16.hip, whose header describes them: S^T = K . Q^T and
// out^T += V^T . P^T on v_mfma_f32_16x16x32_f16, q split hi / lo after the per-row power-of-two pre-scale and p after 2^14, K and V
// exact operands, f32 sums, the running max in units of the raw sums, four waves with their own (m, l, acc), V staged per wave in LDS
// and read back with ds_read_b64_tr_b16, no workgroup barrier in the key loop.  What differs:
//
//   walk     Grid (numHeads, ceil(rows / 16)); key tiles of 32 on ABSOLUTE multiples of 32, tile t on wave t % 4.  A workgroup starts
//            at the tile that holds the lower bound of its FIRST query, lo = lo(pos0 + 16 qt), firstTile = lo / 32, and a wave at the
//            first t >= firstTile with t % 4 == wave: past the window a query tile walks about (window + 16) / 32 tiles wherever it is.
//   mask     live = qlo <= key <= qpos with qlo = lo(qpos) per query, by selection: a masked key's probability is an exact 0, a tile
//            wholly masked for a query leaves its (m, l, acc) bit for bit (alpha = 1, p = 0), a wave with no live key merges as an
//            exact zero.  No wave is known to hold a live key of every query (tile firstTile may be masked for the later ones), so
//            the merge takes its max over all four waves' m: a query's own key is live in some wave's tile.
//   rows     ringRows need not be a multiple of 32: the wrap can fall INSIDE a tile and then cuts through the permuted K rows
//            (kRow = 8 (c / 4) + 4 hf + c % 4) and through the V staging passes.  Per tile ONE wave-uniform remainder (ring_tile_at,
//            kv16_device.h: the row of the tile's first live key), then every key of either map goes through ring_tile::row on its own:
//            clamp, add, one compare-subtract.  The remainder of tile t + 4 is taken with its K prefetch and kept for its V loads.
//   reads    Key indices are clamped into lo .. pos0 + rows - 1 before the ring map: lastKey - lo <= window + rows - 2 < ringRows
//            (kv_window_shape_ok), every clamped key a token the ring holds.  No other ring row and no q row at or past rows is read.
//
// Guarantees:
//   * While pos0 + rows <= window (so lo = qlo = 0, ringRows > every key, row = key) every expression has the value it has in
//     attention_flash16_kernel: an output row has effort_attention_flash_f16's bits for the same q, K and V on a plain cache.
//   * At every position an output row's bits are a function of the query, its absolute position, window and the ring's contents for
//     its window -- not of pos0, rows, the row's place in the block or ringRows: tiles, their waves, the order inside a tile and the
//     merge follow absolute positions, and the tiles below a query's own first live one are no-ops on its state.
//   * No scratch segment and no spills at headDim 64 / 128 / 256.
#include "attention_flash_device.h"
#include "attention_split.h"
#include "effort_internal.h"
#include "kv16_device.h"

namespace effort {

template <int HD>
__global__ __launch_bounds__(64 * kFaWaves) void attention_flash_window_kernel(const float* __restrict__ qAll, const _Float16* __restrict__ kRing,
                                                                               const _Float16* __restrict__ vRing, uint32_t pos0, uint32_t rows,
                                                                               float* __restrict__ outAll, uint32_t numHeads, uint32_t kvRep,
                                                                               uint32_t ringRows, uint32_t window) {
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
    const uint32_t lastKey = pos0 + rows - 1u;          // no token past it is read
    const uint32_t r = qt * 16u + c, qpos = pos0 + r;   // this lane's query: row of the block, absolute position
    const uint32_t qlo = attention_window_lo(qpos, window);                       // ... and the first key it sees
    const size_t rowStride = (size_t)numHeads * HD;
    const uint32_t cHeads = numHeads / kvRep, cHead = head / kvRep;               // the ring's heads per row, this head's among them
    const uint32_t lo = attention_window_lo(pos0 + qt * 16u, window);             // the first key ANY query of the tile sees
    const uint32_t firstTile = lo / kFaTile, lastTile = (pos0 + min(qt * 16u + 15u, rows - 1u)) / kFaTile;
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
                _Float16 hi, lo16;
                fa_split(x[s][j >> 2][j & 3] * up, hi, lo16);
                qh[s][j] = hi;
                ql[s][j] = lo16;
            }
    }
    // this lane's two key rows of a tile (A rows c of the halves 0 / 1): each through the ring on its own
    const uint32_t kRow = 8u * (c >> 2) + (c & 3u);
    auto ask_k = [&](uint32_t t, const ring_tile& ring, fa_f16x8 (&k)[2][NS]) {
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            const _Float16* kp = kRing + ((size_t)ring.row(t * kFaTile + kRow + 4u * hf) * cHeads + cHead) * HD + 16u * g;
#pragma unroll
            for (int s = 0; s < NS; s++) k[hf][s] = *reinterpret_cast<const fa_f16x8*>(kp + 64 * (s >> 1) + 8 * (s & 1));
        }
    };
    // the V tile, row-contiguous: pass u takes keys u RP .. u RP + RP - 1 of the tile, a lane one 16-byte piece of its key's ring row
    const uint32_t vPiece = lane % PR, vRow = lane / PR;
    auto ask_v = [&](uint32_t t, const ring_tile& ring, fa_f16x8 (&v)[NP]) {
#pragma unroll
        for (int u = 0; u < NP; u++)
            v[u] = *reinterpret_cast<const fa_f16x8*>(vRing + ((size_t)ring.row(t * kFaTile + u * RP + vRow) * cHeads + cHead) * HD + 8u * vPiece);
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
    const uint32_t tBegin = firstTile + ((wave + 4u - (firstTile & 3u)) & 3u);    // this wave's first tile: tile t belongs to wave t % 4
    ring_tile ring = ring_tile_at(tBegin * kFaTile, lo, lastKey, ringRows);       // of the tile whose keys are in kf
    if (tBegin <= lastTile) ask_k(tBegin, ring, kf);
    for (uint32_t t = tBegin; t <= lastTile; t += kFaWaves) {                      // (uniform in the wave)
        ask_v(t, ring, vf);                                                        // in flight under the first product
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
        if (t + kFaWaves <= lastTile) {                                            // the next tile's keys, under the second product
            ring = ring_tile_at((t + kFaWaves) * kFaTile, lo, lastKey, ringRows);
            ask_k(t + kFaWaves, ring, kf);
        }
        __builtin_amdgcn_sched_barrier(0);
        // The max is kept in the units of the SUMS (m times sc is the score): a key near the max then loses nothing to the rounding of
        // hi + lo or of the product with sc -- (hi - max) is exact there, and only the small difference meets sc.
        float p[8];
        bool live[8];
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; i++) {                                              // key 8 g + i of the tile: half i / 4, register i % 4
            const uint32_t key = t * kFaTile + 8u * g + i;
            live[i] = key >= qlo && key <= qpos;
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
            _Float16 hi, lo16;
            fa_split(p[i] * kFaPScale, hi, lo16);
            ph[i] = hi;
            pl[i] = lo16;
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
    float M = ms[0][c];                                  // (a query's own key is live in a tile of the walk: M is finite for every row < rows)
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

// the caller checked: kv_window_shape_ok with rows, 1 <= rows <= 64, pos0 + rows <= kWindowMaxPos
hipError_t launch_attention_flash_window(const float* q, const _Float16* kRing, const _Float16* vRing, uint32_t pos0, uint32_t rows, float* out,
                                         uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t ringRows, uint32_t window,
                                         hipStream_t st) {
    const dim3 grid(numHeads, (rows + 15u) / 16u), block(64 * kFaWaves);
    const uint32_t kvRep = numHeads / numHeadsKV;
    switch (headDim) {
        case 64: hipLaunchKernelGGL((attention_flash_window_kernel<64>), grid, block, 0, st, q, kRing, vRing, pos0, rows, out, numHeads, kvRep, ringRows, window); break;
        case 128: hipLaunchKernelGGL((attention_flash_window_kernel<128>), grid, block, 0, st, q, kRing, vRing, pos0, rows, out, numHeads, kvRep, ringRows, window); break;
        case 256: hipLaunchKernelGGL((attention_flash_window_kernel<256>), grid, block, 0, st, q, kRing, vRing, pos0, rows, out, numHeads, kvRep, ringRows, window); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace effort
