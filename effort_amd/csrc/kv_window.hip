// Sliding-window attention over a ROLLING f16 KV cache: the writers, the split decode attention and the block (prefill) attention.
//
//   K, V: _Float16 [ringRows][numHeadsKV][headDim], token t in row t % ringRows; KV head g serves query heads g R .. g R + R - 1 (the
//   compact format of kv16.hip with a ring in place of the token axis).  The query at position p sees tokens lo(p) .. p,
//   lo(p) = max(0, p + 1 - window): `window` keys including its own.  ringRows >= window holds them for a token step; a block of `rows`
//   tokens needs ringRows >= window + rows - 1 (its last write lands in the slot of token pos0 + rows - 1 - ringRows, its first query
//   still needs token pos0 + 1 - window).  So a step's attention costs what it costs at position window - 1 for ever, the cache is
//   window + 64 rows whatever the context, and positions run to 1048576 (exact as f32 in the rope).
//
// Writers.  rope_kv_ring_kernel / rope_kv_rows_ring_kernel: rope_kv_f16_row (kv16_device.h) with the slot at row pos % ringRows -- the
// f32 rope, ONE conversion, overflow to +-inf, q_out's bits.  The token form writes nothing at *pos >= maxPos and raises status bit 0.
//
// attention_window_kernel is attention_split_f16_kernel (kv16.hip) with a window for a key range: its grid (numHeadsKV, S), its waves,
// tiles of 64 keys, lane maps, online softmax, partial states and scratch, merged by attention_merge_kernel; no atomics, flags or waiting.
//   tiles    stay on ABSOLUTE multiples of 64 counted from token 0, tile t on wave t % 4.  The live ones are lo / 64 .. pos / 64 (at most
//            window / 64 + 1); attention_window_tiles (attention_split.h) deals them to the splits, from *pos on the device.
//   keys     a key below lo or above pos is CLAMPED to a live token and its score SELECTED to -inf: its probability is an exact 0 on a
//            live V row, never 0 * something computed from a dead row.
//   rows     a tile may straddle the ring's wrap (ringRows need not be a multiple of 64).  Per tile, ONE wave-uniform remainder: the row
//            of the tile's first live key, first = max(64 t, lo).  A clamped key is first + off with off <= min(63, window - 1) <
//            ringRows, so its row is row0 + off, minus ringRows where that reaches it: one compare-subtract per key, no division.
// Below the window (pos < window, ringRows > pos) every expression has the value it has in attention_split_f16_kernel: the same bits.
//
// attention_block_window_kernel is attention_block_kernel (attention_block.hip) on this format with a per-query lower bound: a workgroup
// is one head and 16 queries, key tiles of 16 on absolute multiples of 16, tile t on wave t % 4, flash-style online softmax, both
// products on v_mfma_f32_16x16x4_f32 with the halves widened in registers.  It starts at tile lo(first query) / 16; the mask is
// lo(q) <= key <= qpos by selection, so a tile wholly masked for a query leaves that query's state as it was (alpha = 1, p = 0) and an
// output row's bits are a function of the query, its absolute position, the window and the tokens in its window -- not of pos0, rows or
// the chunk.  Key indices are clamped into [lo(first query), pos0 + rows - 1], all of them tokens the ring holds; rows as above.
//
// Reads: q, *pos, the ring rows of the tokens in the call's window (every other row may hold NaN).  Writes: the scratch / out only.
#include "attention_split.h"
#include "effort_internal.h"
#include "kv16_device.h"

namespace effort {

// ---- writers
__global__ void rope_kv_ring_kernel(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                                    float* __restrict__ qOut, _Float16* __restrict__ kRing, _Float16* __restrict__ vRing,
                                    const uint32_t* __restrict__ posPtr, uint32_t numHeads, uint32_t numHeadsKV, float logBase,
                                    uint32_t ringRows, uint32_t maxPos, int* __restrict__ status) {
    const uint32_t pos = posPtr[0];
    if (pos >= maxPos) {                               // past the last position: nothing is written, the context's status word says so
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    rope_kv_f16_row(xq, xk, xv, qOut, kRing, vRing, pos, pos % ringRows, blockIdx.x, numHeads, numHeadsKV, logBase);
}
// row blockIdx.y of the block at position pos0 + blockIdx.y (no guard: the host checked the range)
__global__ void rope_kv_rows_ring_kernel(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                                         float* __restrict__ qOut, _Float16* __restrict__ kRing, _Float16* __restrict__ vRing,
                                         uint32_t pos0, uint32_t numHeads, uint32_t numHeadsKV, float logBase, uint32_t ringRows) {
    const size_t qOff = (size_t)blockIdx.y * numHeads * blockDim.x, kvOff = (size_t)blockIdx.y * numHeadsKV * blockDim.x;
    const uint32_t pos = pos0 + blockIdx.y;
    rope_kv_f16_row(xq + qOff, xk + kvOff, xv + kvOff, qOut + qOff, kRing, vRing, pos, pos % ringRows, blockIdx.x, numHeads, numHeadsKV,
                    logBase);
}

// ---- the windowed split decode attention (the ring rows of a key tile: ring_tile, kv16_device.h)
template <int HD, int R>
__global__ __launch_bounds__(64 * kAsWaves) void attention_window_kernel(const float* __restrict__ q, const _Float16* __restrict__ kRing,
                                                                         const _Float16* __restrict__ vRing, const uint32_t* __restrict__ posPtr,
                                                                         float* __restrict__ scratch, uint32_t numHeads, uint32_t ringRows,
                                                                         uint32_t window) {
    constexpr int LPK = HD / 8, KPP = 64 / LPK, KB = LPK < 16 ? LPK : 16, NKB = LPK / KB;   // lanes per key, keys per pass; a tile is LPK passes, in batches of KB
    constexpr int VD = R <= 4 ? 8 : 4, VW = VD / 2;                              // values: dims per lane, words per load
    constexpr int LPV = HD / VD, KPV = 64 / LPV, VB = 64 / VD, NVB = LPV / VB;   // ... a tile is LPV passes, in batches of VB (32 registers)
    __shared__ alignas(16) float sc[kAsWaves][64][R];                            // a wave's strip: scores, then probabilities, of its tile
    __shared__ alignas(16) float ob[kAsWaves][R][HD];
    __shared__ float ms[kAsWaves][R], ls[kAsWaves][R];
    const uint32_t g = blockIdx.x, s = blockIdx.y, S = gridDim.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), head0 = g * R;
    const uint32_t sub = lane % LPK, kk = lane / LPK;                            // scores: this lane's 8 dims, its key of a pass
    const uint32_t dv = (lane % LPV) * VD, kv = lane / LPV;                      // values: this lane's VD dims, its key of a pass
    float* ml = scratch + (size_t)numHeads * S * HD;

    // the queries do not depend on the position: asked for beside it
    float q8[R][8];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const float4* qp = reinterpret_cast<const float4*>(q + (size_t)(head0 + r) * HD + sub * 8u);
        const float4 a = qp[0], b = qp[1];
        q8[r][0] = a.x; q8[r][1] = a.y; q8[r][2] = a.z; q8[r][3] = a.w; q8[r][4] = b.x; q8[r][5] = b.y; q8[r][6] = b.z; q8[r][7] = b.w;
    }
    const uint32_t pos = posPtr[0], lo = attention_window_lo(pos, window);       // the live keys: lo .. pos
    uint32_t t0, t1;
    attention_window_tiles(pos, window, S, s, t0, t1);
    if (t0 >= t1) {                                                              // (uniform) nothing to do: the neutral state
        if (tid < (uint32_t)R) { ml[((size_t)(head0 + tid) * S + s) * 2u] = -INFINITY; ml[((size_t)(head0 + tid) * S + s) * 2u + 1u] = 0.0f; }
        return;
    }
    const size_t rowStride = (size_t)gridDim.x * HD;                             // numHeadsKV heads per row
    const _Float16* kBase = kRing + (size_t)g * HD + sub * 8u;
    const _Float16* vBase = vRing + (size_t)g * HD + dv;
    const float scale = 1.0f / sqrtf((float)HD);

    float m[R], l[R], acc[R][VD];
#pragma unroll
    for (int r = 0; r < R; r++) {
        m[r] = -INFINITY; l[r] = 0.0f;
#pragma unroll
        for (int i = 0; i < VD; i++) acc[r][i] = 0.0f;
    }

    for (uint32_t t = t0 + ((wave + 4u - (t0 & 3u)) & 3u); t < t1; t += kAsWaves) {       // (uniform in the wave)
        const uint32_t key0 = t * kSplitTile;
        const ring_tile ring = ring_tile_at(key0, lo, pos, ringRows);
        uint32_t vw[VB][VW];
#pragma unroll
        for (int kb = 0; kb < NKB; kb++) {
            uint32_t kw[KB][4];
#pragma unroll
            for (int u = 0; u < KB; u++) {
                const uint32_t key = key0 + (uint32_t)(kb * KB + u) * KPP + kk;
                kv_load<4>(kBase + (size_t)ring.row(key) * rowStride, kw[u]);
            }
            if (kb == 0) {
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    const uint32_t key = key0 + (uint32_t)u * KPV + kv;
                    kv_load<VW>(vBase + (size_t)ring.row(key) * rowStride, vw[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < KB; u++) {
                const uint32_t kt = (uint32_t)(kb * KB + u) * KPP + kk;                   // key within the tile
                const bool live = key0 + kt >= lo && key0 + kt <= pos;
                float kf[8];
                kv_widen<4>(kw[u], kf);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    float dot = q8[r][0] * kf[0];
#pragma unroll
                    for (int i = 1; i < 8; i++) dot = fmaf(q8[r][i], kf[i], dot);
                    dot = as_key_sum<LPK>(dot);
                    if (sub == (uint32_t)(LPK - 1)) sc[wave][kt][r] = live ? dot * scale : -INFINITY;   // masked by selection
                }
            }
        }
        as_wave_sync();
        {
            float sv[R];
#pragma unroll
            for (int r = 0; r < R; r++) sv[r] = sc[wave][lane][r];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float mn = fmaxf(m[r], wave_max_f32(sv[r]));
                const float alpha = mn == -INFINITY ? 1.0f : expf(m[r] - mn);
                const float p = sv[r] == -INFINITY ? 0.0f : expf(sv[r] - mn);
                l[r] = l[r] * alpha + wave_sum_f32(p);
                m[r] = mn;
                if (alpha != 1.0f) {                                                      // (uniform; x * 1 is x: skipping it changes no bit)
#pragma unroll
                    for (int i = 0; i < VD; i++) acc[r][i] *= alpha;
                }
                sv[r] = p;
            }
#pragma unroll
            for (int r = 0; r < R; r++) sc[wave][lane][r] = sv[r];
        }
        as_wave_sync();
#pragma unroll
        for (int vb = 0; vb < NVB; vb++) {
            if (vb > 0) {
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    const uint32_t key = key0 + (uint32_t)(vb * VB + u) * KPV + kv;
                    kv_load<VW>(vBase + (size_t)ring.row(key) * rowStride, vw[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < VB; u++) {
                const uint32_t kt = (uint32_t)(vb * VB + u) * KPV + kv;
                float vf[VD];
                kv_widen<VW>(vw[u], vf);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float p = sc[wave][kt][r];                                      // (a clamped key: an exact 0 on a live row)
#pragma unroll
                    for (int i = 0; i < VD; i++) acc[r][i] = fmaf(p, vf[i], acc[r][i]);
                }
            }
        }
        as_wave_sync();                                                                   // the strip is rewritten by the next tile
    }

    // the key phases of a wave share m: their accumulators add up (one fixed tree); then the waves' states through LDS, in wave order
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
        for (int i = 0; i < VD; i++) {
#pragma unroll
            for (int off = LPV; off < 64; off <<= 1) acc[r][i] += __shfl_xor(acc[r][i], off);
            if (kv == 0u) ob[wave][r][dv + i] = acc[r][i];
        }
        if (lane == 0u) { ms[wave][r] = m[r]; ls[wave][r] = l[r]; }
    }
    __syncthreads();
    for (uint32_t idx = tid; idx < (uint32_t)(R * HD); idx += 64u * kAsWaves) {
        const uint32_t r = idx / HD, d = idx % HD;
        float M = ms[0][r];                                                               // (the split has a tile and every live tile a live key: M is finite)
#pragma unroll
        for (int w = 1; w < kAsWaves; w++) M = fmaxf(M, ms[w][r]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int w = 0; w < kAsWaves; w++) {
            const float e = ms[w][r] == -INFINITY ? 0.0f : expf(ms[w][r] - M);           // a wave without a tile: an exact zero
            num += ob[w][r][d] * e;
            den += ls[w][r] * e;
        }
        const size_t slot = (size_t)(head0 + r) * S + s;
        scratch[slot * HD + d] = num;
        if (d == 0u) { ml[slot * 2u] = M; ml[slot * 2u + 1u] = den; }
    }
}

// ---- the windowed block (prefill) attention
constexpr int kWbWaves = 4;
typedef float wb_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 wb_f16x4 __attribute__((ext_vector_type(4)));

template <int HD>
__global__ __launch_bounds__(64 * kWbWaves) void attention_block_window_kernel(const float* __restrict__ qAll, const _Float16* __restrict__ kRing,
                                                                               const _Float16* __restrict__ vRing, uint32_t pos0, uint32_t rows,
                                                                               float* __restrict__ outAll, uint32_t numHeads, uint32_t kvRep,
                                                                               uint32_t ringRows, uint32_t window) {
    constexpr int NJ = HD / 16;                         // 8-byte pieces of a K row (16-byte ones of a q row) per lane
    constexpr int NV = HD / 64;                         // 8-byte pieces of a V row per lane and key
    constexpr int kPitch = HD + 4;                      // (a pitch of HD puts the 16 queries on the same banks)
    __shared__ alignas(16) float ob[16][kPitch];        // the merged accumulator [query][d]
    __shared__ float ms[kWbWaves][16], ls[kWbWaves][16], invL[16];
    const uint32_t head = blockIdx.x, qt = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, c = lane & 15u;
    const uint32_t lastKey = pos0 + rows - 1u;          // no token past it is read
    const uint32_t r = qt * 16u + c, qpos = pos0 + r;   // this lane's query: row of the block, absolute position
    const uint32_t qlo = attention_window_lo(qpos, window);                       // ... and the first key it sees
    const size_t rowStride = (size_t)numHeads * HD;
    const uint32_t cHeads = numHeads / kvRep, cHead = head / kvRep;               // the ring's heads per row, this head's among them
    const uint32_t lo = attention_window_lo(pos0 + qt * 16u, window);             // the first key ANY query of the tile sees
    const uint32_t firstTile = lo >> 4, lastTile = (pos0 + min(qt * 16u + 15u, rows - 1u)) >> 4;
    const float scale = 1.0f / sqrtf((float)HD);

    wb_f32x4 q[NJ];
    {
        const float* qp = qAll + (size_t)min(r, rows - 1u) * rowStride + head * HD + 4u * g;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const wb_f32x4 x = *reinterpret_cast<const wb_f32x4*>(qp + 16 * j);
            q[j] = r < rows ? x : wb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    // keys are clamped into lo .. lastKey: lastKey - lo <= window + rows - 2 < ringRows, every one a token the ring holds
    auto ask_k = [&](uint32_t t, wb_f16x4 (&k)[NJ]) {
        const ring_tile ring = ring_tile_at(t * 16u, lo, lastKey, ringRows);
        const _Float16* kp = kRing + ((size_t)ring.row(t * 16u + c) * cHeads + cHead) * HD + 4u * g;
#pragma unroll
        for (int j = 0; j < NJ; j++) k[j] = *reinterpret_cast<const wb_f16x4*>(kp + 16 * j);
    };
    auto ask_v = [&](uint32_t t, wb_f16x4 (&v)[4][NV]) {
        const ring_tile ring = ring_tile_at(t * 16u, lo, lastKey, ringRows);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const _Float16* vp = vRing + ((size_t)ring.row(t * 16u + 4u * g + i) * cHeads + cHead) * HD + 4u * c;
#pragma unroll
            for (int jj = 0; jj < NV; jj++) v[i][jj] = *reinterpret_cast<const wb_f16x4*>(vp + 64 * jj);
        }
    };

    float m = -INFINITY, l = 0.0f;                      // m: of query c (the same in its four lanes); l: this lane's keys only
    wb_f32x4 acc[4 * NV];
#pragma unroll
    for (int a = 0; a < 4 * NV; a++) acc[a] = wb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    wb_f16x4 kf[NJ], vf[4][NV];
    const uint32_t tBegin = firstTile + ((wave + 4u - (firstTile & 3u)) & 3u);    // this wave's first tile: tile t belongs to wave t % 4
    if (tBegin <= lastTile) ask_k(tBegin, kf);
    for (uint32_t t = tBegin; t <= lastTile; t += kWbWaves) {                      // (uniform in the wave)
        ask_v(t, vf);                                                              // in flight under the first product
        wb_f32x4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;                           // two chains: one does not fill the pipe
#pragma unroll
        for (int j = 0; j < NJ; j += 2) {
            const wb_f32x4 k0 = __builtin_convertvector(kf[j], wb_f32x4), k1 = __builtin_convertvector(kf[j + 1], wb_f32x4);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(k0[e], q[j][e], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[e], q[j + 1][e], s1, 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t + kWbWaves <= lastTile) ask_k(t + kWbWaves, kf);                     // the next tile's keys, under the second product
        __builtin_amdgcn_sched_barrier(0);
        float s[4], p[4];
        bool live[4];
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t key = t * 16u + 4u * g + i;
            live[i] = key >= qlo && key <= qpos;
            s[i] = live[i] ? (s0[i] + s1[i]) * scale : -INFINITY;                 // masked by selection
            tm = fmaxf(tm, s[i]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 16));
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        const float mn = fmaxf(m, tm);
        const float alpha = mn == -INFINITY ? 1.0f : expf(m - mn);                // (no live key yet: the state is zeros, keep it)
#pragma unroll
        for (int i = 0; i < 4; i++) p[i] = live[i] ? expf(s[i] - mn) : 0.0f;
        l = l * alpha + ((p[0] + p[1]) + (p[2] + p[3]));
        m = mn;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {                          // (x * 1 is x: skipping it where no query's max moved changes no bit)
#pragma unroll
            for (int a = 0; a < 4 * NV; a++) acc[a] *= alpha;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int jj = 0; jj < NV; jj++) {
                const wb_f32x4 v4 = __builtin_convertvector(vf[i][jj], wb_f32x4);
#pragma unroll
                for (int e = 0; e < 4; e++)
                    acc[4 * jj + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4[e], p[i], acc[4 * jj + e], 0, 0, 0);
            }
    }

    // merge: the four lanes of a query add their l in the order g = 0 .. 3, then the waves' states in the order w = 0, 1, ...
    const float lq = ((__shfl(l, (int)c) + __shfl(l, (int)c + 16)) + __shfl(l, (int)c + 32)) + __shfl(l, (int)c + 48);
    if (g == 0) { ms[wave][c] = m; ls[wave][c] = lq; }
    __syncthreads();
    float M = ms[0][c];                                  // (a query's own key is live in a tile of the walk: M is finite for every row < rows)
#pragma unroll
    for (int w = 1; w < kWbWaves; w++) M = fmaxf(M, ms[w][c]);
    const float mine = m == -INFINITY ? 0.0f : expf(m - M);                       // a wave with no live key: an exact zero
    if (wave == 0 && g == 0) {
        float L = 0.0f;
#pragma unroll
        for (int w = 0; w < kWbWaves; w++) L += ls[w][c] * (ms[w][c] == -INFINITY ? 0.0f : expf(ms[w][c] - M));
        invL[c] = 1.0f / L;
    }
    for (int w = 0; w < kWbWaves; w++) {
        if ((int)wave == w) {
#pragma unroll
            for (int jj = 0; jj < NV; jj++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    wb_f32x4* o = reinterpret_cast<wb_f32x4*>(&ob[c][64 * jj + 16 * g + 4 * i]);
                    const wb_f32x4 x = wb_f32x4{acc[4 * jj][i], acc[4 * jj + 1][i], acc[4 * jj + 2][i], acc[4 * jj + 3][i]} * mine;
                    *o = w == 0 ? x : *o + x;
                }
        }
        __syncthreads();
    }
    float* out = outAll + (size_t)(qt * 16u) * rowStride + head * HD;
    for (uint32_t idx = tid; idx < 16u * HD; idx += 64u * kWbWaves) {
        const uint32_t qi = idx / HD, d = idx % HD;
        if (qt * 16u + qi < rows) out[(size_t)qi * rowStride + d] = ob[qi][d] * invL[qi];
    }
}

// ---- launches.  The caller checked: kv_window_shape_ok, 1 <= maxPos / pos0 + rows <= kWindowMaxPos, 1 <= rows <= 64, 1 <= S <= kSplitMax
hipError_t launch_rope_kv_ring(const float* xq, const float* xk, const float* xv, float* qOut, _Float16* kRing, _Float16* vRing,
                               const uint32_t* pos, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, float ropeBase, uint32_t ringRows,
                               uint32_t maxPos, int* status, hipStream_t st) {
    hipLaunchKernelGGL(rope_kv_ring_kernel, dim3(numHeads + numHeadsKV), dim3(headDim), 0, st, xq, xk, xv, qOut, kRing, vRing, pos, numHeads,
                       numHeadsKV, logf(ropeBase), ringRows, maxPos, status);
    return hipGetLastError();
}
hipError_t launch_rope_kv_rows_ring(const float* xq, const float* xk, const float* xv, float* qOut, _Float16* kRing, _Float16* vRing,
                                    uint32_t pos0, uint32_t rows, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, float ropeBase,
                                    uint32_t ringRows, hipStream_t st) {
    hipLaunchKernelGGL(rope_kv_rows_ring_kernel, dim3(numHeads + numHeadsKV, rows), dim3(headDim), 0, st, xq, xk, xv, qOut, kRing, vRing, pos0,
                       numHeads, numHeadsKV, logf(ropeBase), ringRows);
    return hipGetLastError();
}
hipError_t launch_attention_window(const float* q, const _Float16* kRing, const _Float16* vRing, const uint32_t* pos, float* out, float* scratch,
                                   uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t ringRows, uint32_t window, uint32_t S,
                                   hipStream_t st) {
    const dim3 grid(numHeadsKV, S), block(64 * kAsWaves);
    const uint32_t R = numHeads / numHeadsKV;
#define EFFORT_AW_CASE(HD_, R_)                                                                                                                  \
    if (headDim == HD_ && R == R_) {                                                                                                             \
        hipLaunchKernelGGL((attention_window_kernel<HD_, R_>), grid, block, 0, st, q, kRing, vRing, pos, scratch, numHeads, ringRows, window);   \
    } else
#define EFFORT_AW_HD(HD_) EFFORT_AW_CASE(HD_, 1) EFFORT_AW_CASE(HD_, 2) EFFORT_AW_CASE(HD_, 4) EFFORT_AW_CASE(HD_, 8)
    EFFORT_AW_HD(64) EFFORT_AW_HD(128) EFFORT_AW_HD(256) return hipErrorInvalidValue;
#undef EFFORT_AW_HD
#undef EFFORT_AW_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_attention_merge(scratch, out, numHeads, headDim, S, st);
}
hipError_t launch_attention_block_window(const float* q, const _Float16* kRing, const _Float16* vRing, uint32_t pos0, uint32_t rows, float* out,
                                         uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t ringRows, uint32_t window,
                                         hipStream_t st) {
    const dim3 grid(numHeads, (rows + 15u) / 16u), block(64 * kWbWaves);
    const uint32_t kvRep = numHeads / numHeadsKV;
    switch (headDim) {
        case 64: hipLaunchKernelGGL((attention_block_window_kernel<64>), grid, block, 0, st, q, kRing, vRing, pos0, rows, out, numHeads, kvRep, ringRows, window); break;
        case 128: hipLaunchKernelGGL((attention_block_window_kernel<128>), grid, block, 0, st, q, kRing, vRing, pos0, rows, out, numHeads, kvRep, ringRows, window); break;
        case 256: hipLaunchKernelGGL((attention_block_window_kernel<256>), grid, block, 0, st, q, kRing, vRing, pos0, rows, out, numHeads, kvRep, ringRows, window); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace effort
