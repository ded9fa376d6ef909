// Prefill attention for a BLOCK of queries: the block's queries share each K / V row that is fetched.
//
//   out[r] = softmax(q[r] . K[t] / sqrt(headDim)) . V[t],  t = 0 .. pos0 + r,  r = 0 .. rows - 1, per head
//
// attention_rows_kernel (prefill.hip) is one workgroup per (head, query): 64 queries read the cache 64 times and keep pos0 + rows
// scores in LDS.  Here a workgroup is one head and one QUERY TILE of 16 rows of the block; it walks the keys in tiles of 16 with a
// flash-style online softmax (running max m, running sum l, a [16 x headDim] accumulator), so a fetched K / V tile serves 16 queries
// and the state -- registers plus kAbLds bytes of LDS for the final merge -- does not grow with the position.
//
// Arithmetic: f32 end to end, both products on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain).  Lane l = 16 g + c.
//   S^T = K . Q^T   A = K tile (lane: key c, k = g), B = Q^T (lane: query c, k = g).  The sum over d runs in the permuted order
//                   d = 16 j + 4 g + e, step (j, e): a lane's operands of the four steps e are ONE 16-byte load, K and Q alike.
//                   The result has the query on the lane and keys 4 g + i in registers i = 0 .. 3.
//   out^T += V^T . P^T   those four registers ARE the B operand of k step i (k = g <-> key 4 g + i): no lane movement, no LDS.  A =
//                   V^T (lane: row c of the d tile, key 4 g + i).  Row c of d tile 4 jj + e stands for d = 64 jj + 4 c + e, so a
//                   lane's A operands of four d tiles are one 16-byte load and 16 lanes read 256 contiguous bytes of a V row.
//                   Accumulator register i of d tile 4 jj + e is then d = 64 jj + 16 g + 4 i + e of query c.
// (A wrong lane map moves every element by O(1): tests/test_gpu_attention_block.py compares each with float64 on random -- asymmetric
// -- operands, and with marker keys that put a query's whole weight on one V row.)
//
// Geometry: grid (numHeads, ceil(rows / 16)), kAbWaves waves per workgroup.  Wave w takes the ABSOLUTE key tiles w, w + kAbWaves, ...
// up to the query tile's last position and keeps its own (m, l, acc); the states merge through LDS in the order w = 0, 1, ...
// Measured at 32 heads, headDim 128, 64 rows at position 4032, us per call (profiles/r10_prefill_attention.json; DESIGN 4.4a has the
// table): this kernel 112 -- effort_attention_rows 1867; before the accumulator's rescale was skipped where no max moved 119; eight
// waves 100 there but slower below position 1000 and out of registers at headDim 256; a second pair of K / V buffers loaded a
// whole tile ahead 111 there and 37 against 32 at position 960; the next tile's first product issued beside the softmax 266.  The
// f32 matrix rate bounds it at 55 (the grid fills half the CUs at 32 heads): it runs at half that, and what holds it has not
// been profiled.
//
// The order of the sums follows the absolute position only.  Key tiles sit on multiples of 16 counted from token 0, tile t belongs
// to wave t % kAbWaves, a wave takes its tiles in ascending order and the states merge in wave order.  A key that a query may not
// see is SELECTED out (score -inf, probability 0 -- never 0 * something computed), so a tile that is wholly masked for a query
// leaves its state as it was, bit for bit (alpha = exp(0) = 1, p = 0), and a wave that saw no live key merges as an exact zero.
// So an output row's bits are a function of the query, its absolute position and cache rows 0 .. position -- not of pos0, rows or
// the row's place in the block.  They are NOT the bits of effort_attention / effort_attention_rows (another order of the sums).
//
// Reads: cache rows below pos0 + rows and q rows below rows only.  A key index at or past pos0 + rows is CLAMPED to the last live
// row: its score is selected out, its probability is an exact 0 on a finite V row.  A q row at or past rows is a zero operand.
#include "effort_internal.h"

namespace effort {

constexpr int kAbWaves = 4;

typedef float ab_f32x4 __attribute__((ext_vector_type(4)));

template <int HD>
__global__ __launch_bounds__(64 * kAbWaves) void attention_block_kernel(const float* __restrict__ qAll, const float* __restrict__ kCache,
                                                                        const float* __restrict__ vCache, uint32_t pos0, uint32_t rows,
                                                                        float* __restrict__ outAll, uint32_t numHeads) {
    constexpr int NJ = HD / 16;                         // 16-byte pieces of a K (and q) row per lane
    constexpr int NV = HD / 64;                         // 16-byte pieces of a V row per lane and key
    constexpr int kPitch = HD + 4;                      // (a pitch of HD puts the 16 queries on the same banks)
    __shared__ alignas(16) float ob[16][kPitch];        // the merged accumulator [query][d]
    __shared__ float ms[kAbWaves][16], ls[kAbWaves][16], invL[16];
    const uint32_t head = blockIdx.x, qt = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, c = lane & 15u;
    const uint32_t limit = pos0 + rows;                 // no cache row at or past it is read
    const uint32_t r = qt * 16u + c, qpos = pos0 + r;   // this lane's query: row of the block, absolute position
    const size_t rowStride = (size_t)numHeads * HD;
    const uint32_t lastTile = (pos0 + min(qt * 16u + 15u, rows - 1u)) >> 4;
    const float scale = 1.0f / sqrtf((float)HD);

    ab_f32x4 q[NJ];
    {
        const float* qp = qAll + (size_t)min(r, rows - 1u) * rowStride + head * HD + 4u * g;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const ab_f32x4 x = *reinterpret_cast<const ab_f32x4*>(qp + 16 * j);
            q[j] = r < rows ? x : ab_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    auto ask_k = [&](uint32_t t, ab_f32x4 (&k)[NJ]) {
        const float* kp = kCache + ((size_t)min(t * 16u + c, limit - 1u) * numHeads + head) * HD + 4u * g;
#pragma unroll
        for (int j = 0; j < NJ; j++) k[j] = *reinterpret_cast<const ab_f32x4*>(kp + 16 * j);
    };
    auto ask_v = [&](uint32_t t, ab_f32x4 (&v)[4][NV]) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float* vp = vCache + ((size_t)min(t * 16u + 4u * g + i, limit - 1u) * numHeads + head) * HD + 4u * c;
#pragma unroll
            for (int jj = 0; jj < NV; jj++) v[i][jj] = *reinterpret_cast<const ab_f32x4*>(vp + 64 * jj);
        }
    };

    float m = -INFINITY, l = 0.0f;                      // m: of query c (the same in its four lanes); l: this lane's keys only
    ab_f32x4 acc[4 * NV];
#pragma unroll
    for (int a = 0; a < 4 * NV; a++) acc[a] = ab_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    ab_f32x4 kf[NJ], vf[4][NV];
    if (wave <= lastTile) ask_k(wave, kf);
    for (uint32_t t = wave; t <= lastTile; t += kAbWaves) {                        // (uniform in the wave)
        ask_v(t, vf);                                                              // in flight under the first product
        ab_f32x4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;                           // two chains: one does not fill the pipe
#pragma unroll
        for (int j = 0; j < NJ; j += 2)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][e], q[j][e], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j + 1][e], q[j + 1][e], s1, 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
        if (t + kAbWaves <= lastTile) ask_k(t + kAbWaves, kf);                     // the next tile's keys, under the second product
        __builtin_amdgcn_sched_barrier(0);
        float s[4], p[4];
        bool live[4];
        float tm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            live[i] = t * 16u + 4u * g + i <= qpos;
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
            for (int jj = 0; jj < NV; jj++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    acc[4 * jj + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i][jj][e], p[i], acc[4 * jj + e], 0, 0, 0);
    }

    // merge: the four lanes of a query add their l in the order g = 0 .. 3, then the waves' states in the order w = 0, 1, ...
    const float lq = ((__shfl(l, (int)c) + __shfl(l, (int)c + 16)) + __shfl(l, (int)c + 32)) + __shfl(l, (int)c + 48);
    if (g == 0) { ms[wave][c] = m; ls[wave][c] = lq; }
    __syncthreads();
    float M = ms[0][c];                                  // (wave 0 owns tile 0 and key 0 is live for every query: M is finite)
#pragma unroll
    for (int w = 1; w < kAbWaves; w++) M = fmaxf(M, ms[w][c]);
    const float mine = m == -INFINITY ? 0.0f : expf(m - M);                       // a wave with no live key: an exact zero
    if (wave == 0 && g == 0) {
        float L = 0.0f;
#pragma unroll
        for (int w = 0; w < kAbWaves; w++) L += ls[w][c] * (ms[w][c] == -INFINITY ? 0.0f : expf(ms[w][c] - M));
        invL[c] = 1.0f / L;
    }
    for (int w = 0; w < kAbWaves; w++) {
        if ((int)wave == w) {
#pragma unroll
            for (int jj = 0; jj < NV; jj++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    ab_f32x4* o = reinterpret_cast<ab_f32x4*>(&ob[c][64 * jj + 16 * g + 4 * i]);
                    const ab_f32x4 x = ab_f32x4{acc[4 * jj][i], acc[4 * jj + 1][i], acc[4 * jj + 2][i], acc[4 * jj + 3][i]} * mine;
                    *o = w == 0 ? x : *o + x;
                }
        }
        __syncthreads();
    }
    float* out = outAll + (size_t)(qt * 16u) * rowStride + head * HD;
    for (uint32_t idx = tid; idx < 16u * HD; idx += 64u * kAbWaves) {
        const uint32_t qi = idx / HD, d = idx % HD;
        if (qt * 16u + qi < rows) out[(size_t)qi * rowStride + d] = ob[qi][d] * invL[qi];
    }
}

// the caller checked: 1 <= rows <= 64, pos0 + rows <= maxTokens <= 8192, headDim 64 / 128 / 256
hipError_t launch_attention_block(const float* q, const float* kCache, const float* vCache, uint32_t pos0, uint32_t rows, float* out,
                                  uint32_t numHeads, uint32_t headDim, hipStream_t st) {
    const dim3 grid(numHeads, (rows + 15u) / 16u), block(64 * kAbWaves);
    switch (headDim) {
        case 64: hipLaunchKernelGGL(attention_block_kernel<64>, grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads); break;
        case 128: hipLaunchKernelGGL(attention_block_kernel<128>, grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads); break;
        case 256: hipLaunchKernelGGL(attention_block_kernel<256>, grid, block, 0, st, q, kCache, vCache, pos0, rows, out, numHeads); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace effort
