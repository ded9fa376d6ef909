/*
 * effort_hip.h -- C ABI of the MI355X (gfx950) implementation of Effort's bucketMul hot path.
 *
 * This is the drop-in boundary: every entry point below replaces one piece of the reference's
 * Swift/Metal interface for the path (file:line relative to kolinko/effort @ 2024_08_07).  A
 * Swift shim that keeps `bucketMul(v:by:expNo:out:effort:)` / `bucketMulQ4(...)` and forwards
 * here is shown in INTEGRATION.md.  Plain pointers and sizes only; all `*_dev` pointers are
 * device (HBM) addresses owned by the caller.  Nothing here depends on PyTorch.
 *
 * Conventions (reference: helpers/gpu.swift:109-196)
 *   - Calls ENQUEUE work on the context's HIP stream and return; results are valid after
 *     effort_sync() (= gpu.eval(), helpers/gpu.swift:109-119) or any later work on that stream.
 *   - The reference aborts on violated preconditions (assert/precondition); this ABI returns a
 *     negative error code instead and enqueues nothing.
 *   - One effort_ctx per host thread / stream (the reference's BucketMul.shared singleton,
 *     bucketMul.swift:24, is not re-entrant; a context is its re-entrant equivalent and owns the
 *     same scratch: cutoff, dispatch counter, partial tiles).
 */
#ifndef EFFORT_HIP_H
#define EFFORT_HIP_H

#include <stdint.h>

#if defined(__GNUC__)
#define EFFORT_API __attribute__((visibility("default")))
#else
#define EFFORT_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct effort_ctx effort_ctx;
typedef struct effort_w effort_w;      /* = class ExpertWeights, loader.swift:46-167 */

enum {
    EFFORT_OK = 0,
    EFFORT_ERR_ARG = -1,          /* null pointer / bad handle                                        */
    EFFORT_ERR_SHAPE = -2,        /* inDim >= 4096, outDim % 32 == 0, outDim <= 16384 (bucketMul.swift:36,52,73) */
    EFFORT_ERR_EFFORT = -3,       /* effort outside [0,1]                                              */
    EFFORT_ERR_HIP = -4,          /* a HIP runtime call failed (see effort_last_error)                 */
    EFFORT_ERR_KIND = -5,         /* FP16 weights passed to the Q4 call or vice versa                  */
    EFFORT_ERR_CONVERT = -6,      /* bucketize() preconditions (convert.swift:210-215,239)             */
    EFFORT_ERR_BLAS = -7,         /* rocBLAS failure in effort_dense_gemv                              */
    EFFORT_ERR_COMM = -8          /* an RCCL call failed (see effort_last_error)                       */
};

/* ---- context = class Gpu + the BucketMul / BucketMulQ4 singletons ------------------------------ */

/* helpers/gpu.swift:36-60 (device, queue) + bucketMul.swift:24-32 (scratch).  `stream` is a
 * hipStream_t (NULL = the default stream).  Returns NULL on failure. */
EFFORT_API effort_ctx* effort_create(int device, void* stream);
EFFORT_API void effort_destroy(effort_ctx* ctx);
EFFORT_API int effort_set_stream(effort_ctx* ctx, void* stream);
/* gpu.eval() -- helpers/gpu.swift:109-119: block until everything enqueued so far has finished. */
EFFORT_API int effort_sync(effort_ctx* ctx);
/* Overlap of independent launches (the reference's command queue lets independent kernels overlap too, helpers/gpu.swift:
 * 135-196).  lanes = 1 (default): every call is enqueued on the context's stream, in order.  lanes = 2..4: the context owns
 * that many internal streams, each with its own scratch, and every effort_bucketmul* call goes to one of them, ordered
 *   - after everything enqueued ON THE CONTEXT'S STREAM before the call -- exactly that: outside a capture the lane forks from the
 *     stream only if the stream still has work (hipStreamQuery); when it answers "idle" everything enqueued on it has completed and
 *     no edge is recorded.  Work the caller keeps on OTHER streams is ordered against a multiply only through the context's stream:
 *     make that stream wait for it (hipStreamWaitEvent) before the call -- a wait enqueued on the stream keeps it "busy" until
 *     the event fires, so the fork happens -- and do not rely on an earlier, already completed wait.  Inside a capture the fork
 *     is always a graph edge; a lane's completion event is recorded lazily, when something first waits for the lane (a join, a
 *     dependent launch on another lane), which may be inside a capture that began after the lane's launches: the event then becomes a
 *     node of that graph and orders the graph's work after launches enqueued BEFORE the capture (a join at the top of the
 *     capture is the explicit form) -- and
 *   - after earlier multiplies of this context whose outputs it reads or overwrites, or whose inputs it overwrites (address
 *     ranges of v / expNo / aux / resid / out are compared);
 * otherwise it runs beside the multiplies still in flight: the head of one launch (staging, cutoffs, selection: HBM idle)
 * hides under the streaming of the others (one 32-call launch after another, each on its own matrices: 0.60 -> 0.70 of the
 * HBM roofline).  Results are bit-identical for FP16 and outlier-free Q4 bundles (Q4 outlier sums: see effort_bucketmul_q4).  The multiplies become visible to the context's stream at effort_join (enqueues waits, returns at
 * once), and implicitly at effort_sync, at any other effort_* call on the context and at the test hooks.  A caller who
 * enqueues its OWN work on the stream to consume an output calls effort_join first; inside a hipGraph capture call
 * effort_join before ending the capture (the lanes fork from and must rejoin the capturing stream).
 * Costs 64 MiB of scratch per extra lane.
 * Runtime note (HIP 7.0.x as bundled by torch 2.10+rocm7.0, found in round 6): DESTROYING a hipGraph that was captured across several
 * streams -- which every capture of a context with lanes > 1 is -- corrupts the HIP runtime's heap (reproducible with plain torch ops,
 * tools/lab/graph_event_repro.py); keep such graphs for the life of the process, or capture with lanes = 1. */
EFFORT_API int effort_set_overlap(effort_ctx* ctx, int lanes);
EFFORT_API int effort_join(effort_ctx* ctx);
/* Cache policy of the bucket-row stream.  reuse = 0 (default): the kept rows are read NON-TEMPORALLY -- a row is read once per call and a
 * model's weights are tens of times the chip's caches (Mistral-7B at 25 % effort reads 3.5 GB per token against 32 MB of L2 and 256 MB of
 * Infinity Cache), so the stream should not push the row means, the partial tiles and the other launches' lines out on its way through
 * (one 32-call launch 160 -> 150 us, four in flight 133 -> 127, a lone call 18.1 -> 17.75: DESIGN.md 4.1).  reuse = 1: the ordinary policy,
 * for a caller whose launches in flight read the SAME matrices within a few hundred MB of one another (a batch of inputs on one set of
 * weights, through effort_set_overlap lanes or several contexts): the later launches then hit in the Infinity Cache (four launches in flight
 * on one set of 32 matrices: 117 us per launch against 130).  Speed only: results are bit-identical either way.  Takes effect with the next
 * launch (a captured launch keeps the policy it was captured with).  The second policy lives in the kernels that serve GROUP launches (persistent grids,
 * and plain grids of 256-column tiles): lone calls, pairs and plain launches of narrower tiles ignore the hint (two copies of the loop cost them 0.1-0.3 us
 * per call on the default path). */
EFFORT_API int effort_set_row_reuse(effort_ctx* ctx, int reuse);
/* Text of the context's last error; with ctx == NULL: why the last effort_create returned NULL ("null context" if none did). */
EFFORT_API const char* effort_last_error(effort_ctx* ctx);
EFFORT_API const char* effort_version(void);

/* ---- weights = ExpertWeights ------------------------------------------------------------------- */

/* FP16 bundle (loader.swift:46-167, layout written by convert.swift:209-260):
 *   buckets f16 [numExperts][inDim*percentLoad][outDim/16]   rank-major bucket rows, low 4 mantissa
 *                                                            bits of each weight = output position
 *   stats   f16 [numExperts][inDim*percentLoad][4]           mean|row| in all four lanes (.w is read)
 *   probes  f16 [numExperts][4096]
 * percentLoad (1..16) = rank slices present per expert (loader.swift:50, expertSize = percentLoad*inDim).
 * Accepted sizes (anything else: NULL, EFFORT_ERR_SHAPE, nothing read): 4096 <= inDim <= 65535 (odd ones included), outDim a multiple of 32
 * up to 16384, and -- the multiply addresses every per-row array with 32-bit offsets -- with rows = numExperts * percentLoad * inDim
 * bucket rows in the whole stack: buckets (rows * row pitch) < 4 GiB AND stats (rows * 8 bytes) < 4 GiB, i.e. rows < 2^29.  The second
 * limit is the tighter one only where a bucket row is shorter than 8 bytes (outDim 32; Q4: outDim 32, 64, 96).
 * Pointers are BORROWED: the caller keeps the buffers alive while the handle is in use.  Registration reads the
 * buckets once (max |w| of every bucket row, which bounds the multiply's fixed-point accumulators): fill the
 * buffers BEFORE registering, and register again if their contents change. */
EFFORT_API effort_w* effort_weights_fp16(effort_ctx* ctx, const void* buckets_dev, const void* stats_dev,
                              const void* probes_dev, int inDim, int outDim, int percentLoad,
                              int numExperts);

/* The same with bucket rows `rowPitchBytes` apart (0 = 2*outDim/16, the reference's dense layout; otherwise a multiple of 4
 * bytes >= that: rows are read as dwords.  The CONVERTER is stricter -- effort_convert_fp16_pitched writes pitches that are
 * multiples of 8 -- and effort_aligned_row_pitch returns multiples of 128; one shape rule everywhere: outDim % 32 == 0).
 * The reference's rows are 2*cols bytes apart (1376 for 11008 outputs): the 512-byte row pieces the multiply streams then
 * straddle 128-byte lines and HBM delivers 5.4-5.6 TB/s where line-aligned rows reach 6.1-6.9.  A loader that places the rows
 * effort_aligned_row_pitch(outDim) bytes apart (effort_convert_fp16_pitched writes them so) gets the fast stream with no
 * second copy of the buckets (+2.3 % bytes for 11008 outputs).  Results are bit-identical for any pitch. */
EFFORT_API effort_w* effort_weights_fp16_pitched(effort_ctx* ctx, const void* buckets_dev, int rowPitchBytes, const void* stats_dev,
                                      const void* probes_dev, int inDim, int outDim, int percentLoad, int numExperts);
/* 2*outDim/16 rounded up to whole 128-byte lines; EFFORT_ERR_SHAPE for an outDim registration would refuse (outDim % 32, <= 16384). */
EFFORT_API int effort_aligned_row_pitch(int outDim);

/* Q4 bundle (layout written by q4_draft.py:70-322; loaded by loader.swift:70,98,124):
 *   buckets  u16 [numExperts][inDim*8][outDim/32]   4 nibbles per word, nibble = sign<<3 | pos,
 *                                                   bucket row i = inRow*8 + rank (input-major)
 *   stats    f32 [numExperts][inDim*8][2]           (mean|row|, same); .y is read
 *   probes   f16 [numExperts][4096]
 *   outliers f32 [nOutliers][4]                     (value, inIdx, outIdx, 0); may be NULL / 0
 * Borrowed like the FP16 bundle, except the outlier table: registration turns it into an index in HBM of FOUR bytes per
 * outlier (f16 value | output within a block of 2^(16 - bits of inDim) outputs | input: hence inDim, outDim <= 65536 when there
 * are outliers) and does not read outliers_dev again.  Every entry must name an element of this matrix and carry a value that
 * is an f16 number (the table comes from an f16 matrix, q4_draft.py:58-67): otherwise NULL is returned (EFFORT_ERR_ARG). */
EFFORT_API effort_w* effort_weights_q4(effort_ctx* ctx, const void* buckets_dev, const void* stats_dev,
                            const void* probes_dev, const void* outliers_dev, int64_t nOutliers,
                            int inDim, int outDim, int numExperts);
EFFORT_API void effort_weights_free(effort_w* w);
/* The multiply accumulates in fixed point; its scale comes from a per-expert bound on the weights (sum over ranks of the
 * rank's largest |w|; Q4: largest row mean) read at registration.  If the borrowed buffers are REWRITTEN afterwards (the
 * reference's loader.swift buffers are mutable) call effort_weights_refresh before the next multiply: with a stale bound
 * the sums of larger weights can wrap (a bound too SMALL by a factor g wraps an output that exceeds 2/g of the true bound L
 * below; short of that it merely makes the grid finer; one that is too LARGE makes it coarser in proportion).  get/set copy the bound
 * ([numExperts] floats, host memory): a column shard of a multi-GPU split can take the full matrix's bound, so that every
 * rank rounds its products on the same grid.
 * What the bound costs: a workgroup rounds each product to a step in (L * 2^-30, L * 2^-29], L = (sum of |v_j| over its row
 * slice) * bound, so an output of m products is off by about sqrt(m / 12) * L * 2^-29.5.  Against max|out| that is 1-6e-6 for
 * weights at ONE scale (L / max|out| about 2^9 on the whole input, divided by the slice count) and finer than an f32 running
 * sum while the slice's L / max|out| stays below about 2^5.  The bound is a worst case over every input channel: a per-channel
 * scale spread, one large channel or one large weight raise L and not the outputs (L / max|out| 2^11 .. 2^18 measured), and the
 * error grows in proportion -- past 2e-5 * max|out| once the slice's ratio exceeds about 2^8 (measured table).
 * FP16 handles also keep a compact copy of the row means (stats lane .w, 2 bytes per bucket row: +0.15 % of the buckets'
 * size) that big launches stage instead of the 8-byte stats; effort_weights_refresh re-reads it with the bound. */
EFFORT_API int effort_weights_refresh(effort_w* w);
/* Row pitch.  The converter's bucket rows are 2*cols bytes apart (1376 for 11008 outputs), so the row pieces the multiply
 * streams straddle 128-byte lines and HBM delivers 5.4-5.6 TB/s instead of 6.1-6.9 (measured on line-aligned shapes).
 * effort_weights_align_rows gives a handle registered on the dense layout its OWN device copy of the buckets with every row
 * on a 128-byte boundary and reads that from then on (bit-identical results; the caller's buffer is no longer read by
 * multiplies and may be freed -- keep it if effort_weights_refresh will be needed).  Call it BEFORE capturing launches of
 * the handle into a hipGraph (a captured launch keeps the pointers it was given).  No-op if the pitch is aligned already
 * (buckets converted or loaded with effort_aligned_row_pitch: no second copy).  effort_weights_row_pitch: bytes. */
EFFORT_API int effort_weights_align_rows(effort_w* w);
EFFORT_API int effort_weights_row_pitch(const effort_w* w);
EFFORT_API int effort_weights_get_bound(effort_w* w, float* host_out);
EFFORT_API int effort_weights_set_bound(effort_w* w, const float* host_in);

/* ---- the hot path ------------------------------------------------------------------------------ */

/* func bucketMul(v:by:expNo:out:effort:) -- bucketMul.swift:11-15 -> BucketMul.fullMul (:54-70):
 * findCutoff32 + prepareDispatch + roundUp/zeroRange32 + bucketMul + bucketIntegrate
 * (bucketMul.metal:11-247).  v_dev f32[inDim], out_dev f32[outDim] (fully overwritten),
 * expNo_dev = device u32 expert index (NULL = expert 0; expertMul.swift:18-22), effort in [0,1].
 * Row selection (cutoff, dispatch set) is bit-exact with the reference's arithmetic.  Products are accumulated in
 * per-workgroup fixed point: order-free, hence bit-identical run to run; within 2e-5 * max|out| of
 * an f32 accumulation for weights at one scale (measured 1-6e-6), beyond it where the weights' bound is loose (see
 * effort_weights_refresh above and DESIGN.md 2.1). */
EFFORT_API int effort_bucketmul(effort_ctx* ctx, const effort_w* w, const float* v_dev, const uint32_t* expNo_dev,
                     float* out_dev, double effort);

/* func bucketMulQ4(...) -- bucketMulQ4.swift:11-17 -> fullMul (:54-63), INCLUDING the caller's
 * out.zero() (expertMul.swift:27) and the calcOutliers pass (bucketMulQ4.metal:13-21).
 * Determinism: the bucket rows are accumulated in fixed point like effort_bucketmul's (order-free).  The OUTLIER sums are f32, as the
 * reference's float atomics are: an output's entries are added in the table's order, and an item whose share of the outputs is thin
 * splits them among the waves of its workgroup, the partial sums added in wave order.  How they are split follows the launch geometry
 * (group size, the device's CU count, a column shard against the full handle), so a bundle WITH outliers gives bit-identical results
 * run to run for one geometry, and results that may differ in the last bits between a lone call, a grouped call and a column shard
 * (all within the 2e-5 * max|out| bar).  The split also follows the effort_set_overlap setting (a context with lanes picks other
 * launch geometries) and, in a group, the efforts of the group's calls (a thin group is sliced differently): the same call in another
 * group, or under another lanes setting, may differ in those last bits too.  Without outliers Q4 is as order-free as FP16. */
EFFORT_API int effort_bucketmul_q4(effort_ctx* ctx, const effort_w* w, const float* v_dev, const uint32_t* expNo_dev,
                        float* out_dev, double effort);

/* func basicMul(v:by:out:) -- helpers/mps.swift:14-47: dense out = W * f16(v), W f16 [outDim,inDim]
 * row-major, f32 result; the "100 % effort dense" baseline.  A streaming HIP kernel (csrc/gemv.hip) by default;
 * effort_set_dense_backend(ctx, 1) routes it through rocBLAS' hssgemv instead (the library the north star names: the
 * bench reports both). */
EFFORT_API int effort_dense_gemv(effort_ctx* ctx, const void* W_f16_dev, const float* v_dev, float* out_dev,
                      int inDim, int outDim);
EFFORT_API int effort_set_dense_backend(effort_ctx* ctx, int rocblas);
/* basicMul on ONE expert of a stack of cores, W f16 [numExperts][outDim][inDim], the expert number read from device memory
 * (*expNo_dev, as the multiplies take it): the dense baseline of a routed FFN without gathering the expert's matrix first.  The
 * same kernel body and summation order as effort_dense_gemv on W[*expNo_dev], hence its result bit for bit; instantiation and
 * cache policy follow the size of one expert's matrix.  Always the in-tree kernel, whatever effort_set_dense_backend says:
 * EFFORT_ERR_SHAPE where that kernel does not serve the shape (inDim % 16, inDim > 65536) or the whole stack reaches 4 GiB.
 * A device value cannot be refused by a return code: an expert number >= numExperts is CLAMPED to numExperts - 1. */
EFFORT_API int effort_dense_gemv_expert(effort_ctx* ctx, const void* W_f16_dev, const uint32_t* expNo_dev, const float* v_dev,
                             float* out_dev, int inDim, int outDim, int numExperts);

/* A GROUP of n (1..32) independent bucketMul calls in ONE kernel launch: call i multiplies vs[i] by ws[i] at
 * efforts[i] into outs[i] (expNos may be NULL, or hold NULL entries = expert 0).  Same row selection as n
 * effort_bucketmul calls, exactly; outputs equal up to the f32 rounding of the per-slice partial sums (the slicing
 * depends on how many calls share the launch; bit for bit when it is pinned with effort_hip_debug.h's effort_set_tuning).  The point is
 * throughput: the decode loop issues such groups back to back on unchanged
 * input -- Wq|Wk|Wv (runNetwork.swift:132-134) and W1|W3 (runNetwork.swift:178-182) -- and the reference's command
 * buffer lets them overlap; here their workgroups share the CUs inside one launch.  All handles of a group are of
 * the same kind; shapes may differ (a launch carries four distinct shapes; a group with more is issued as consecutive
 * launches).  effort_group_dispatch_count / effort_group_cutoff read call idx's hooks. */
EFFORT_API int effort_bucketmul_group(effort_ctx* ctx, int n, const effort_w* const* ws, const float* const* vs_dev,
                           const uint32_t* const* expNos_dev, float* const* outs_dev, const double* efforts);
/* effort_bucketmul_group with the decode loop's neighbouring element-wise steps folded into the launch (FP16 bundles):
 *   prologues[i] (NULL = all 0): how call i derives its input from vs[i] --
 *     EFFORT_PRE_NONE      input = v
 *     EFFORT_PRE_SILU_GATE input = x3 * v / (1 + exp(-v)), x3 = v_aux[i] f32 [inDim]: silu(x1, x3, out: x2) feeding w2
 *                          (runNetwork.swift:181-182, matrix.metal:25-35)
 *     EFFORT_PRE_RMSNORM   input = v / sqrt(mean(v^2) + 1e-5) * w, w = v_aux[i] f16 [inDim]: rmsNormFast + mul(by:)
 *                          feeding wq|wk|wv and w1|w3 (runNetwork.swift:121-122,173-175; aux.metal:113-152)
 *   resids[i] (NULL array or entry = none): out = resid + product -- h.add(by:) after wo and w2 (runNetwork.swift:172,183);
 *     resid may alias outs[i] (h += product in place).
 * Cutoff, dispatch and accumulation see the derived input exactly as if it had been materialised first.  A decoder layer
 * is then five launches instead of eight (Mistral-7B shapes at 25 % effort: 307 against 300 tokens/s, bit-identical logits). */
#define EFFORT_PRE_NONE 0
#define EFFORT_PRE_SILU_GATE 1
#define EFFORT_PRE_RMSNORM 2
EFFORT_API int effort_bucketmul_group_fused(effort_ctx* ctx, int n, const effort_w* const* ws, const float* const* vs_dev,
                                 const uint32_t* const* expNos_dev, float* const* outs_dev, const double* efforts,
                                 const int* prologues, const void* const* v_aux_dev, const float* const* resids_dev);
EFFORT_API int effort_bucketmul_q4_group(effort_ctx* ctx, int n, const effort_w* const* ws, const float* const* vs_dev,
                              const uint32_t* const* expNos_dev, float* const* outs_dev, const double* efforts);
/* effort_bucketmul_q4_group with the same prologues and residual epilogue as effort_bucketmul_group_fused, for Q4 bundles: the
 * argument contract is that entry's (prologues / v_aux_dev / resids_dev may be NULL or hold 0 / NULL entries; resid may alias
 * outs[i]; refused with EFFORT_ERR_KIND after effort_set_split_cutoff; effort_bucketmul_group_fused itself keeps refusing Q4
 * handles with EFFORT_ERR_KIND).  The derived input is what effort_silu_mul / effort_add_rmsnorm_mul would have written, bit for
 * bit, so cutoff and row selection equal the materialise-first path's exactly; out = resid + (fixed-point sum + outlier sum), one
 * f32 add of the finished product, and nothing is stored to out before resid has been read.
 * OUTLIERS: calcOutliers needs the whole derived input, which the kernel keeps in LDS for inDim <= 16384.  A handle WITH outliers
 * and inDim > 16384 that carries a prologue is refused with EFFORT_ERR_SHAPE (nothing is enqueued): materialise the input with
 * the glue kernel, or register the bundle without outliers.  Without outliers, or with a residual alone, any size works. */
EFFORT_API int effort_bucketmul_q4_group_fused(effort_ctx* ctx, int n, const effort_w* const* ws, const float* const* vs_dev,
                                    const uint32_t* const* expNos_dev, float* const* outs_dev, const double* efforts,
                                    const int* prologues, const void* const* v_aux_dev, const float* const* resids_dev);
EFFORT_API int effort_group_dispatch_count(effort_ctx* ctx, int idx, uint32_t* host_out);
EFFORT_API int effort_group_cutoff(effort_ctx* ctx, int idx, float* host_out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------------------------------
 * The reference is single-device (helpers/gpu.swift:36-38); this is what a host needs to spread the path over the GPUs of a
 * node.  Two partitions: whole MATRICES on different ranks (nothing below but the communicator and the gather of the output
 * vectors), or bucket COLUMNS of one matrix across the ranks:
 *   effort_weights_column_shard(full, rank, world) -- rank's columns [rank*C/world, (rank+1)*C/world) of every bucket row of a
 *     registered bundle, i.e. outputs [rank*outDim/world, ...), as a VIEW of the full handle's buffers (no copy; C/world must be
 *     even); stats and probes are shared -- they are row-global, so every rank computes the same cutoff and selects the same rows
 *     -- and the shard takes the full matrix's fixed-point bound.  Q4: with the slice of the outlier index on those outputs.
 *     Multiply it like any handle; free it BEFORE the full handle; after rewriting weights in place refresh the FULL handle and
 *     shard again (effort_weights_refresh refuses a shard).
 *   effort_comm_unique_id: rank 0 makes the 128-byte id, the host program ships it to the other ranks by its own means;
 *   effort_comm_create(ctx, rank, world, id): collective over the world (ncclCommInitRank); one communicator per context;
 *   effort_allgather_outputs(ctx, send, recv, count): recv f32 [world][count] = every rank's `count` outputs, enqueued on the
 *     context's stream after the multiplies that wrote them (send may be recv + rank*count).  Matrices sharing an input
 *     vector put their shards' outputs side by side and gather ONCE (the messages are KB-scale: latency-bound over xGMI). */
#define EFFORT_COMM_ID_BYTES 128
EFFORT_API effort_w* effort_weights_column_shard(const effort_w* full, int rank, int world);
EFFORT_API int effort_comm_unique_id(void* id_out_128_bytes);
EFFORT_API int effort_comm_create(effort_ctx* ctx, int rank, int world, const void* id_128_bytes);
EFFORT_API int effort_comm_destroy(effort_ctx* ctx);
EFFORT_API int effort_comm_rank(effort_ctx* ctx);
EFFORT_API int effort_comm_world(effort_ctx* ctx);
EFFORT_API int effort_allgather_outputs(effort_ctx* ctx, const float* send_dev, float* recv_dev, int count);

/* ---- reference-visible state / test hooks ------------------------------------------------------ */

/* dispatch.size after calcDispatch (bucketMul.swift:46-47): number of bucket rows selected by the most
 * recent effort_bucketmul / _q4 / effort_calc_dispatch, before padding.  Synchronises the stream. */
EFFORT_API int effort_last_dispatch_count(effort_ctx* ctx, uint32_t* host_out);
/* BucketMul.shared.cutoff (bucketMul.swift:22).  Synchronises the stream. */
EFFORT_API int effort_last_cutoff(effort_ctx* ctx, float* host_out);

/* BucketMul.calcDispatch (bucketMul.swift:34-47) materialised in the reference's format: float2
 * entries {v[row % inDim] (Q4: v[row/8]*mean), float(row*cols)} in ASCENDING bucket-row order (the
 * reference's atomic append order is unspecified), count written to *count_dev.  dispatch_dev must
 * hold 2*inDim*percentLoad floats.  Not used by the fused hot path; kept for parity tests. */
EFFORT_API int effort_calc_dispatch(effort_ctx* ctx, const effort_w* w, const float* v_dev, const uint32_t* expNo_dev,
                         double effort, float* dispatch_dev, uint32_t* count_dev);

/* ---- decode-loop glue around the multiplies (runNetwork.swift:68-316) -----------------------------
 * The callers either side of the hot path: what a token step does between two expertMul calls.  The token position
 * and the token id live in DEVICE memory (pos_dev, id_dev), so a whole token step can be replayed from one hipGraph.
 * All vectors f32 on the device (VectorFloat), norm weights / embeddings f16. */

/* h += delta (delta may be NULL); out = h / sqrt(mean(h^2) + 1e-5) * w -- rmsNormFast + mul(by:) + add(by:)
 * (aux.metal:113-152,268-274; runNetwork.swift:121-122,170-173). */
EFFORT_API int effort_add_rmsnorm_mul(effort_ctx* ctx, float* h_dev, const float* delta_dev, const void* w_f16_dev, float* out_dev, int n);
/* rope_mx on q and on k, repeat4x32 of k and v over the query heads, stored at cache row *pos_dev
 * (runNetwork.swift:128-149, aux.metal:218-261, createFreqsCis2 model.swift:693-717; caches f32 [maxTokens][numHeads][headDim]). */
EFFORT_API int effort_rope_kv(effort_ctx* ctx, const float* xq_dev, const float* xk_dev, const float* xv_dev, float* q_out_dev,
                   float* k_cache_dev, float* v_cache_dev, const uint32_t* pos_dev, int numHeads, int numHeadsKV, int headDim,
                   int maxTokens, float ropeBase);
/* calcScores (/sqrt(headDim)) + softmax + sumScores over tokens 0..*pos_dev (runNetwork.swift:151-163, aux.metal:185-198,379-447). */
EFFORT_API int effort_attention(effort_ctx* ctx, const float* q_dev, const float* k_cache_dev, const float* v_cache_dev,
                     const uint32_t* pos_dev, float* out_dev, int numHeads, int headDim, int maxTokens);
/* effort_rope_kv + effort_attention in one launch (one workgroup per query head; the newest token is attended from LDS). */
EFFORT_API int effort_rope_attention(effort_ctx* ctx, const float* xq_dev, const float* xk_dev, const float* xv_dev, float* k_cache_dev,
                          float* v_cache_dev, const uint32_t* pos_dev, float* out_dev, int numHeads, int numHeadsKV, int headDim,
                          int maxTokens, float ropeBase);
/* silu(x1, x3, out:) = x3 * x1 / (1 + exp(-x1)) (matrix.metal:25-35). */
EFFORT_API int effort_silu_mul(effort_ctx* ctx, const float* x1_dev, const float* x3_dev, float* out_dev, int n);
/* tokEmbeddings.fetchRow(id, out:) (aux.metal:355): row *id_dev of an f16 [vocab][n] table as f32. */
EFFORT_API int effort_fetch_row(effort_ctx* ctx, const void* emb_f16_dev, const uint32_t* id_dev, float* out_dev, int n);
/* Mixtral routing (runNetwork.swift:185-199): idx2_dev = the two largest gate logits' experts (mpsTopK(topK: 2)),
 * val2_dev = softmax over those two logits; effort_mix2: out = f0 * val2[0] + f1 * val2[1]. */
EFFORT_API int effort_top2_softmax(effort_ctx* ctx, const float* gate_dev, int n, uint32_t* idx2_dev, float* val2_dev);
EFFORT_API int effort_mix2(effort_ctx* ctx, const float* f0_dev, const float* f1_dev, const float* val2_dev, float* out_dev, int n);
/* Mixtral routing in ONE launch (runNetwork.swift:173-175,185-189): x = h / sqrt(mean(h^2) + 1e-5) * norm_w; gate[e] = sum f16(x) * gate[e][.]
 * (exact f16 products, f32 sums; gate f16 [numExperts][n]); idx2_dev = the two largest logits' experts (strict >, lowest index first; with
 * numExperts == 1 expert 0 is picked twice with the weights 0.5 / 0.5, as effort_top2_softmax writes them), val2_dev = softmax over
 * those two.  Bit for bit what effort_add_rmsnorm_mul(h, NULL, norm_w, x) ->
 * effort_dense_gemv(gate, x, logits) on the in-tree kernel -> effort_top2_softmax write in a row; h is not modified.  gate_out_dev
 * (may be NULL) receives the numExperts logits, for tests and debugging.  n % 16 == 0, 16 <= n <= 16384, 1 <= numExperts <= 64;
 * anything else returns EFFORT_ERR_SHAPE with nothing enqueued. */
EFFORT_API int effort_moe_route(effort_ctx* ctx, const float* h_dev, const void* norm_w_f16_dev, const void* gate_f16_dev, int n, int numExperts,
                     float* gate_out_dev, uint32_t* idx2_dev, float* val2_dev);
/* h[i] = h[i] + (f0[i] * val2[0] + f1[i] * val2[1]): effort_mix2 and the residual add of the following effort_add_rmsnorm_mul in one
 * launch, bit for bit (runNetwork.swift:190-199). */
EFFORT_API int effort_mix2_add(effort_ctx* ctx, float* h_dev, const float* f0_dev, const float* f1_dev, const float* val2_dev, int n);
/* greedy pick: *id_out_dev = argmax(logits) (the reference takes mpsTopK[0], helpers/mps.swift:52-84); if history_dev is
 * given, history_dev[*pos_dev] = the pick; then *pos_dev += 1. */
EFFORT_API int effort_argmax(effort_ctx* ctx, const float* logits_dev, int n, uint32_t* id_out_dev, uint32_t* pos_dev, uint32_t* history_dev,
                  int historyLen);
/* The position lives in device memory, so the glue cannot refuse a step with a return code: a step at *pos_dev >= maxTokens
 * (effort_rope_kv, effort_rope_attention) or >= historyLen (effort_argmax) writes NOTHING to the cache / history and raises
 * bit 0 of the context's decode status; an argmax over NaN logits returns token 0 and raises bit 1.  Reads and clears it. */
EFFORT_API int effort_decode_status(effort_ctx* ctx, int* host_out);

/* ---- prompt prefill: a block of tokens shares one pass over the weights -------------------------
 * The token step streams every matrix once per token.  These entry points take a BLOCK of 1 .. EFFORT_PREFILL_MAX_ROWS tokens: row r of
 * every operand is token r of the block, rows contiguous.  pos0 and rows are HOST values -- prefill is eager and is never captured into
 * a graph --, so every refusal is a return code with nothing enqueued and the decode status is not involved.  The argument VALUES are
 * judged before the pointers (rows outside 1 .. 64, pos0 < 0, pos0 + rows > maxTokens, a dimension < 1: EFFORT_ERR_ARG; a shape the
 * kernels do not serve: EFFORT_ERR_SHAPE; then a null pointer: EFFORT_ERR_ARG), and the lanes are joined before anything is launched. */
#define EFFORT_PREFILL_MAX_ROWS 64

/* out[r] = W * f16(x[r]) for r < rows: basicMul (helpers/mps.swift:14-47) for a block -- x rounded to f16 once, exact f16 products, f32
 * sums -- on v_mfma_f32_16x16x32_f16; W f16 [outDim][inDim] row-major as effort_dense_gemv takes it, x f32 [rows][inDim], out f32
 * [rows][outDim].  The weights are read once per call, whatever rows is.  inDim % 32 == 0, inDim <= 65536, 1 <= outDim <= 2^24, W below 4 GiB;
 * anything else returns EFFORT_ERR_SHAPE (the caller falls back to effort_dense_gemv row by row).
 * CONTRACT: row r of out depends on row r of x and on W only -- not on rows, not on the other rows, not on r: its bits are the same
 * for every rows and every row position (the order of the sums over k is fixed).  Token columns past rows are zero operands: no x row
 * at or beyond rows is read, no out element at or beyond rows * outDim is written.  It agrees with effort_dense_gemv to rounding of
 * the f32 sums, not bit for bit (another order).  Uses context scratch shared with effort_bucket_gemm_rows alone: 64 * inDim halves
 * for f16(x) and splits * 64 * outDim floats for the partial sums of its k split (splits <= 16, a function of the shape).  Both only
 * grow: a call that needs more than there is synchronises the stream, frees and allocates.  The entry point is meant to be called
 * eagerly.  A captured graph that holds it keeps the scratch addresses of its capture, so it stays valid only if no later call grows
 * either buffer: before capturing, call it eagerly with 64 rows once for EVERY (inDim, outDim) pair the context will ever see.
 * Up to three launches: convert, multiply, and the reduce when the shape has more than one split. */
EFFORT_API int effort_dense_gemm_rows(effort_ctx* ctx, const void* W_f16_dev, const float* x_dev, float* out_dev, int inDim, int outDim, int rows);
/* The ROUTED block multiply (a Mixtral block): W f16 [numExperts][outDim][inDim], one expert's matrix as effort_dense_gemm_rows takes it.
 * Assignment a = 2 r + s (token r < rows, slot s of its top-2) multiplies expert e = min(idx2_dev[a], numExperts - 1) -- the clamp of
 * effort_dense_gemv_expert: a device value cannot be refused by a return code.  Its input row is x[r] when xPerSlot == 0 (w1 / w3: both
 * slots read the token's normed state; x f32 [rows][inDim]) and x[a] when xPerSlot == 1 (w2: a gated vector per slot; x f32
 * [2 * rows][inDim]); out[a] = W[e] * f16(input), out f32 [rows][2][outDim].
 * The assignments are grouped by expert on the device, in assignment order (the expert numbers never reach the host); an expert's
 * workgroups stream its matrix ONCE for all its token columns (64 columns a walk: 65 .. 128 assignments on one expert, which only
 * duplicates or clamping produce, walk it again), and an expert nobody picked is not read.
 * CONTRACT: out[a] is BIT FOR BIT what effort_dense_gemm_rows(ctx, W + e * outDim * inDim, input, ., inDim, outDim, 1) writes: the
 * same k split, the same order of the sums, zero operands for dead columns.  So it depends on the input row and W[e] alone -- not on
 * rows, not on a, not on who else picked e.  No x row and no idx2 entry at or past rows (xPerSlot == 1: x rows past 2 * rows) is read;
 * nothing outside out[0 .. 2 * rows * outDim) is written.
 * Shapes: one expert's (inDim, outDim) as effort_dense_gemm_rows serves them (ONE expert below 4 GiB: the stack may be larger),
 * numExperts <= 64; anything else returns EFFORT_ERR_SHAPE (the caller falls back to effort_dense_gemv_expert per assignment).
 * xPerSlot other than 0 / 1, numExperts < 1: EFFORT_ERR_ARG.  The weight stream is nt when ONE expert's matrix is above 64 MiB.
 * Uses context scratch shared with effort_bucket_gemm_rows_routed alone: 128 * inDim halves for f16(x), splits * 128 * outDim floats for
 * the partial sums of the k split, and 64 * 129 words for the groups.  The first two only grow, by effort_dense_gemm_rows's rule, and the
 * same advice holds before capturing.  Up to three launches: convert + group, multiply, and the reduce when the shape has more than
 * one split. */
EFFORT_API int effort_dense_gemm_rows_routed(effort_ctx* ctx, const void* W_f16_dev, int numExperts, const uint32_t* idx2_dev, const float* x_dev,
                                  int xPerSlot, float* out_dev, int inDim, int outDim, int rows);
/* ---- prefill straight from the bucketed weights: no f16 core ------------------------------------
 * At percentLoad 16 an FP16 bundle's buckets hold the whole matrix, so the f16 core a prefill would read is a second copy.  These
 * entry points multiply a block by the UN-BUCKETED matrix U of a registered handle, un-bucketing on the fly:
 *   for expert e, input j, bucket column c and rank r let w be the 16-bit entry buckets[e][r * inDim + j][c].  w == 0x0000 is
 *   skipped; otherwise U[e][16 c + (w & 15)][j] = w -- the position bits STAY in the value, exactly as bucketMul multiplies them
 *   (bucketMul.metal:100-102); elements no entry names are +0.
 * A bundle is UN-BUCKETABLE iff no two non-skipped entries of one (e, j, c) name the same position.  The converter's fast path
 * always writes such bundles; its literal preBucketize path (zero padding of a non-power-of-two row, effort_convert_status reports
 * drops) can write collisions, and those bundles are refused (EFFORT_ERR_CONVERT), never guessed at.
 * U is the core with its low four mantissa bits replaced by positions: a prefill through these calls writes the K / V a decode at
 * effort 1.0 would write (up to the order of the sums and the f16(x) rounding), NOT the dense path's K / V.
 *
 * effort_weights_bucket_dense_ok: *host_out = 1 when the handle is un-bucketable, 0 when not.  One small kernel over the buckets;
 * synchronises.  The answer is cached on the handle; effort_weights_refresh clears it (the next call looks again).  The multiplies
 * below run it themselves on a handle's first use.  EFFORT_ERR_KIND for a Q4 handle, EFFORT_ERR_SHAPE as below.
 *
 * effort_bucket_gemm_rows: out[r] = U[expert] * f16(x[r]) for r < rows, x f32 [rows][inDim], out f32 [rows][outDim].
 * CONTRACT: BIT FOR BIT what effort_dense_gemm_rows writes when U[expert] is given to it as W (the same k split, the same order of
 * the sums, the same operand slots on v_mfma_f32_16x16x32_f16, zero operands for dead token columns and for k past inDim); so that
 * entry's contract holds here word for word -- row r of out depends on row r of x and on U alone, no x row at or beyond rows is
 * read, nothing at or beyond rows * outDim is written.  A bucket row is read only inside its 2 * outDim / 16 payload bytes (the pitch
 * padding may hold anything), other experts' buckets are not read, and any row pitch registration accepts is served.  The bucket
 * stream is nt when one expert's matrix is above 64 MiB.
 *
 * effort_bucket_gemm_rows_routed: effort_dense_gemm_rows_routed on the handle's expert stack (numExperts, inDim, outDim are the
 * handle's): out[a] = U[min(idx2_dev[a], numExperts - 1)] * f16(input of a), BIT FOR BIT what effort_bucket_gemm_rows writes for that
 * input row and expert alone with rows = 1.  Expert e's bucket rows start at row 16 * inDim * e; an expert nobody picked is not read;
 * an expert's columns are walked 64 at a time.
 *
 * Refusals, nothing enqueued on any of them, values before pointers: rows outside 1 .. 64, expert outside 0 .. numExperts - 1,
 * xPerSlot other than 0 / 1, a NULL handle: EFFORT_ERR_ARG; a Q4 handle: EFFORT_ERR_KIND; percentLoad != 16, a column shard,
 * inDim % 32 != 0, routed with numExperts > 64: EFFORT_ERR_SHAPE; then a NULL pointer (or a context other than the handle's):
 * EFFORT_ERR_ARG; then, the lanes joined, a bundle that is not un-bucketable: EFFORT_ERR_CONVERT (on a handle's first use this runs
 * the check, which writes a status word of the context and nothing else).
 * SCRATCH: effort_bucket_gemm_rows uses effort_dense_gemm_rows's context scratch and effort_bucket_gemm_rows_routed uses
 * effort_dense_gemm_rows_routed's (the sizes are the same; the calls are eager on one stream, so neither finds the other's data in
 * use); the growth rule and the advice before capturing are those entries'.  Up to three launches each, as their core twins. */
EFFORT_API int effort_weights_bucket_dense_ok(effort_w* w, int* host_out);
EFFORT_API int effort_bucket_gemm_rows(effort_ctx* ctx, const effort_w* w, int expert, const float* x_dev, float* out_dev, int rows);
EFFORT_API int effort_bucket_gemm_rows_routed(effort_ctx* ctx, const effort_w* w, const uint32_t* idx2_dev, const float* x_dev, int xPerSlot,
                                   float* out_dev, int rows);
/* Prompt prefill straight from the Q4 buckets (csrc/prefill_q4.hip): the Q4 twins of the two plain entry points above, so that a Q4
 * model prefills with no f16 core of a Q4 bundle in memory.  The matrix U4 of a registered Q4 handle:
 *   bucket row i = 8 j + r of expert e holds rank r of input j, outDim / 32 16-bit words; word x holds four nibbles, the first in bits
 *   15 .. 12; nibble n = sign << 3 | pos names output 32 x + 8 n + pos, and U4[e][32 x + 8 n + pos][j] = +-f16(m) with m = stats[i].y
 *   (the second lane of the f32 x 2 stats, what prepareDispatchQ4 reads), a clear sign bit +: a zero weight counts as +m.
 * A Q4 bundle is UN-BUCKETABLE iff for every (e, j, x, n) the eight ranks name eight different positions and every stats[i].y is a
 * finite f16 number stored as f32; every element of U4 is then named exactly once.  The converter always writes such bundles;
 * others are refused (EFFORT_ERR_CONVERT), never guessed at.  A prefill through these calls writes the K / V a Q4 decode at effort
 * 1.0 would write (up to the order of the sums and the f16(x) rounding), NOT the dense path's.
 *
 * effort_weights_q4_dense_ok: *host_out = 1 when the handle is un-bucketable, 0 when not.  One kernel over the buckets and lane .y
 * of the stats, which also writes the handle's compact f16 copy of the means (what the multiply reads); synchronises.  The answer is
 * cached on the handle; effort_weights_refresh clears it.  The multiply runs it itself on a handle's first use.
 *
 * effort_q4_gemm_rows: out[r] = U4[expert] * f16(x[r]) + sum over the handle's outliers k on that output of val_k * x[r][in_k], for
 * r < rows, x f32 [rows][inDim], out f32 [rows][outDim].  CONTRACT: for a handle without outliers BIT FOR BIT what
 * effort_dense_gemm_rows writes when U4[expert] is given to it as W, so that entry's contract holds word for word.  The outlier term
 * uses the f32 x (calcOutliers, bucketMulQ4.metal:13-21) and is added to the product in f32, one fmaf per outlier in the order of the
 * handle's outlier index (an output's entries in table order): a function of the handle and of row r alone, never of rows.  A bucket
 * row is read only inside its outDim / 16 payload bytes, lane .y of the stats only through the compact copy, other experts' rows not
 * at all.  One more launch than effort_bucket_gemm_rows when the handle has outliers, none otherwise.
 *
 * Refusals, nothing enqueued on any of them, values before pointers: rows outside 1 .. 64, expert outside 0 .. numExperts - 1, a NULL
 * handle: EFFORT_ERR_ARG; an FP16 handle: EFFORT_ERR_KIND; a column shard, inDim % 32 != 0, a shape effort_dense_gemm_rows refuses:
 * EFFORT_ERR_SHAPE; then a NULL pointer (or a context other than the handle's): EFFORT_ERR_ARG; then, the lanes joined, a bundle that
 * is not un-bucketable: EFFORT_ERR_CONVERT.  SCRATCH: effort_dense_gemm_rows's.  No routed form: the reference writes no Q4 Mixtral
 * model.  effort_weights_bucket_dense_ok and effort_bucket_gemm_rows keep answering EFFORT_ERR_KIND for Q4 handles. */
EFFORT_API int effort_weights_q4_dense_ok(effort_w* w, int* host_out);
EFFORT_API int effort_q4_gemm_rows(effort_ctx* ctx, const effort_w* w, int expert, const float* x_dev, float* out_dev, int rows);
/* Block forms of the Mixtral glue, per row BIT FOR BIT the token forms (the same body):
 * effort_moe_route_rows: effort_moe_route on row r of h [rows][n]; idx2 / val2 [rows][2], gate_out (may be NULL) [rows][numExperts].
 * effort_mix2_add_rows: effort_mix2_add on row r of h [rows][n] with f0 = f[r][0], f1 = f[r][1] (f f32 [rows][2][n]) and val2[r]. */
EFFORT_API int effort_moe_route_rows(effort_ctx* ctx, const float* h_dev, const void* norm_w_f16_dev, const void* gate_f16_dev, int n, int numExperts,
                          float* gate_out_dev, uint32_t* idx2_dev, float* val2_dev, int rows);
EFFORT_API int effort_mix2_add_rows(effort_ctx* ctx, float* h_dev, const float* f_dev, const float* val2_dev, int n, int rows);
/* Block forms of the glue: per row, BIT FOR BIT what the single-token entry point writes (the same sums in the same order).
 * effort_fetch_rows: out[r] = row ids_dev[r] of the table (effort_fetch_row).
 * effort_add_rmsnorm_mul_rows: effort_add_rmsnorm_mul on row r of h, delta (may be NULL) and out; one norm weight vector.
 * effort_rope_kv_rows: effort_rope_kv with row r roped at position pos0 + r; cache rows pos0 .. pos0 + rows - 1 are written, no other.
 *   xq f32 [rows][numHeads * headDim], xk / xv f32 [rows][numHeadsKV * headDim], q_out as xq.  Head geometry as effort_rope_kv.
 * effort_attention_rows: row r is effort_attention at position pos0 + r: it attends over cache rows 0 .. pos0 + r (causal inside the
 *   block) and reads no cache row beyond.  A grid of (numHeads, rows) workgroups; every query reads its keys and values from the cache
 *   again.  It needs the block's effort_rope_kv_rows to have completed: enqueue both on the context's stream.  Head geometry as
 *   effort_attention. */
EFFORT_API int effort_fetch_rows(effort_ctx* ctx, const void* emb_f16_dev, const uint32_t* ids_dev, float* out_dev, int n, int rows);
EFFORT_API int effort_add_rmsnorm_mul_rows(effort_ctx* ctx, float* h_dev, const float* delta_dev, const void* w_f16_dev, float* out_dev, int n, int rows);
EFFORT_API int effort_rope_kv_rows(effort_ctx* ctx, const float* xq_dev, const float* xk_dev, const float* xv_dev, float* q_out_dev,
                        float* k_cache_dev, float* v_cache_dev, int pos0, int rows, int numHeads, int numHeadsKV, int headDim,
                        int maxTokens, float ropeBase);
EFFORT_API int effort_attention_rows(effort_ctx* ctx, const float* q_dev, const float* k_cache_dev, const float* v_cache_dev, int pos0, int rows,
                          float* out_dev, int numHeads, int headDim, int maxTokens);
/* effort_attention_block: what effort_attention_rows computes -- out[r] = softmax(q[r] . K[t] / sqrt(headDim)) . V[t] over cache rows
 * t = 0 .. pos0 + r, causal inside the block --, with the block's queries SHARING each K / V row that is fetched: a workgroup is one
 * head and 16 queries and walks the keys in tiles of 16 with an online softmax (running max, running sum, a [16 x headDim]
 * accumulator), both products on the f32-input MFMA (v_mfma_f32_16x16x4_f32), f32 end to end.  A fetched K / V
 * tile serves 16 queries, so it asks for a sixteenth of effort_attention_rows's K / V bytes, and its LDS does not grow with the position.
 * Arguments, layouts and refusals (same codes, same order, nothing enqueued) are effort_attention_rows's, one for one; eager only.
 * BAR: every output element is within 2e-5 * max|row| of the float64 value, cosine >= 0.999999 (tests/test_gpu_attention_block.py).
 * Its BITS DIFFER from effort_attention / effort_attention_rows: another order of the sums.
 * ORDER OF THE SUMS: it follows the absolute position only.  Key tiles sit on multiples of 16 counted from token 0, the wave that
 * owns a tile follows from the tile's absolute index, partial states merge in a fixed order, and a key a query may not see is
 * selected out (never multiplied by zero), so a wholly masked tile is an exact no-op.  An output row's bits are a function of the
 * query, its absolute position pos0 + r and cache rows 0 .. pos0 + r: not of pos0, rows or r on their own.
 * No cache row at or past pos0 + rows and no q row at or past rows is read (they may hold NaN); nothing outside out[0 .. rows) is
 * written.  It needs the block's effort_rope_kv_rows to have completed: enqueue both on the context's stream. */
EFFORT_API int effort_attention_block(effort_ctx* ctx, const float* q_dev, const float* k_cache_dev, const float* v_cache_dev, int pos0, int rows,
                           float* out_dev, int numHeads, int headDim, int maxTokens);

/* ---- sampled pick: top-k / top-p / temperature on the device ------------------------------------ */

/* The settings of effort_sample live in DEVICE memory (a token step is captured once into a hipGraph and graphs are kept for the
 * life of the process: a value in the kernel arguments would need a graph per seed or temperature).  32 bytes, little endian, no
 * padding.  The host cannot validate device values, so the kernel sanitises them: top_k is clamped to [1, min(64, n)];
 * temperature <= 0 or not finite means the pick is the largest logit (greedy); top_p outside (0, 1] is treated as 1. */
#define EFFORT_SAMPLE_MAX_K 64
typedef struct effort_sample_params {
    float temperature;
    float top_p;
    uint32_t top_k;
    uint32_t seed_lo;             /* Philox key = (seed_lo, seed_hi) */
    uint32_t seed_hi;
    uint32_t stream;              /* counter word 1: independent sequences under one seed */
    uint32_t reserved[2];
} effort_sample_params;

/* Takes effort_argmax's place in a sampled token step (one launch of one workgroup).
 *  1. The K = top_k largest logits, sorted by value descending, lowest index first among equal values (-0.0 == +0.0; NaN is never
 *     selected; -inf is an ordinary value) -- the reference's mpsTopK (helpers/mps.swift:49-80).  If topk_idx_dev / topk_val_dev are given
 *     (either may be NULL) they receive the K indices and values (the logits as stored); entries past the number of non-NaN
 *     logits get 0xFFFFFFFF / -inf.
 *  2. One lane, f32, in rank order: w_j = expf((v_j - v_0) / temperature), running sums c_j; the nucleus is the shortest prefix with
 *     c_j >= top_p * c_{K-1}, its mass S; the pick is the smallest j of the nucleus with c_j > u * S, or its last entry if rounding leaves
 *     none.  An infinite v_0 picks rank 0.
 *  3. u = (x0 >> 8) * 2^-24, x0 = word 0 of Philox4x32-10 at counter (*pos_dev, stream, 0, 0) under key (seed_lo, seed_hi)
 *     (effort_sample_bits): a replayed graph draws anew at every position, a run is reproducible from its seed.
 *  4. What effort_argmax writes: *id_out_dev, history_dev[*pos_dev] (or decode status bit 0 past historyLen), *pos_dev += 1; every logit
 *     NaN: token 0 and status bit 1.  With top_k = 1 or a greedy temperature the result is effort_argmax's, bit for bit. */
EFFORT_API int effort_sample(effort_ctx* ctx, const float* logits_dev, int n, const effort_sample_params* params_dev, uint32_t* id_out_dev,
                  uint32_t* pos_dev, uint32_t* history_dev, int historyLen, uint32_t* topk_idx_dev, float* topk_val_dev);
/* mpsTopK(v:topK:) (helpers/mps.swift:49-80): step 1 of effort_sample alone, 1 <= k <= 64 (the reference asks for 16).  idx_dev / val_dev
 * receive k entries; those past the number of non-NaN logits (n < k, or NaN logits) are 0xFFFFFFFF / -inf.  No position, no status. */
EFFORT_API int effort_topk(effort_ctx* ctx, const float* logits_dev, int n, int k, uint32_t* idx_dev, float* val_dev);
/* Host only -- no context, no HIP call: x0 of the draw at (seed, stream, pos), from the same definition the kernel compiles. */
EFFORT_API uint32_t effort_sample_bits(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t pos);

/* ---- generation rules: penalties, bias, min-p, stop tokens on the device ------------------------ */

/* The settings of effort_logit_rules live in DEVICE memory, for effort_sample_params' reason: one captured graph serves every
 * setting.  64 bytes, little endian, no padding.  The host cannot validate device values, so the kernel sanitises them (step 0). */
#define EFFORT_RULES_MAX_WINDOW 1024
#define EFFORT_RULES_MAX_BIAS   256
#define EFFORT_RULES_MAX_STOP   8
typedef struct effort_rules_params {
    float    repetition_penalty;       /* 1 = off */
    float    presence_penalty;         /* 0 = off */
    float    frequency_penalty;        /* 0 = off */
    float    min_p_log;                /* f32(ln(min_p)) computed by the HOST; -inf = off */
    uint32_t last_n;                   /* window length, 0 = no penalties */
    uint32_t n_bias;
    uint32_t n_stop;
    uint32_t first_pos;                /* positions below it never stop (the prompt) */
    uint32_t stop_ids[EFFORT_RULES_MAX_STOP];
} effort_rules_params;

/* One launch of one workgroup between the LM head and the pick (effort_argmax / effort_sample) of a token step: logits_out_dev
 * receives the n logits of logits_in_dev with the rules applied.  Every arithmetic step is ONE float32 operation rounded on its own
 * (no fused multiply-add, a correctly rounded divide).  pos = *pos_dev is read and never advanced (the pick advances it);
 * tok = *tok_dev is the token this step consumed.
 *  0. Sanitise.  repetition_penalty not finite or <= 0 counts as 1; presence_penalty / frequency_penalty not finite as 0; last_n,
 *     n_bias, n_stop are clamped to the three maxima; min_p_log is active only when finite and <= 0; a bias entry whose value is NaN
 *     is absent; token ids >= n are ignored, in the window and in the bias table alike.
 *  1. Record.  If tok_dev and seq_dev are given: pos < seqLen: seq[pos] = tok.  Otherwise nothing is written, the window is empty
 *     and bit 0 of the context's decode status is raised (the meaning it has for the cache and the history).  Without them the
 *     window is empty.
 *  2. Stop.  If stop_pos_dev is given, pos >= first_pos, tok is among stop_ids[0 .. n_stop) and *stop_pos_dev == 0xFFFFFFFF:
 *     *stop_pos_dev = pos (the stop token was picked at step pos - 1; only the first stop is recorded; no status bit).
 *  3. Copy.  out = in.  logits_out_dev == logits_in_dev is allowed and gives the same bits.
 *  4. Penalties.  W = min(last_n, pos + 1), the window is seq[pos + 1 - W .. pos], c the number of times token t occurs in it.
 *     Each distinct t of the window once: l = out[t]; if repetition_penalty != 1: l = l > 0 ? l / repetition_penalty
 *     : l * repetition_penalty (the rule of HF RepetitionPenaltyLogitsProcessor and of llama.cpp); l = l - (f32(c) *
 *     frequency_penalty + presence_penalty), two rounded operations and then the subtraction.
 *  5. Bias.  out[id] = out[id] + val; for an id named more than once the (present) entry with the highest index is the one
 *     applied; val = -inf bans a token.
 *  6. Min-p.  m = the largest non-NaN element of out.  If the rule is active and m is finite: thr = m + min_p_log, every
 *     element < thr becomes -inf; NaN elements stay.  It acts on the ruled logits at temperature 1: effort_sample's temperature,
 *     top-k and top-p come after it, on out.
 * NaN: a NaN logit passes steps 4 and 5 with its bits unchanged, and a NaN that their arithmetic makes of other values (inf - inf) is
 * stored as 0x7FC00000.  With every rule off, out is in bit for bit, NaN payloads and -0.0 included.
 * Refusals (EFFORT_ERR_ARG, nothing enqueued): n < 1 or seqLen < 0; then a NULL among logits_in_dev, logits_out_dev, params_dev,
 * pos_dev; exactly one of tok_dev / seq_dev or of bias_ids_dev / bias_vals_dev.  Without the bias tables n_bias counts as 0;
 * stop_pos_dev may be NULL, and stop reporting needs tok_dev. */
EFFORT_API int effort_logit_rules(effort_ctx* ctx, const float* logits_in_dev, int n, const effort_rules_params* params_dev,
                                  const uint32_t* tok_dev, const uint32_t* pos_dev, uint32_t* seq_dev, int seqLen,
                                  const uint32_t* bias_ids_dev, const float* bias_vals_dev, uint32_t* stop_pos_dev, float* logits_out_dev);

/* ---- weight layout converter ------------------------------------------------------------------- */

/* func bucketize(_:outTensorsPref:tensors:goQ8:false) -- convert.swift:209-260 with kernels getProbes,
 * prepareValsIdxs, idxsBitonicSortAbs, preBucketize, bucketize, makeStats (convert.metal:14-119,
 * 315-342).  W_f16_dev is the HF matrix [outDim, inDim]; outputs as in effort_weights_fp16 with
 * percentLoad 16, one expert.  Runs on the GPU (all device pointers), enqueued on the stream. */
EFFORT_API int effort_convert_fp16(effort_ctx* ctx, const void* W_f16_dev, int outDim, int inDim,
                        void* buckets_dev, void* stats_dev, void* probes_dev);
/* The same, writing bucket rows `rowPitchBytes` apart (0 = dense; otherwise a multiple of 8 bytes >= 2*outDim/16 -- the stats pass
 * reads 8 bytes at a time; see effort_weights_fp16_pitched; the padding is left untouched). */
EFFORT_API int effort_convert_fp16_pitched(effort_ctx* ctx, const void* W_f16_dev, int outDim, int inDim,
                                void* buckets_dev, int rowPitchBytes, void* stats_dev, void* probes_dev);
/* Elements the last effort_convert_fp16 calls could not place: the reference's preBucketize (convert.metal:40-61) drops an
 * element whose bucket is already full, which happens when zero padding of a non-power-of-two row ties with real zeros;
 * the converter reproduces that and counts the drops here.  Reads and clears the count (0 = every element was placed). */
EFFORT_API int effort_convert_status(effort_ctx* ctx, int* host_out);

/* q4_draft.convert(core2) (q4_draft.py:70-322; driver q4_convert.py:41-81) for one matrix, on the GPU.  core2_f16_dev is
 * W.T: f16 [inDim][outDim], outDim % 32 == 0.  Outputs (device buffers of the caller): buckets u16 [inDim*8][outDim/32],
 * stats f32 [inDim*8][2], probes f16 [min(inDim, outDim)] (the diagonal after outlier removal), outliers f32 [n][4] =
 * (value, inIdx, outIdx, 0) with n = effort_q4_outlier_count(inDim, outDim, perc) = int(inDim*outDim*perc), ordered by |w|
 * descending, flat index ascending on ties (the reference's unstable argsort leaves ties unspecified).  Bit-identical to
 * the reference's outputs (tests/golden/q4_*.npz).  Synchronises the stream; allocates its scratch (4*inDim*outDim bytes
 * + the sort's) for the duration of the call. */
EFFORT_API int64_t effort_q4_outlier_count(int inDim, int outDim, double perc);
EFFORT_API int effort_convert_q4(effort_ctx* ctx, const void* core2_f16_dev, int inDim, int outDim, double perc, void* buckets_dev,
                      void* stats_dev, void* probes_dev, void* outliers_dev);

/* VectorFloat.cosineSimilarityTo (model.swift:511-519; aux.metal:293-312).  Synchronises. */
EFFORT_API int effort_cosine(effort_ctx* ctx, const float* a_dev, const float* b_dev, int n, float* host_out);

/* Tuning knobs, profiling, tracing and ablation hooks live in effort_hip_debug.h: they are not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif /* EFFORT_HIP_H */
