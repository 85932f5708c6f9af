/* C-ABI of libltu_hip.so — the MI355X (gfx950) kernels behind the LinTransUNet hot path.
 *
 * The reference (freshman97/LinTransUNet) is pure PyTorch and has no FFI of its own; each entry
 * point below replaces the ATen op(s) reached from the cited reference lines (paths relative to
 * the reference root).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - Activations are channels-last: a reference tensor [B,C,H,W,D] lives in HBM as [B,H,W,D,C]
 *     (C fastest), so a voxel is a token and 1x1x1 convs / Linear layers are the same GEMM.
 *   - `dtype` is the storage type of activations (LTU_F32 / LTU_BF16); weights, statistics,
 *     probabilities and gradients of weights are fp32; all accumulation is fp32.
 *   - Ownership: the caller allocates every buffer (outputs, workspaces, saved statistics).  The
 *     library never allocates, frees, retains pointers or synchronises; all work is enqueued on
 *     `stream`.  Entry points keep no state between calls and may be called from several threads
 *     (one process per GPU is the intended use).  The only process-global data are (a) the tuning
 *     knob table of ltu_config_set (mutex-protected; knobs are looked up per call: override, then
 *     the environment variable of the same name, then the default) and (b) per-device "dynamic
 *     LDS limit raised" latches for five kernels (atomic bit masks).
 *   - Dropout: (p, seed) select a counter-based hash mask (a murmur3 finalizer + a linear expansion to 64 bits per
 *     4-element group, csrc/common.h); the backward entry points regenerate
 *     the mask from the same (p, seed) instead of reading a stored one.  Independence: the four keep decisions of a group are
 *     PAIRWISE independent only (every pair of the four 16-bit words is a full-rank GF(2) image of the 32-bit hash; the third and
 *     fourth word are deterministic functions of the first two), not 4-wise independent like nn.Dropout's Bernoulli draws; groups
 *     are independent of each other.  tests/test_gpu_ops.py::test_dropout_group_pattern_histogram holds the joint 16-pattern
 *     histogram of a group against Bernoulli^4.  p = 0 disables.  `step` (nullable) is a
 *     device-resident counter mixed into the seed at run time, so a captured HIP graph draws fresh masks per replay.
 *   - Workspaces: every entry point that takes a caller-owned workspace / scratch buffer also takes its CAPACITY (the argument
 *     right behind the pointer, in floats unless it says elements) and returns LTU_E_ARG WITHOUT launching anything when the
 *     geometry it is about to launch needs more.  The *_ws_floats() queries tell what a call needs; launch geometry may depend on
 *     tuning knobs (ltu_config_set / environment), so a query and a launch made under different knob values can disagree - the
 *     capacity check turns that into an error code instead of a write past the end.  The two entry points whose width the caller
 *     chooses per launch (ltu_linear_wgrad_group, ltu_upconv_wgrad) take that width as an argument of both the query and the launch.
 *   - Return value: 0 = LTU_OK, negative = LTU_E_* argument error, positive = hipError_t.
 */
#ifndef LTU_HIP_H
#define LTU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ltu_stream_t; /* hipStream_t */

enum { LTU_F32 = 0, LTU_BF16 = 1 };
enum { LTU_OK = 0, LTU_E_DTYPE = -1, LTU_E_SHAPE = -2, LTU_E_ALIGN = -3, LTU_E_ARG = -4,
       LTU_E_COMM = -100 /* RCCL not loaded / not loadable; LTU_E_COMM - r = RCCL returned ncclResult_t r > 0 */ };
enum { LTU_ACT_NONE = 0, LTU_ACT_LRELU = 1 };

int ltu_version(void);
/* bit 0: built with -DLTU_EXPERIMENTS (kernel variants that lost their measurements and ltu_selftest_last_arriver are compiled in) */
int ltu_build_flags(void);
/* Tuning / ablation knobs (grid sizes, split counts, kernel-variant switches; names = the LTU_* environment variables
 * listed in DESIGN.md).  Sets (clear = 0) or removes (clear != 0) a process-wide override that takes precedence over
 * the environment.  Results never depend on a knob beyond fp32 summation order.  Used by the tests to force code
 * paths (e.g. several tiles per split in the linear-attention reductions at small N). */
int ltu_config_set(const char* name, int value, int clear);
/* Self-test of the cross-lane reductions every norm / softmax / loss kernel builds on (DPP + v_permlane16/32_swap, common.h):
 * sum[i] / mx[i] = sum / max of x over the aligned group of G lanes (G = 2 .. 64, a power of two) that holds element i; n is a
 * multiple of 64.  Exists because the permlane-swap builtins of hipcc 7.2 miscompile (tests/test_gpu_ops.py keeps the inline-asm
 * replacement honest on the hardware). */
int ltu_selftest_group_reduce(const float* x, float* sum, float* mx, int n, int G, ltu_stream_t s);
#ifdef LTU_EXPERIMENTS      /* exported by an experiments build only (make EXPERIMENTS=1); ltu_build_flags() & 1 tells */
/* Self-test and price of an in-launch "last arriver" fold against the two-stage form the step uses (per-workgroup partial rows + a
 * second small launch): nwg workgroups with uneven load (workgroup i sums 1 + (7 i mod skew) chunks of rows_per_chunk rows of x
 * [rows][n], n <= 256) publish one partial row each; mode 0 folds them with a second launch, mode 1 inside the launch (write-through
 * partials, agent-scope ticket, one acquire by the last arriver: the guide's hand-off recipe R1).  Both fold in the same fixed
 * order, so `out` [n] must be bit-identical.  part: nwg * n floats (pre-read by every workgroup: an L1-warm consumer), counter: one
 * zeroed word (left zero by the last arriver), sink: nwg floats (never written for finite data).  tests/test_gpu_ops.py runs 10^4
 * launches of it in one process; profiles/r03_last_arriver.txt has the timings of both forms. */
int ltu_selftest_last_arriver(const float* x, float* part, float* out, unsigned* counter, float* sink, int nwg, int n,
                              int rows_per_chunk, int skew, int mode, ltu_stream_t s);
#endif

/* ---- window embedding: model/Unet_3Dblock.py:123-136 ------------------------------------------
 * x f32 [B,1,H,W,D] (reference layout) -> y T [B,H/2,W/2,D,8]; channel kh*2+kw, channels 4..7 = 0
 * (padding so that the stem conv gathers whole vectors). */
int ltu_window_embed(const float* x, void* y, int dtype, int B, int H, int W, int D, ltu_stream_t s);
/* K input channels, 1 <= K <= LTU_MAX_INPUT_CHANNELS: x f32 [B,K,H,W,D] -> y T [B,H/2,W/2,D,CP], CP = 8 * ceil(4K / 8) (8 for K = 1, 2;
 * 16 for K = 3, 4); channel 4c + 2kh + kw = x[b][c][2h+kh][2w+kw][d] (the inverse of the reference's windows_unembedding), channels
 * 4K .. CP-1 = 0.  K = 1 writes the bits of ltu_window_embed.  NULL x / y, B < 0 LTU_E_ARG; K outside the range, odd H or W, an
 * extent < 1 LTU_E_SHAPE; both before any launch. */
#define LTU_MAX_INPUT_CHANNELS 4
int ltu_window_embed_multi(const float* x, void* y, int dtype, int B, int K, int H, int W, int D, ltu_stream_t s);

/* ---- weight repacking (weights are tiny; done per step) ----------------------------------------
 * GEMM weight operands are consumed in the activation dtype: these produce them from the fp32 masters.
 * conv weight [Co,Ci,3,3,3] -> wf [CoP][27][CiP] (forward / weight-gradient operand) and/or
 * wd [CiP][27][CoP] (data-gradient operand), zero padded, stored as out_dtype; either output may be NULL. */
int ltu_pack_conv_weight(const float* w, void* wf, void* wd, int Co, int Ci, int CoP, int CiP, int out_dtype, ltu_stream_t s);
/* gradient back to the PyTorch layout: dwf [CoP][27][CiP] -> dw [Co,Ci,3,3,3] */
int ltu_unpack_conv_wgrad(const float* dwf, float* dw, int Co, int Ci, int CiP, ltu_stream_t s);
/* out[c*ldo + col_off + r] = in[r*C + c], stored as out_dtype (Linear weight for the data-gradient GEMM) */
int ltu_transpose_f32(const float* in, void* out, int R, int C, int ldo, int col_off, int out_dtype, ltu_stream_t s);
/* out[i] = (out_dtype) in[i] */
int ltu_cast_f32(const float* in, void* out, long long n, int out_dtype, ltu_stream_t s);
/* All of the above for a whole model in ONE launch.  table: n device-resident 40-byte records
 * { const float* src; void* dst; int kind, R, C, p0, p1, pad; } with kind 0 = cast (R*C elements),
 * 1 = transpose ([R][C] -> dst[c*p0 + p1 + r]), 2 = pack wf ([R=Co][C=Ci][27] -> [p0=CoP][27][p1=CiP]),
 * 3 = pack wd (-> [p1=CiP][27][p0=CoP]), 4 = fp32 copy of R*C elements (padded biases), 5 / 6 = the sub-pixel
 * operands of ltu_upconv_* ([8][CoP][8][CiP] and [CiP][64][CoP]), 7 = pack wd of one member of a fused conv group: columns
 * [off, off+cnt) of dst [p1=CiP][27][p0=stride], pad = off << 16 | cnt (its wf rows are a kind-2 record at a row offset),
 * 8 / 9 = MFMA fragment order of a dense weight [R][C] for the row-block chain kernels (ltu_layer_tail_*): element
 * ((ct * KS + ks) * 64 + lane) * 8 + j = W[ct*32 + lane%32][ks*16 + 8*(lane/32) + j] (kind 8, KS = C/16: outputs = rows) or
 * W[ks*16 + 8*(lane/32) + j][ct*32 + lane%32] (kind 9, KS = R/16: outputs = columns); R*C destination elements. */
int ltu_weight_prep(const void* table, int n, int out_dtype, ltu_stream_t s);
/* The same with the work dealt out in chunks of LTU_WPREP_CHUNK destination elements: chunks = nchunks device-resident
 * { int record; int first_element / LTU_WPREP_CHUNK } pairs (a model has hundreds of records of very different sizes); the grid
 * walks the list, one chunk per workgroup and trip (four for lists of >= 6 000 chunks), at most LTU_WPREP_BLOCKS workgroups wide
 * when that knob is set.  Destination element counts per kind: 0/1/4: R*C; 2/3: p0*27*p1; 5/6: 64*p0*p1; 7: cnt*27*p1. */
#define LTU_WPREP_CHUNK 4096
int ltu_weight_prep_chunks(const void* table, const int* chunks, int nchunks, int out_dtype, ltu_stream_t s);

/* ---- dense projections: nn.Linear (model/trans_block.py:144,156,166,187,189) and 1x1x1 convs
 *      (model/Unet_3Dblock.py:200-215).  y[M,N] (+)= a[M,K] . w[N,K]^T + bias;  w in the activation dtype, bias fp32.
 * Up to three weight blocks of N/nw rows each may be given (q,k,v fused: nw = 3); bias entries may
 * be NULL.  accumulate != 0 adds to y. */
int ltu_linear_fwd(const void* a, int lda, const void* const* w, int nw, const float* const* bias, void* y, int ldy,
                   int M, int N, int K, int accumulate, int dtype, ltu_stream_t s);
/* FFN front half: u [M,N] = a . w^T + bias and h = dropout(gelu(u)) (model/trans_block.py:203-208).  bf16 shapes of the
 * weight-stationary projection kernel get both from one launch (GELU + dropout in its epilogue); otherwise the projection and
 * ltu_gelu_dropout_fwd run back to back with identical results.  ltu_gelu_dropout_bwd(dh, u, ...) is the matching backward. */
int ltu_linear_gelu_fwd(const void* a, int lda, const void* w, const float* bias, void* u, void* h, int M, int N, int K, float p,
                        uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);
/* ---- post-attention half of a transformer layer as ONE launch (model/trans_block.py:203-211), bf16 storage, d = 128 | 256 ----
 *   z1 = x + drop(a Wo^T + bo); t1 = LN1(z1); u = t1 W1^T + b1; h = drop(gelu(u)); z2 = t1 + drop(h W2^T + b2); y = LN2(z2)
 * a workgroup carries 32 token rows through the whole chain in LDS (the five separate launches - projection, LayerNorm,
 * projection + GELU, projection, LayerNorm - re-read every intermediate and are latency-bound on the small token levels).
 * wo / w1 / w2: bf16 weights in MFMA fragment order (ltu_weight_prep kind 8 of the [out][in] fp32 masters).  All intermediate
 * tensors the backward pass needs are written (z1, t1, u, h, z2: bf16; stat1 / stat2 [M][2] = mean, rstd).  Rounding points and
 * dropout masks are those of the op-by-op path (ltu_linear_fwd, ltu_layernorm_fwd, ltu_linear_gelu_fwd).
 * u_mode 0: `u` receives the FFN pre-activation (what ltu_gelu_dropout_bwd expects); u_mode 1: it receives
 * dropout_mask * gelu'(u) instead, the factor ltu_layer_tail_bwd (same u_mode) multiplies dh by - the forward pass has the
 * Gaussian terms at hand, and the backward chain then needs no exp / rcp / mask hash for this stage.
 * qkv != NULL fuses phase B of the linear attention in front of the chain (trans_block.py:41-67 after the context has been
 * formed): the block's q rows are read from qkv [M][3d], `ctx` [B*H][32][32] is the merged context of ltu_linattn_ctx,
 * ntok = tokens per sample (a multiple of 32); `a` is then an OUTPUT ([M][d], the attention output the out-projection weight
 * gradient needs) and qstat [M][H][2] receives the row statistics ltu_linattn_bwd expects.  qkv == NULL: `a` is the input.
 * With qkv_next != NULL the q | k | v projection of the NEXT layer (model/trans_block.py:156-158, which follows :210 of this layer
 * with nothing in between) is formed from the block's y rows before they leave LDS: qkv_next [M][3d] = y cat(Wq, Wk, Wv)^T + cat(b);
 * wq_next = the three [d][d] weights of that layer in fragment order, back to back (ltu_weight_prep kind 8 each), bq0..2 their biases. */
int ltu_layer_tail_fwd(const void* a, const void* x, const void* wo, const void* w1, const void* w2, const float* bo,
                       const float* b1, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                       void* z1, void* t1, void* u, void* h, void* z2, void* y, float* stat1, float* stat2, long long M, int d,
                       float eps, float p, uint64_t seed1, uint64_t seedg, uint64_t seed2, const uint64_t* step, int u_mode,
                       const void* qkv, const float* ctx, float* qstat, int ntok, const void* wq_next, const float* bq0,
                       const float* bq1, const float* bq2, void* qkv_next, int dtype, ltu_stream_t s);

/* The backward of the same chain as ONE launch: LayerNorm 2 backward, data gradients through linear2 / GELU + dropout / linear1,
 * LayerNorm 1 backward (on dt1 + dz2), data gradient through the out projection.  dy2 (nullable): second gradient of y, summed on
 * load.  w2t / w1t / wot: fragment-ordered TRANSPOSED weights (ltu_weight_prep kind 9 of the fp32 masters).  Outputs: da, dz1
 * (gradient of the residual input x) and dr2 / du / dr1 = the G operands of the three weight gradients (ltu_linear_wgrad_group
 * with X = h / t1 / a).  `u` / u_mode: as written by ltu_layer_tail_fwd with the same u_mode.  lnws2 / lnws1: ltu_layer_tail_blocks(M) x 2d floats each = per-workgroup (gamma, beta) column sums,
 * interleaved, folded by ltu_reduce_batch (mode 1). */
long long ltu_layer_tail_blocks(long long M);
int ltu_layer_tail_bwd(const void* dy, const void* dy2, const void* z2, const void* z1, const void* u, const float* stat2,
                       const float* stat1, const float* g2, const float* g1, const void* w2t, const void* w1t, const void* wot,
                       void* dr2, void* du, void* dr1, void* dz1, void* da, float* lnws2, float* lnws1, long long lnws_floats /* each */,
                       long long M, int d, float p,
                       uint64_t seed1, uint64_t seedg, uint64_t seed2, const uint64_t* step, int u_mode, int dtype, ltu_stream_t s);

/* ---- deferred second stage of the two-stage reductions ------------------------------------------
 * ltu_linear_wgrad / ltu_layernorm_bwd can leave the folding of their per-split partial sums to the caller: pass a job
 * record, collect a few, and fold them with ONE launch (ltu_reduce_batch) before the gradients are read.  A record whose
 * `part` comes back NULL needs nothing (the call reduced in place).  The workspace handed to the producing call must stay
 * untouched until the batch has run. */
typedef struct ltu_reduce_job {
  const float* part;   /* mode 0: [nsplit][n][k] tiles followed by [nsplit][n] bias partials; mode 1: [nsplit][n] */
  int nsplit, n, k, nseg;
  float* out[3];       /* mode 0: weight-gradient blocks [n/nseg][k] (+=);  mode 1: out[0][i/2] (i even), out[1][i/2] (i odd) */
  float* outb[3];      /* mode 0: bias-gradient blocks (nullable) */
  int mode;
} ltu_reduce_job;
int ltu_reduce_batch(const ltu_reduce_job* jobs, int njobs, ltu_stream_t s);   /* jobs: host array */

/* dw_i[N/nw,K] += g[:, block i]^T . a[M,K];  db_i += column sums of g (fp32 gradients, accumulated; db may be NULL).
 * ws: optional workspace of ltu_wgrad_ws_floats(M,N,K) floats - with it (bf16) the row-split partial tiles are stored and
 * summed by a second kernel (no atomics, one launch for all nw blocks); without it fp32 atomics are used. */
long long ltu_wgrad_ws_floats(long long M, int N, int K);
int ltu_linear_wgrad(const void* g, int ldg, const void* a, int lda, float* const* dw, float* const* db, int nw, int M, int N,
                     int K, float* ws, long long ws_floats, ltu_reduce_job* defer, int dtype, ltu_stream_t s);
/* Several of the above in ONE launch + ONE fold: the weight / bias gradients of the four projections of a transformer layer
 * (model/trans_block.py:144,156,166,187,189: q,k,v as one job with nw = 3, out, linear1, linear2).  Together they offer 8-32
 * output tiles, so a few row splits per tile fill the chip and the fp32 partial tiles shrink 4x against four separate calls.
 * The host side may also hand in the jobs of SEVERAL layers of one transformer at once (small levels, where a layer's group is
 * launch-latency-bound): all jobs of a group share one split count, so they should have the same M.
 * jobs: host array (<= LTU_WGRAD_GROUP_MAX); blocks: the workgroup budget of the launch (<= 0: the library default, 256 = one per
 * CU; train.GraphedStep passes 128 for launches that run on its side stream beside the main chain).  The geometry (tile types,
 * per-job split counts, workspace layout) is a function of the jobs' shapes and `blocks` only; the size query and the launch take
 * the same `blocks`, and the launch is told the capacity of ws (ws_floats) and returns LTU_E_ARG without launching when its
 * geometry needs more.  ltu_linear_wgrad_group_ws_floats() == 0: this group is not handled - use ltu_linear_wgrad per job (handled:
 * bf16 storage, N and K multiples of 128, M a multiple of 32 and >= 1024). */
#define LTU_WGRAD_GROUP_MAX 32
typedef struct ltu_wgrad_job {
  const void* grad;    /* g [M][ldg] */
  const void* a;       /* a [M][lda] */
  float* dw[3];        /* nw gradient blocks [N/nw][K] (+=) */
  float* db[3];        /* nw bias-gradient blocks (nullable) */
  int ldg, lda, nw, M, N, K;
} ltu_wgrad_job;
long long ltu_linear_wgrad_group_ws_floats(const ltu_wgrad_job* jobs, int njobs, int blocks);
int ltu_linear_wgrad_group(const ltu_wgrad_job* jobs, int njobs, int blocks, float* ws, long long ws_floats, int dtype, ltu_stream_t s);

/* Workspace (floats) that ltu_upconv_wgrad needs for M = B*H*W*D coarse voxels (bf16 path; sub-pixel un-embedding of
 * model/Unet_3Dblock.py:419-432) at a workgroup budget of `blocks` (<= 0: the library default; the launch takes the same value). */
long long ltu_upconv_wgrad_ws_floats(long long M, int Co, int Ci, int blocks);

/* ---- 3x3x3 convolution, padding 1: model/Unet_3Dblock.py:310,314,375,421,523,528,588,1328,1353 --
 * x0 [B,Hi,Wi,Di,C0] (+ optional x1 [..,C1]: the channel concat of Unet_3Dblock.py:553 without
 * materialising it), wf [Co][27][C0+C1], stride (sh,sw,sd) in {1,2}; ups != 0: the conv reads the
 * nearest-neighbour x2 upsampling of x0 (nn.Upsample of Unet_3Dblock.py:421), (Hi,Wi,Di) are then
 * the physical dims.  y [B,Ho,Wo,Do,Co]. */
int ltu_conv3d_fwd(const void* x0, const void* x1, const void* wf, const float* bias, void* y, int B, int Hi, int Wi,
                   int Di, int C0, int C1, int Co, int sh, int sw, int sd, int ups, float* ws, long long ws_floats, int dtype,
                   ltu_stream_t s);
/* ws of ltu_conv3d_fwd / ltu_conv3d_dgrad (optional, bf16 stride-1 convs only): floats of workspace that let a conv over a
 * small grid (the deep U-Net levels) split its input channels over several workgroups per tile; 0 when the shape does not
 * split.  (B,H,W,D) = the conv's output grid, C = input channels of the call (Co for the data gradient), Co = its outputs. */
long long ltu_conv3d_ws_floats(int B, int H, int W, int D, int C, int Co);
/* the same for the gather implicit GEMMs (strided convs: M output voxels, N = Co, K = 27*C; ltu_upconv_dgrad: M = B*H*W*D,
 * N = Ci, K = 64*Co): floats of workspace that let a small grid split its K loop, 0 when it does not split */
long long ltu_igemm_ws_floats(long long M, int N, int K);
/* Two stride-1 convs over the same input in one pass (a decoder level's conv1 and its mask head read the same upsampled tensor:
 * model/Unet_3Dblock.py:1353 + 1380): wf [N0+N1][27][C], bias [N0+N1]; columns [0,N0) -> y0 [..,N0], the rest -> y1 [..,N1].
 * Data gradient of the pair: g0 [..,N0] and g1 [..,N1] read as one virtual concat against wd [C][27][N0+N1] -> dx [..,C]
 * (no separate add of two input gradients).  ws as for ltu_conv3d_fwd with Co = N0+N1 (C = N0+N1, Co = C for the gradient). */
int ltu_conv3d_pair_fwd(const void* x, const void* wf, const float* bias, void* y0, void* y1, int B, int H, int W, int D, int C,
                        int N0, int N1, float* ws, long long ws_floats, int dtype, ltu_stream_t s);
int ltu_conv3d_pair_dgrad(const void* g0, const void* g1, const void* wd, void* dx, int B, int H, int W, int D, int C, int N0,
                          int N1, float* ws, long long ws_floats, int dtype, ltu_stream_t s);
/* weight gradients of the pair (+=) straight into the two PyTorch-layout gradients dwa [co_a][ci][3][3][3], dwb [co_b][ci][3][3][3]
 * and dba / dbb; ws: ltu_wgrad_ws_floats(B*H*W*D, N0+N1, 27*C) floats (one pass over x for both) or NULL. */
int ltu_conv3d_pair_wgrad(const void* g0, const void* g1, const void* x, float* dwa, float* dba, float* dwb, float* dbb, int B,
                          int H, int W, int D, int C, int N0, int N1, int co_a, int co_b, int ci, float* ws, long long ws_floats,
                          int dtype, ltu_stream_t s);
/* data gradient: g [B,Ho,Wo,Do,Co], wd [C0+C1][27][Co] -> dx0 [B,Hl,Wl,Dl,C0] (+ dx1 [..,C1]); (Hl,Wl,Dl)
 * are the LOGICAL input dims (= 2x physical when the forward used ups: pool with ltu_sumpool2). */
int ltu_conv3d_dgrad(const void* g, const void* wd, void* dx0, void* dx1, int B, int Hl, int Wl, int Dl, int C0,
                     int C1, int Co, int sh, int sw, int sd, float* ws, long long ws_floats, int dtype, ltu_stream_t s);
/* weight gradient (+=, the caller zero-fills): torch_co == 0: into the packed layout dwf [Co][27][C0+C1];
 * torch_co != 0: straight into a PyTorch-layout gradient [torch_co][torch_ci][3][3][3] (padded rows/channels dropped).
 * db[Co] += column sums of g.
 * ws: optional workspace of ltu_wgrad_ws_floats(B*Ho*Wo*Do, Co, 27*(C0+C1)) floats (two-stage reduction, see above). */
int ltu_conv3d_wgrad(const void* g, const void* x0, const void* x1, float* dwf, float* db, int B, int Hi, int Wi,
                     int Di, int C0, int C1, int Co, int sh, int sw, int sd, int ups, int torch_co, int torch_ci, float* ws,
                     long long ws_floats, int dtype, ltu_stream_t s);
/* ---- nearest x2 upsampling + 3x3x3 conv as a sub-pixel conv: model/Unet_3Dblock.py:419-432 (UpEmbedBlock) ------------
 * Same result as ltu_conv3d_* with ups = 1 at 64/216 of the multiply-adds: the 8 output parity classes are 2x2x2-tap
 * convs on the low-res grid with pre-summed weights (ltu_weight_prep kinds 5 / 6).  x [B,H,W,D,Ci] -> y [B,2H,2W,2D,Co]. */
int ltu_upconv_fwd(const void* x, const void* wsub_f, const float* bias, void* y, int B, int H, int W, int D, int Ci, int Co,
                   int dtype, ltu_stream_t s);
int ltu_upconv_dgrad(const void* g, const void* wsub_d, void* dx, int B, int H, int W, int D, int Ci, int Co, float* ws,
                     long long ws_floats, int dtype, ltu_stream_t s);
/* dweff: zero-filled scratch [8][Co][8][Ci] fp32; dw_torch [co_real][ci_real][3][3][3] += and db[Co] += ;
 * ws: optional ltu_upconv_wgrad_ws_floats(B*H*W*D, Co, Ci, blocks) floats (bf16 two-stage reduction); blocks: workgroup budget of the
 * launch (<= 0: the library default), the value the size query was given */
int ltu_upconv_wgrad(const void* g, const void* x, float* dweff, float* db, float* dw_torch, int co_real, int ci_real, float* ws,
                     long long ws_floats, int blocks, int B, int H, int W, int D, int Ci, int Co, int dtype, ltu_stream_t s);
/* y[b,h,w,d,c] = sum of the 2x2x2 children of x [B,2H,2W,2D,C] (adjoint of nearest x2 upsampling) */
int ltu_sumpool2(const void* x, void* y, int B, int H, int W, int D, int C, int dtype, ltu_stream_t s);

/* ---- linear attention core: model/trans_block.py:41-67 -----------------------------------------
 * qkv [B*N][3d] (q | k | v; head h = columns h*32..h*32+31 of each third) -> out [B*N][d].
 * Saved for backward: ctx [B*H][32][32], colstats [B*H][64] (column max | column sum of exp),
 * qstat [B*N][H][2] (row max, 1/(rowsum*sqrt(32))).  part_ws: ltu_linattn_ws_floats(B, N, d) floats (= B * (ns + ns/16 + 2) * H * 1088
 * for the split count ns the launches pick; the backward needs B * ns * H * 1024 of them); ltu_linattn_splits(B, N) is an upper
 * bound of ns over d. */
int ltu_linattn_splits(int B, int N);
long long ltu_linattn_ws_floats(int B, int N, int d);
int ltu_linattn_fwd(const void* qkv, void* out, float* ctx, float* colstats, float* qstat, float* part_ws, long long ws_floats, int B,
                    int N, int d, int dtype, ltu_stream_t s);
/* phase A of ltu_linattn_fwd alone: ctx [B*H][32][32] and colstats [B*H][64] (same workspace); phase B then runs inside
 * ltu_layer_tail_fwd (its qkv / ctx / qstat arguments) */
int ltu_linattn_ctx(const void* qkv, float* ctx, float* colstats, float* part_ws, long long ws_floats, int B, int N, int d, int dtype,
                    ltu_stream_t s);
/* dqkv [B*N][3d] from dout [B*N][d]; dctx [B*H][32][32] is a scratch output; tvec [B*H][32] is reserved (may be NULL: the term it
 * held is formed inside the per-token kernel since round 2) */
int ltu_linattn_bwd(const void* qkv, const void* dout, const float* ctx, const float* colstats, const float* qstat,
                    void* dqkv, float* dctx, float* tvec, float* part_ws, long long ws_floats, int B, int N, int d, int dtype,
                    ltu_stream_t s);

/* ---- InstanceNorm3d (+LeakyReLU, residual, dropout): model/Unet_3Dblock.py:312-339,526-556,593 ----
 * x [B][S][C].  sums [B][C][3] = {shift, sum(x-shift), sum((x-shift)^2)} (zero-filled by the caller).
 * apply: y = dropout(act((x-mean)*rstd)) + res (res may be NULL). */
/* `ws` (nullable) is a scratch buffer of at least ltu_norm_ws_floats() floats: with it the per-block partial sums are folded by a
 * second small kernel instead of fp32 atomics (same results up to summation order).  One buffer can serve every call on a stream. */
long long ltu_norm_ws_floats(void);
int ltu_instnorm_stats(const void* x, float* sums, float* ws, long long ws_floats, int B, long long S, int C, int dtype, ltu_stream_t s);
int ltu_instnorm_apply(const void* x, const float* sums, const void* res, void* y, int B, long long S, int C, int act,
                       float slope, float p, uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);
/* stats + apply in ONE call (what the model's forward uses): when the shape qualifies (bf16 or fp32, C a power of two, a few KB
 * of partial sums per sample) the statistics kernel leaves its per-chunk partials in `ws` and every workgroup of the apply kernel
 * folds them itself - no fold launch in between; workgroup 0 of each sample publishes sums[b][c][1..2] for the backward pass.
 * Otherwise exactly ltu_instnorm_stats followed by ltu_instnorm_apply. */
int ltu_instnorm_fwd(const void* x, float* sums, float* ws, long long ws_floats, const void* res, void* y, int B, long long S, int C, int act,
                     float slope, float p, uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);
/* dx from dy (+ dy2 + dy3, nullable: the gradients of further consumers of y, summed on load instead of by a stand-alone add pass:
 * the skip tensors of the U-Net and the transformer inputs have two or three consumers); bsums [B][C][2] zero-filled scratch */
int ltu_instnorm_bwd(const void* dy, const void* dy2, const void* dy3, const void* x, const float* sums, float* bsums, float* ws,
                     long long ws_floats, void* dx, int B, long long S, int C, int act, float slope, float p, uint64_t seed, const uint64_t* step,
                     int dtype, ltu_stream_t s);

/* ---- residual LayerNorm: model/trans_block.py:205-206,209-210 -----------------------------------
 * y = LN(x + dropout(r)) * gamma + beta over rows of d in {32,64,128,256}; r is OVERWRITTEN with the
 * pre-norm sum z; stat [M][2] = {mean, rstd}. */
int ltu_layernorm_fwd(const void* x, void* r, const float* gamma, const float* beta, void* y, float* stat, long long M,
                      int d, float eps, float p, uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);
/* dz (gradient of x) and dr = dz*dropmask (dr may alias dz when p = 0); dgamma/dbeta += (zero-filled) */
/* dy2 (nullable): a second upstream gradient, summed with dy on load (the layer output feeds both the next projection and the next
 * residual; folding the sum here saves autograd's separate add pass);
 * ws (nullable: atomics): at least 2 * d * ceil(M / rows) floats of partial (gamma, beta) rows with rows >= ceil(M / 1024), i.e. 2048 * d
 * floats always suffice (ltu_norm_ws_floats() too) */
int ltu_layernorm_bwd(const void* dy, const void* dy2, const void* z, const float* stat, const float* gamma, void* dz, void* dr,
                      float* dgamma, float* dbeta, float* ws, long long ws_floats, ltu_reduce_job* defer, long long M, int d, float p, uint64_t seed,
                      const uint64_t* step, int dtype, ltu_stream_t s);

/* ---- GELU(erf) + dropout: model/trans_block.py:208 ---------------------------------------------- */
int ltu_gelu_dropout_fwd(const void* u, void* h, long long n, float p, uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);
int ltu_gelu_dropout_bwd(const void* dh, const void* u, void* du, long long n, float p, uint64_t seed, const uint64_t* step, int dtype,
                         ltu_stream_t s);

/* ---- class-probability heads ---------------------------------------------------------------------
 * mask head softmax (model/Unet_3Dblock.py:1380-1381): logits T [M][CP] (first C valid) -> p f32 [M][C]; 1 <= C <= 8 in both heads
 * (else LTU_E_SHAPE); the backward writes the padding columns C .. CP-1 of dz as zero */
int ltu_head_softmax_fwd(const void* z, float* p, long long M, int C, int CP, int dtype, ltu_stream_t s);
int ltu_head_softmax_bwd(const float* dp, const float* p, void* dz, long long M, int C, int CP, int dtype, ltu_stream_t s);
/* final head (model/Unet_3Dblock.py:1392-1394): z [B,h,w,D,4C] -> window un-embedding + softmax -> p f32 [B,2h,2w,D,C] */
int ltu_final_softmax_fwd(const void* z, float* p, int B, int h, int w, int D, int C, int CP, int dtype, ltu_stream_t s);   /* z rows of CP >= 4C channels (padded conv output) */
int ltu_final_softmax_bwd(const float* dp, const float* p, void* dz, int B, int h, int w, int D, int C, int CP, int dtype,
                          ltu_stream_t s);
/* The heads of a region model (csrc/region.hip): channel r is the sigmoid of logit r, p = 1 / (1 + exp(-z)), finite and in [0, 1] for
 * every finite logit; arguments, padded columns (CP), dtypes and window un-embedding of the softmax heads above, 1 <= R <= 8.  The
 * backward forms dz = (dp p) (1 - p) from the saved p and writes the padding columns as zero; every launch form of a row (one
 * 16-byte store per 8 bf16 columns, vector or scalar accesses) gives the same bits. */
int ltu_head_sigmoid_fwd(const void* z, float* p, long long M, int R, int CP, int dtype, ltu_stream_t s);
int ltu_head_sigmoid_bwd(const float* dp, const float* p, void* dz, long long M, int R, int CP, int dtype, ltu_stream_t s);
int ltu_final_sigmoid_fwd(const void* z, float* p, int B, int h, int w, int D, int R, int CP, int dtype, ltu_stream_t s);
int ltu_final_sigmoid_bwd(const float* dp, const float* p, void* dz, int B, int h, int w, int D, int R, int CP, int dtype,
                          ltu_stream_t s);
/* eval branch of a region model: o[i] = p[i] > thr ? 1 : 0, f32, i < n */
int ltu_prob_indicator(const float* p, float* o, long long n, float thr, ltu_stream_t s);
/* eval branch (model/trans_3DUnet.py:199-202): one-hot of the arg-max class, p/o f32 [M][C] */
int ltu_onehot_argmax(const float* p, float* o, long long M, int C, ltu_stream_t s);

/* ---- attention gate: model/Unet_3Dblock.py:217-221 + 1385 ---------------------------------------
 * u1 = Wx.skip, u2 = Wg.up ([B][S][C], from ltu_linear_fwd), sums1/sums2 their InstanceNorm sums.
 * a = sigmoid(psi . relu(IN(u1)+IN(u2)) + b) -> a_out f32 [B*S]; out = skip * a. */
int ltu_gate_fwd(const void* u1, const void* u2, const float* sums1, const float* sums2, const float* psi_w,
                 const float* psi_b, const void* skip, float* a_out, void* out, int B, long long S, int C, int dtype,
                 ltu_stream_t s);
/* -> dskip (direct path), du1, du2, dpsi_w[C] +=, dpsi_b[1] +=; ds_ws f32 [B*S], bs1/bs2 [B][C][2] zero-filled scratch */
int ltu_gate_bwd(const void* dout, const void* u1, const void* u2, const float* sums1, const float* sums2,
                 const float* psi_w, const void* skip, const float* a_in, void* dskip, float* ds_ws, float* dpsi_w,
                 float* dpsi_b, float* bs1, float* bs2, float* ws, long long ws_floats, void* du1, void* du2, int B, long long S, int C,
                 int dtype, ltu_stream_t s);   /* ws: ltu_norm_ws_floats() floats (two-stage reduction) or NULL (atomics) */

/* ---- positional depthwise conv: model/trans_block.py:86-96 on the grid of Unet_3Dblock.py:267-270 ----
 * y = chan_dropout(x + dwconv3x3x3(x) + bias), x [B,H,W,D,C]; w [C,1,3,3,3] with the reference's kernel
 * axes (D,H,W); nn.Dropout3d draws one keep/drop per (sample, channel). */
int ltu_dwconv_fwd(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int D, int C, float p,
                   uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);
/* dx, and dw [C][27] +=, db [C] += (zero-filled by the caller); dy2 (nullable): gradient of a second consumer, summed on load.
 * ws: ltu_dwconv_bwd_ws_floats(...) floats for the per-workgroup partial sums of dw / db, folded in a fixed order; NULL falls
 * back to float atomics (the two gradients then differ in the last bits from run to run).  dx NULL: only dw / db are computed;
 * dw NULL: only dx (the two halves are independent launches: the weight gradient can be issued later, off the data-gradient chain). */
long long ltu_dwconv_bwd_ws_floats(int B, int H, int W, int D, int C, int dtype);
int ltu_dwconv_bwd(const void* dy, const void* dy2, const void* x, const float* w, void* dx, float* dw, float* db, float* ws,
                   long long ws_floats, int B, int H, int W, int D, int C, float p, uint64_t seed, const uint64_t* step, int dtype, ltu_stream_t s);

/* ---- dynamic ROI: model/Unet_3Dblock.py:821-873, 37-49 (box), 51-82 (index maps), 985-1117 (warps) ----
 * prob f32 [B,H,W,D,C]: foreground = (1 - prob[...,0]) >= thr.  Writes box [B][6] = (x0,y0,0,x1,y1,D-1)
 * and the sampling plans (sizes from ltu_roi_plan_size) used by ltu_roi_resample.  hist: n_hist ints of zero-filled scratch
 * (foreground histograms; the library issues no memsets of its own, see csrc/roi.hip). */
int ltu_roi_plan_size(int B, int H, int W, int roi_size, long long* n_int, long long* n_float, long long* n_hist);
int ltu_roi_plan(const float* prob, int B, int H, int W, int D, int C, int roi_size, float thr, float* box, int* plan_i,
                 float* plan_f, int* hist, ltu_stream_t s);
/* the plan of a region model (csrc/region.hip): foreground = (max_r prob[...,r]) >= thr over the C <= 8 region channels; the
 * comparison, the plan kernel, the buffers and ltu_roi_plan_size are those of ltu_roi_plan */
int ltu_roi_plan_union(const float* prob, int B, int H, int W, int D, int C, int roi_size, float thr, float* box, int* plan_i,
                       float* plan_f, int* hist, ltu_stream_t s);
/* which = 0: image [B,H,W,D,C] -> ROI grid [B,eh,ew,D,C] (roi_alignment2); which = 1: ROI grid -> image
 * (post_processing2).  adjoint != 0 applies the transposed operator to a gradient (in has the shape of the
 * forward output, out the shape of the forward input). */
int ltu_roi_resample(const void* in, void* out, int* plan_i, float* plan_f, int which, int adjoint, int B, int H, int W,
                     int D, int C, int roi_size, int dtype, ltu_stream_t s);

/* ---- trilinear x(2,2,sd) upsampling, align_corners=True: model/Unet_3Dblock.py:1341-1345,1375-1378 ----
 * forward: in [B,H,W,D,C] -> out [B,2H,2W,sd*D,C]; adjoint != 0: in = gradient of the output, in2 (nullable, adjoint only) =
 * gradient of a second consumer of the output, summed on load. */
int ltu_trilinear_up(const void* in, const void* in2, void* out, int adjoint, int B, int H, int W, int D, int C, int sd, int dtype,
                     ltu_stream_t s);
/* The adjoint in separable form (one 1-D transposed interpolation per upsampled axis: at most 5 candidates per output instead of
 * ~64 gathers).  ws: ltu_trilinear_adjoint_ws_elems(...) elements of the storage type; intermediates are rounded to it. */
long long ltu_trilinear_adjoint_ws_elems(int B, int H, int W, int D, int C, int sd);
int ltu_trilinear_adjoint(const void* dy, const void* dy2, void* dx, void* ws, long long ws_elems, int B, int H, int W, int D, int C, int sd,
                          int dtype, ltu_stream_t s);

/* ---- deep-supervision losses of one level: loss/criterions.py:35-70,416-442,696-735;
 *      loss/multi_criterions.py:58-110,594-615 ------------------------------------------------------
 * p f32 [B][S][C] probabilities, label u8 [B][S].  total = w_ce*CE + w_bal*BalancedDice + sum_c w_dice[c]*Dice_c
 * + w_dice[4]*Dice of the foreground union (1 - p_0 vs label != 0: multi_criterions.py:30-56, DiceClassLoss0); w_dice: 5 host floats.
 * values (9 floats): [0] = total, [1] = CE, [2] = balanced Dice, [3+c] = Dice_c, [7] = union Dice, [8] = total again;
 * sums: scratch of ltu_loss_ws_floats(B, S, C) floats (no initialisation needed: per-block partial sums behind the final
 * [B][C][4] sums, folded in a fixed order - no floating-point atomics, the loss and its gradient are reproducible bit for bit);
 * coef [B][C][3] feeds ltu_loss_bwd: dp = gscale[0] * dTotal/dp.  scale_dev (nullable): device-resident factor on all three
 * weights, read at run time (the per-epoch level weight of train3D.py:122-137 divided by the accumulation count of
 * utils/utils_3D_embed_full.py:85, so a captured graph follows both without re-capture). */
long long ltu_loss_ws_floats(int B, long long S, int C);
int ltu_loss_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B, long long S, int C,
                 float w_ce, float w_bal, const float* w_dice, const float* scale_dev, ltu_stream_t s);
int ltu_loss_bwd(const float* p, const uint8_t* label, const float* coef, const float* gscale, float* dp, int B,
                 long long S, int C, ltu_stream_t s);
/* ---- the same losses for 2 <= C <= 8 classes (csrc/loss.hip; loss/multi_criterions.py:58-83, DiceClassLoss(class_index)) ----
 * The kernels of ltu_loss_fwd with room for 8 classes.  w_dice: C + 1 host floats, the Dice weight of every class, then that
 * of the foreground union.  values (C + 5 floats): [0] = total, [1] = CE, [2] = balanced Dice, [3 + c] = Dice_c, [3 + C] = union
 * Dice, [4 + C] = total again.  sums: scratch of ltu_loss_wide_ws_floats(B, S, C) floats, no initialisation, folded in a fixed
 * order (no floating-point atomics: two calls agree bit for bit).  coef [B][C][3] feeds ltu_loss_wide_bwd (ltu_loss_bwd hands C > 4
 * over to it).  LTU_E_SHAPE: C outside 2 .. 8 or B C 4 > 256 (the finalize's row limit; the size query then returns 0); LTU_E_ARG:
 * a NULL pointer or sums shorter than the geometry needs; both before anything is launched. */
long long ltu_loss_wide_ws_floats(int B, long long S, int C);
int ltu_loss_wide_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B, long long S,
                      int C, float w_ce, float w_bal, const float* w_dice, const float* scale_dev, ltu_stream_t s);
int ltu_loss_wide_bwd(const float* p, const uint8_t* label, const float* coef, const float* gscale, float* dp, int B, long long S, int C,
                      ltu_stream_t s);
/* ---- the wider loss family of one level: loss/criterions.py:8-32,466-530,563-615,618-644,738-751;
 *      loss/multi_criterions.py:517-541,617-663, and the five terms of ltu_loss_fwd ---------------------------------------
 * p f32 [B][S][C] probabilities, label u8 [B][S], 2 <= C <= 4 and B (7 C + 3) <= 256 (else LTU_E_SHAPE).  cfg: LTU_LOSS_EXT_NCFG
 * host floats, the weight of every term (index LTU_LOSS_EXT_CE .. LTU_LOSS_EXT_CLASSIFY; DICE0 + c = DiceClassLoss of class c)
 * followed by gamma (FocalLoss), sigma (SSLoss), alpha (ContainLoss), alpha2 (ContainLoss2) and eps (the new terms' epsilon);
 * a non-finite entry, or a Dice weight of a class c >= C, is LTU_E_ARG.  total = sum_k cfg[k] * term_k over the terms with
 * cfg[k] != 0 (a term switched off adds nothing to total or gradient, even where its value is inf / NaN on the data; its value
 * is still reported), every weight times scale_dev[0] when scale_dev is given
 * (device-resident, read at run time, as in ltu_loss_fwd).  values (LTU_LOSS_EXT_NTERM + 2 floats): [0] = total, [1 + k] = term
 * k, [1 + NTERM] = total again.  sums: scratch of ltu_loss_ext_ws_floats(B, S, C) floats, no initialisation, folded in a fixed
 * order (bit-reproducible); shorter is LTU_E_ARG.  coef [B][C][8] feeds ltu_loss_ext_bwd (same cfg): dp = gscale[0] * dTotal/dp.
 * Argument errors return before anything is launched.  Terms switched off by a zero weight cost nothing in the streaming passes. */
enum { LTU_LOSS_EXT_CE = 0, LTU_LOSS_EXT_BAL = 1, LTU_LOSS_EXT_DICE0 = 2 /* .. 5 */, LTU_LOSS_EXT_FG = 6, LTU_LOSS_EXT_DICE = 7,
       LTU_LOSS_EXT_IOU = 8, LTU_LOSS_EXT_SS = 9, LTU_LOSS_EXT_FOCAL = 10, LTU_LOSS_EXT_MSE = 11, LTU_LOSS_EXT_CONTAIN = 12,
       LTU_LOSS_EXT_CONTAIN2 = 13, LTU_LOSS_EXT_BAL2 = 14, LTU_LOSS_EXT_CE0 = 15, LTU_LOSS_EXT_CLASSIFY = 16,
       LTU_LOSS_EXT_NTERM = 17,
       LTU_LOSS_EXT_GAMMA = 17, LTU_LOSS_EXT_SIGMA = 18, LTU_LOSS_EXT_ALPHA = 19, LTU_LOSS_EXT_ALPHA2 = 20, LTU_LOSS_EXT_EPS = 21,
       LTU_LOSS_EXT_NCFG = 22 };
long long ltu_loss_ext_ws_floats(int B, long long S, int C);
int ltu_loss_ext_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values, float* coef, int B, long long S,
                     int C, const float* cfg, const float* scale_dev, ltu_stream_t s);
int ltu_loss_ext_bwd(const float* p, const uint8_t* label, const float* coef, const float* cfg, const float* gscale, float* dp, int B,
                     long long S, int C, ltu_stream_t s);
/* ---- boundary loss of one level (Kervadec et al., "Boundary loss for highly unbalanced segmentation"; no reference counterpart;
 *      csrc/distmap.hip, csrc/loss_boundary.hip) ---------------------------------------------------------------------------
 * distmap_signed: label u8 [B][H][W][D], classes a HOST array of K distinct ids in 0 .. 255 (1 <= K <= 8; a repeated id is
 * LTU_E_ARG) -> phi f32 [B][K][H][W][D], the signed Euclidean distance map of G = {label == classes[k]} inside the patch with
 * spacing (sh, sw, sd) > 0: phi(x) = dist(x, G) outside G, -(dist(x, not G) - 1) inside G (the 1 is not scaled by the spacing:
 * Kervadec's one_hot2dist), and phi = 0 everywhere when G is empty or fills the patch, decided on the device.  Squared distances
 * are formed in double and kept as fp32 between the three line passes (exact integers with unit spacing); the passes keep their
 * envelopes in LDS.  scratch: ltu_distmap_scratch_elems(B, K, H, W, D) 4-byte elements, no initialisation.  One call serves all
 * B K volumes and both polarities on stream s (capturable), no atomics, no host read: two calls agree bit for bit.
 * LTU_E_SHAPE: an axis outside 1 .. 512, K outside 1 .. 8, B K > 65535; LTU_E_ARG: a bad class id, a non-finite or non-positive
 * spacing, a NULL pointer, short scratch; all before anything is launched.
 * loss_boundary: p f32 [B][S][C] probabilities (2 <= C <= 8), phi f32 [B][K][S], classes / w HOST arrays of the K terms (a class
 * >= C or a non-finite weight is LTU_E_ARG).  values (1 + K floats): [1 + k] = value_k = (1 / (B S)) sum_b sum_s p[b][s][c_k]
 * phi[b][k][s] (unweighted), [0] = (base_total ? base_total[0] : 0) + scale sum_k w_k value_k with scale = scale_dev[0] *
 * term_scale_dev[0] (each NULL = 1; device-resident, read at run time, as in ltu_loss_fwd).  sums: scratch of
 * ltu_loss_boundary_sums_floats(B, S, K) floats on an 8-byte boundary, no initialisation, folded in a fixed order (no atomics:
 * bit-reproducible); shorter is LTU_E_ARG.  bwd: dp [B][S][C] gets gscale[0] scale w_k phi[b][k][s] / (B S) in channel c_k:
 * added to what ltu_loss_bwd / ltu_loss_wide_bwd / ltu_loss_ext_bwd has just written there when accumulate != 0, else written
 * with zeros in every other channel.  Argument errors return before anything is launched. */
long long ltu_distmap_scratch_elems(int B, int K, int H, int W, int D);
int ltu_distmap_signed(const uint8_t* label, const int* classes, int K, float* phi, void* scratch, long long scratch_elems, int B, int H,
                       int W, int D, float sh, float sw, float sd, ltu_stream_t s);
long long ltu_loss_boundary_sums_floats(int B, long long S, int K);
int ltu_loss_boundary_fwd(const float* p, const float* phi, const int* classes, const float* w, int K, float* sums, long long sums_floats,
                          float* values, const float* base_total, const float* scale_dev, const float* term_scale_dev, int B,
                          long long S, int C, ltu_stream_t s);
int ltu_loss_boundary_bwd(const float* phi, const int* classes, const float* w, int K, const float* scale_dev,
                          const float* term_scale_dev, const float* gscale, float* dp, int accumulate, int B, long long S, int C,
                          ltu_stream_t s);
/* ---- top-k cross-entropy of one level (nnU-Net's TopKLoss; no reference counterpart; csrc/loss_topk.hip) -------------------------
 * p f32 [B][S][C] probabilities (2 <= C <= 8), label u8 [B][S], N = B S.  Per voxel l = -log(max(p[label], 1e-6)) in fp32 (0 and
 * no gradient where label >= C; such voxels still count in N).  k = min(max(floor((double)frac N), 1), N) with frac the host
 * argument or, when frac_dev != NULL, frac_dev[0] read on the device at run time (out of range: clamped to k = 1 / k = N;
 * non-finite: k = N).  tau = the k-th largest l over the whole batch, n_gt = #{l > tau}, n_eq = #{l == tau}:
 *   value = (sum_{l > tau} l + (k - n_gt) tau) / k          (k = N: the plain mean)
 *   values[0] = (base_total ? base_total[0] : 0) + scale_dev[0] w value (scale_dev NULL = 1), values[1] = value, values[2] = tau.
 * bwd: dp[b][s][label] gets gscale[0] scale_dev[0] w weight (-1 / p) where p >= 1e-6, with weight = 1 / k where l > tau, 0 where
 * l < tau and (k - n_gt) / (n_eq k) where l == tau (tied voxels share what is left of the k: the symmetric subgradient, which
 * makes the result a function of the input where torch.topk picks arbitrarily); added to what a level's base backward has just
 * written when accumulate != 0, else written with zeros in every other channel.
 * tau is found by an exact radix select on the bits of l with integer histograms (integer LDS / global atomics only, no
 * floating-point atomics; partial sums folded in a fixed order): two calls agree bit for bit; no host read, capturable.
 * scratch: ltu_loss_topk_scratch_elems(B, S) 4-byte elements on a 16-byte boundary (else LTU_E_ALIGN), no initialisation; it
 * keeps l and the selection record, and the backward reads the scratch its forward wrote.
 * LTU_E_SHAPE: C outside 2 .. 8, B S outside 1 .. 2^31 - 1; LTU_E_ARG: a NULL pointer, short scratch, non-finite w, host frac
 * outside (0, 1] when frac_dev is NULL; all before anything is launched. */
long long ltu_loss_topk_scratch_elems(int B, long long S);
int ltu_loss_topk_fwd(const float* p, const uint8_t* label, void* scratch, long long scratch_elems, float* values /* 3 */,
                      const float* base_total, float w, float frac, const float* frac_dev, const float* scale_dev, int B,
                      long long S, int C, ltu_stream_t s);
int ltu_loss_topk_bwd(const float* p, const uint8_t* label, const void* scratch, long long scratch_elems, float w,
                      const float* scale_dev, const float* gscale, float* dp, int accumulate, int B, long long S, int C,
                      ltu_stream_t s);
/* ---- losses for class-imbalanced tasks: Tversky, focal Tversky, focal cross-entropy (csrc/loss_imbalance.hip) -------------------
 * The fourth stage of a level's loss chain.  p f32 [B][S][C] probabilities (2 <= C <= 8), label u8 [B][S].  With t_c = [label == c]
 * (t = 0 in every class where label >= C, as in the base losses) the sums pass accumulates per (b, c), each sum directly and none
 * as a difference of two others (no cancellation when p[label] == 1.0 on most voxels; all four are >= 0):
 *     I = sum p t    FP = sum p (1 - t)    FN = sum t (1 - p)    F = sum t (1 - p)^gf (-log max(p, 1e-6))
 * Tversky term k (K <= 8 terms, class classes[k], weight w[k]; Salehi et al., focal form of Abraham & Khan) with the shared
 * params = {alpha, beta, gamma, eps, batch}, alpha, beta >= 0, alpha + beta > 0, 1 <= gamma <= 3 (1: plain Tversky), eps > 0, batch 0 / 1:
 *     1 - TI = (alpha FP + beta FN) / (I + alpha FP + beta FN + eps)          (TI = (I + eps) / (the same denominator))
 *     batch == 0:  value_k = (1 / B) sum_b (1 - TI[b, c])^(1 / gamma)
 *     batch == 1:  I, FP, FN summed over b first (in the order of b), value_k = (1 - TI[c])^(1 / gamma)       (nnU-Net's batch_dice;
 *                  alpha = beta = 0.5, eps = 0.5e-5 is its soft Dice (2 I + 1e-5) / (P + T + 1e-5); the batch is this call's)
 *   Where 1 - TI is exactly 0 and gamma > 1 the power's derivative is infinite: the gradient of that term is 0 there (the chosen
 *   subgradient).
 * Focal cross-entropy (weight w_focal; gf = focal_gamma is 0 or in [1, 5] - in (0, 1) the derivative at p = 1 is unbounded;
 * focal_alpha: C class weights a_c, finite and >= 0, NULL = all 1):
 *     value = (1 / (B S)) sum_{b, c} a_c F[b, c]          (gf = 0, a = 1: the plain mean of -log max(p[label], 1e-6))
 *   With w_focal == 0 the term is not evaluated (no log per voxel) and its value reads 0.
 *   Voxels with label >= C add 0 and count in B S.  The gradient is that of the clamped expression: below p = 1e-6 the
 *   -(1 - p)^gf / p part is absent.
 * values [K + 3] = {total, value_0 .. value_{K-1}, focal value, total again}, total = (base_total ? base_total[0] : 0) + scale
 * (sum_k w[k] value_k + w_focal value), scale = scale_dev ? scale_dev[0] : 1 read on the device.  coef [B][C][3], already weighted
 * and scaled, serves the backward: dp[b][s][c] = gscale[0] (A + t_c (Bc + G f'(p))), f = (1 - p)^gf log max(p, 1e-6), written
 * (accumulate == 0) or added into what dp holds (accumulate != 0); pass the forward's focal_gamma.
 * Per-workgroup partials folded in a fixed order, no floating-point atomics: two calls agree bit for bit; no host read, capturable.
 * sums: ltu_loss_imb_ws_floats(B, S, C) floats, no initialisation (0: a shape the calls refuse).
 * LTU_E_SHAPE: C outside 2 .. 8, B < 1, S < 1, B C 4 > 256 (the finalize kernel's rows, as ltu_loss_wide_fwd); LTU_E_ARG: a NULL
 * pointer (base_total, focal_alpha and scale_dev may be NULL; classes and w when K == 0), K outside 0 .. 8, short sums or coef, a
 * term of a class >= C, a non-finite weight or parameter, a parameter outside the ranges above; all before anything is launched. */
long long ltu_loss_imb_ws_floats(int B, long long S, int C);
int ltu_loss_imb_fwd(const float* p, const uint8_t* label, float* sums, long long sums_floats, float* values /* K + 3 */,
                     float* coef /* [B][C][3] */, const float* base_total, const int* classes, const float* w, int K,
                     const float* params /* 5 */, float w_focal, float focal_gamma, const float* focal_alpha, const float* scale_dev,
                     int B, long long S, int C, ltu_stream_t s);
int ltu_loss_imb_bwd(const float* p, const uint8_t* label, const float* coef, long long coef_floats, float focal_gamma,
                     const float* gscale, float* dp, int accumulate, int B, long long S, int C, ltu_stream_t s);
/* ---- soft morphology, soft skeleton and soft-clDice (csrc/softmorph.hip) ---------------------------------------------------------
 * Volumes are f32 [N][H][W][D], N any leading product, H W D < 2^31.  op 0, erode: the minimum over the 7-voxel cross (centre, -H, +H,
 * -W, +W, -D, +D); op 1, dilate: the maximum over the 3 x 3 x 3 cube.  Taps outside the volume are left out.  tap u8 [N][H][W][D]
 * receives the code of the first tap that attains the extremum, centre first (erode: 0 centre, 1 .. 6 in the order above; dilate:
 * 9 (dh + 1) + 3 (dw + 1) + (dd + 1), centre 13, the others visited in raster order), and the backward gives the whole gradient of an
 * output voxel to that tap, as a gather: no atomics, two calls agree bit for bit.
 * Skeleton, 1 <= iters <= 10: I_0 = x, I_{j+1} = erode(I_j), D_j = dilate(I_{j+1}), delta_j = relu(I_j - D_j), s_0 = delta_0, s_j =
 * s_{j-1} + relu(delta_j - s_{j-1} delta_j), y = s_iters, relu'(0) = 0.  scratch: ltu_soft_skeleton_scratch_elems(..) 4-byte elements,
 * no initialisation; the forward leaves I_1 .. I_{iters+1} and the taps in it (6 bytes per voxel and erosion) and the backward, which
 * reads the scratch its forward wrote, uses the rest (4 bytes per voxel and erosion, and 8).
 * ltu_label_skeletons: out u8 [B][K][H][W][D] = the skeleton of the 0 / 1 maps [label == classes[k]], byte for byte what the float
 * chain gives on them, computed on the bytes of `out` alone (no scratch).
 * LTU_E_SHAPE: an extent < 1, H W D >= 2^31; LTU_E_ARG: a NULL pointer, op outside {0, 1}, iters outside 1 .. 10, K outside 1 .. 8,
 * a class listed twice, a short scratch; all before anything is launched. */
long long ltu_soft_skeleton_scratch_elems(long long N, int H, int W, int D, int iters);
int ltu_soft_morph_fwd(const float* x, float* y, uint8_t* tap, int op, long long N, int H, int W, int D, ltu_stream_t s);
int ltu_soft_morph_bwd(const float* g_out, const uint8_t* tap, float* dx, int op, long long N, int H, int W, int D, ltu_stream_t s);
int ltu_soft_skeleton_fwd(const float* x, float* y, void* scratch, long long scratch_elems, long long N, int H, int W, int D,
                          int iters, ltu_stream_t s);
int ltu_soft_skeleton_bwd(const float* x, const float* g_out, float* dx, void* scratch, long long scratch_elems, long long N, int H,
                          int W, int D, int iters, ltu_stream_t s);
int ltu_label_skeletons(const uint8_t* label, const int* classes, int K, uint8_t* out, int B, int H, int W, int D, int iters,
                        ltu_stream_t s);
/* The fifth stage of a level's loss chain: soft-clDice (Shit et al., CVPR 2021), one term per named class.  p f32 [B][H][W][D][C]
 * probabilities (2 <= C <= 8), label u8 [B][H][W][D], skel u8 [B][K][H][W][D] (ltu_label_skeletons with the same classes and iters).
 * Term k, c = classes[k] (distinct, < C): P = p[..., c], G = [label == c], S_P = skeleton(P), S_G = skel[:, k], sums over the batch:
 *     Tprec = (sum S_P G + 1) / (sum S_P + 1)    Tsens = (sum S_G P + 1) / (sum S_G + 1)    value_k = 1 - 2 Tprec Tsens / (Tprec + Tsens)
 * values [K + 1] = {total, value_0 ..}, total = (base_total ? base_total[0] : 0) + scale sum_k w[k] value_k, scale = scale_dev ?
 * scale_dev[0] : 1 read on the device.  bwd: dp[..., c] gets gscale[0] times the gradient (through S_P, and S_G / (sum S_G + 1)
 * directly), written with zeros in every other channel (accumulate == 0) or added into what dp holds.  The sums are taken in double
 * and folded in a fixed order; no atomics, no host read, capturable; two calls agree bit for bit.
 * scratch: ltu_loss_cldice_scratch_elems(..) 4-byte elements on an 8-byte boundary (else LTU_E_ALIGN), no initialisation; the backward reads the
 * scratch its forward wrote (with the same classes and iters).
 * LTU_E_SHAPE: C outside 2 .. 8, K outside 1 .. 8, an extent < 1; LTU_E_ARG: a NULL pointer (base_total and scale_dev may be), iters
 * outside 1 .. 10, a class >= C or listed twice, a non-finite weight, a short scratch; all before anything is launched. */
long long ltu_loss_cldice_scratch_elems(int B, int H, int W, int D, int K, int iters);
int ltu_loss_cldice_fwd(const float* p, const uint8_t* label, const uint8_t* skel, const int* classes, const float* w, int K, int iters,
                        void* scratch, long long scratch_elems, float* values /* K + 1 */, const float* base_total,
                        const float* scale_dev, int B, int H, int W, int D, int C, ltu_stream_t s);
int ltu_loss_cldice_bwd(const float* p, const uint8_t* label, const int* classes, int K, int iters, void* scratch,
                        long long scratch_elems, const float* gscale, float* dp, int accumulate, int B, int H, int W, int D, int C,
                        ltu_stream_t s);
/* label pyramid (utils/utils_3D_embed_full.py:64,73-76): u8 [B,H,W,D] -> max over (2,2,kd) windows */
int ltu_label_maxpool(const uint8_t* x, uint8_t* y, int B, int H, int W, int D, int kd, ltu_stream_t s);

/* ---- region-based training (csrc/region.hip): R <= 8 overlapping label regions, one sigmoid channel each -------------------------
 * Region r is a set of u8 label values; a voxel's membership of all regions is one byte, bits = lut[label], lut[v] = sum_r [v in
 * region r] << r (a label in no region is background for every channel).
 * ltu_region_bits: out[i] = lut[label[i]], i < n; lut: 256 bytes of HOST memory, passed to the kernel by value.
 * ltu_bits_orpool: u8 [B,H,W,D] -> bitwise OR over the (2, 2, kd) windows of ltu_label_maxpool, kd in {1, 2}: every region's
 * indicator max-pooled on its own.  LTU_E_SHAPE: kd outside {1, 2}, H or W odd, D % kd != 0, an empty output. */
int ltu_region_bits(const uint8_t* label, const uint8_t* lut /* 256 host bytes */, uint8_t* out, long long n, ltu_stream_t s);
int ltu_bits_orpool(const uint8_t* x, uint8_t* y, int B, int H, int W, int D, int kd, ltu_stream_t s);
/* The region stage of a level's loss chain: p f32 [B][S][R] sigmoid probabilities (channels-last), bits u8 [B][S], t_r = (bits >> r)
 * & 1.  Per (sample, region), each sum accumulated directly:
 *     I = sum p t   FP = sum p (1 - t)   FN = sum t (1 - p)   E = sum -[t log max(p, 1e-6) + (1 - t) log max(1 - p, 1e-6)]
 *     BCE  = sum_{b, r} E / (B S R)
 *     D_r  = (FP + FN) / (2 I + FP + FN + 2 eps)     batch != 0: I, FP, FN summed over b first; else the mean over b of the ratio
 *     Dice = (1 / R) sum_r D_r           (D_r: the Tversky term of ltu_loss_imb_fwd at alpha = beta = 0.5, same eps)
 * values [R + 4] = {total, BCE, Dice, D_0 .. D_{R-1}, total again}, total = (base_total ? base_total[0] : 0) + scale (w_bce BCE +
 * w_dice Dice), scale = scale_dev ? scale_dev[0] : 1 read on the device.  coef [B][R][3], already weighted and scaled, serves the
 * backward: dp[b][s][r] = gscale[0] (A + t Bc + G e'(p, t)), e' the derivative of the clamped expression (-1 / p where t = 1 and p >
 * 1e-6, 1 / (1 - p) where t = 0 and 1 - p > 1e-6, else 0), written (accumulate == 0) or added into what dp holds.
 * nnU-Net applies its BCE to the logits; on probabilities clamped at 1e-6 the two differ only where |z| > 13.8.
 * Per-workgroup partials folded in a fixed order, no floating-point atomics: two calls agree bit for bit; no host read, capturable.
 * sums: ltu_loss_region_ws_floats(B, S, R) floats, no initialisation (0: a shape the calls refuse).
 * LTU_E_SHAPE: R outside 1 .. 8, B < 1, S < 1, B R 4 > 256; LTU_E_ARG: a NULL pointer (base_total and scale_dev may be NULL), short
 * sums or coef, a non-finite weight, eps not > 0, batch outside {0, 1}; all before anything is launched. */
long long ltu_loss_region_ws_floats(int B, long long S, int R);
int ltu_loss_region_fwd(const float* p, const uint8_t* bits, float* sums, long long sums_floats, float* values /* R + 4 */,
                        float* coef /* [B][R][3] */, const float* base_total, float w_bce, float w_dice, int batch, float eps,
                        const float* scale_dev, int B, long long S, int R, ltu_stream_t s);
int ltu_loss_region_bwd(const float* p, const uint8_t* bits, const float* coef, long long coef_floats, const float* gscale, float* dp,
                        int accumulate, int B, long long S, int R, ltu_stream_t s);
/* Back to labels and scoring.  p f32: channels-last [B][N][R] (planes == 0) or planes [B][R][N] (planes == 1).
 * ltu_region_labels: nnU-Net's rule - out u8 [B][N] starts at 0; for r = 0 .. R-1 in order, class_order[r] (host ints, 0 .. 255) is
 * written where p_r > thr, so a later region wins.  ltu_region_prob_bits: out[b][i] = sum_r [p_r > thr] << r.
 * ltu_region_counts: counts i64 [B][R][3] = {TP, FP, FN} between two bit-mask volumes u8 [B][N], ZERO on entry (integer atomics; the
 * library issues no memsets), then dice f32 [B][R] = 2 TP / (2 TP + FP + FN), 1 where both sides are empty.
 * LTU_E_SHAPE: R outside 1 .. 8, B outside 1 .. 65535, N < 1; LTU_E_ARG: a NULL pointer, planes outside {0, 1}, a NaN threshold, a
 * class_order entry outside 0 .. 255. */
int ltu_region_labels(const float* p, int planes, const int* class_order, float thr, uint8_t* out, int B, long long N, int R,
                      ltu_stream_t s);
int ltu_region_prob_bits(const float* p, int planes, float thr, uint8_t* out, int B, long long N, int R, ltu_stream_t s);
int ltu_region_counts(const uint8_t* pred_bits, const uint8_t* true_bits, long long* counts, float* dice, int B, long long N, int R,
                      ltu_stream_t s);

/* ---- sliding-window whole-volume inference (inference_embed_attn.py:92-185; monai 0.7.0 sliding_window_inference) --------
 * The windows live in the PADDED image Hp x Wp x Dp (a dimension smaller than the window is padded symmetrically with zeros:
 * pad_lo = (roi - dim) / 2).  ltu_window_gather_mirror and ltu_window_blend (below) gather them and accumulate
 * votes f32 [B][C][Hp][Wp][Dp] and count f32 [B][Hp][Wp][Dp] (the sum of the weights; zero-filled before the first blend) for
 * every blending mode; finalize: out f32 [B][C][H][W][D] = votes / count without the padding, pad_lo = (ph, pw, pd). */
int ltu_vote_finalize(const float* votes, const float* count, float* out, int B, int C, int H, int W, int D, int Hp, int Wp, int Dp,
                      int ph, int pw, int pd, ltu_stream_t s);
/* ---- window gather and blending (monai 0.7.0 sliding_window_inference mode="constant" / "gaussian", plus mirror test-time
 * augmentation) ----------------------------------------------------------------------------------------------------------------
 * desc is a HOST int32 array [n][5] = (sample b, h0, w0, d0, mask) of n <= LTU_BLEND_ITEMS_MAX items (the descriptors travel as
 * kernel arguments); (h0, w0, d0) is the window start in the padded image Hp x Wp x Dp, which holds vol [B][H][W][D] at offset
 * pad_lo = (Hp - H) / 2 per axis (zeros elsewhere); bit a of mask flips axis a (0 = H, 1 = W, 2 = D) of the window.
 * gather_mirror: win [n][h][w][d] with win[k][u] = padded[b][start + u'], u'_a = r_a - 1 - u_a on a flipped axis, else u_a.
 * blend: seg f32 [n][h][w][d][C] channels-last (one-hot or softmax), 1 <= C <= 8; for every padded voxel p covered by item k,
 * v = p - start_k, u = v flipped as above: votes[b][c][p] += w(v) seg[k][u][c], wsum[b][p] += w(v), w(v) = max(g0[v0] g1[v1]
 * g2[v2], wmin) with device tables g0 [h], g1 [w], g2 [d] (tables of ones and wmin = 1: constant weights).  No atomics: each covered
 * voxel is read and written once per launch by one thread, which applies the covering items in item order, so the sums do not
 * depend on how the items are split into launches.  ltu_vote_finalize(votes, wsum, ...) divides and crops.
 * LTU_E_ARG: a NULL pointer, n outside 0 .. LTU_BLEND_ITEMS_MAX, a mask above 7; LTU_E_SHAPE: C outside 1 .. 8, a window larger
 * than the padded image, an image larger than the padded one, h w d >= 2^31, b outside 0 .. B-1, a window not inside the padded
 * image.  Both refuse before any HIP call. */
#define LTU_BLEND_ITEMS_MAX 32
int ltu_window_gather_mirror(const float* vol, float* win, const int* desc, int n, int B, int H, int W, int D, int Hp, int Wp, int Dp,
                             int h, int w, int d, ltu_stream_t s);
int ltu_window_blend(const float* seg, float* votes, float* wsum, const float* g0, const float* g1, const float* g2, float wmin,
                     const int* desc, int n, int B, int C, int Hp, int Wp, int Dp, int h, int w, int d, ltu_stream_t s);
/* evaluation metrics of the driver on p = [pred[b][ci] >= threshold] against target u8 [B][H][W][D] (0/1):
 * values[0..3] = DiceClassLoss (criterions.py:35-70), Recall (280-311), Precision (348-379), LocalizationLoss (179-241),
 * means over the batch; rows f32 [B][3][H] scratch (per-h sums of p, t, p*t over W*D = WD elements). */
int ltu_seg_metrics(const float* pred, const uint8_t* target, float* rows, float* values, int B, int C, int ci, int H, long long WD,
                    float threshold, ltu_stream_t s);

/* surface-distance metrics of the evaluation (no reference counterpart; csrc/surface.hip): per (sample b, class k) with
 * A = pred[b][k] >= threshold and B = target[b] == k, the boundary dX = voxels of X with a face neighbour outside X (beyond the
 * volume counts as outside), d(x, dY) = min over y in dY of sqrt(sum_i ((x_i - y_i) s_i)^2), DA = d(dA, dB), DB = d(dB, dA):
 * HD = max(max DA, max DB), HD95 = max(P95 DA, P95 DB) (numpy's linear percentile), ASSD = (sum DA + sum DB) / (|dA| + |dB|),
 * NSD = (#{DA <= tau} + #{DB <= tau}) / (|dA| + |dB|) (boundary-voxel counts, not surfel areas).  Both boundaries empty:
 * 0 / 0 / 0 / 1; exactly one empty: inf / inf / inf / 0.  A box (h0, w0, d0, h, w, d) is a crop of the [H][W][D] volume.
 *   boundary: pred f32 [B][C][H][W][D], target u8 [B][H][W][D] -> edges u8 [B][H][W][D] (bit 0 = dA, bit 1 = dB) and bbox int32
 *             [B][6] = (min h, w, d, max h, w, d) of dA u dB (max < 0: both empty), found with integer atomics.
 *   edt:      dist f32 [2][h][w][d] = exact squared distance, spacing (sh, sw, sd) > 0, from every voxel of the box to the
 *             nearest voxel of bit 0 (channel 0) and of bit 1 (channel 1) of edges [H][W][D] inside the box, +inf without one;
 *             with unit spacing every finite value is an integer below 2^24 (axes up to 2048) and exact.
 *   stats:    from edges + dist over the same box, rec f64 [12] = |dA|, |dB|, max DA, max DB, sum DA, sum DB, #{DA <= tau},
 *             #{DB <= tau}, then the floor / ceil order statistics of the 95th percentile of DA and of DB (radix select on the
 *             device).  Per-workgroup partials folded in a fixed order: two calls give bit-identical records.
 *   finalize: out f32 [4][B][K] = HD, HD95, ASSD, NSD from rec [K][B][12] (a pair whose boundaries are both empty keeps its
 *             zero-filled record).
 * scratch of edt and stats: ltu_surface_ws_elems(h, w, d) 4-byte elements of the box. */
int ltu_surface_boundary(const float* pred, const uint8_t* target, uint8_t* edges, int* bbox, int B, int C, int k, int H, int W,
                         int D, float threshold, ltu_stream_t s);
long long ltu_surface_ws_elems(int h, int w, int d);
int ltu_surface_edt(const uint8_t* edges, float* dist, void* scratch, long long scratch_elems, int H, int W, int D, int h0, int w0,
                    int d0, int h, int w, int d, float sh, float sw, float sd, ltu_stream_t s);
int ltu_surface_stats(const uint8_t* edges, const float* dist, double* rec, void* scratch, long long scratch_elems, int H, int W,
                      int D, int h0, int w0, int d0, int h, int w, int d, float tau, ltu_stream_t s);
int ltu_surface_finalize(const double* rec, float* out, int B, int K, ltu_stream_t s);

/* multi-class evaluation metrics of inference_multi_classes.py:153 (loss/multi_criterions.py: DiceClassLoss0 30-56, DiceClassLoss /
 * DiceClassLoss2 58-110, LocalizationLoss 219-281, Recall / Recall2 320-375, Precision / Precision2 406-462) and its label map
 * (argmax(predict2, 1), line 158); csrc/class_metrics.hip.  pred f32 [B][C][H][W][D] (2 <= C <= 8), target u8 class ids
 * [B][H][W][D]; p = pred as given, or [pred >= threshold] when threshold >= 0.
 *   pass:     one read of pred and target: per (sample, row h, chunk of the row) the sums over (W, D) of p_c, [t == c],
 *             p_c [t == c] for every class and of 1 - p_0, [t != 0], (1 - p_0) [t != 0] into scratch (fp64 partials, no
 *             atomics); label_map u8 [B][H][W][D] = the arg-max over C of pred, first maximal index on ties (nullable: not written).
 *   finalize: folds the partials in a fixed order in fp64 and writes out f32 [B + 1][3C + 2].  Row b < B: Dice[C] =
 *             (2 sum pt + 1e-9) / (sum p + sum t + 1e-9), Recall[C] = (sum pt + 1e-5) / (sum t + 1e-5), Precision[C] =
 *             (sum pt + 1e-5) / (sum p + 1e-5), the foreground Dice of 1 - p_0 against [t != 0] (eps 1e-9), LocalizationLoss =
 *             mean over h of |cp_h - ct_h|, cp / ct = cumulative sums over H of sigmoid(foreground profile - 10) divided by
 *             (their sum + 1e-6).  Row B: 1 - mean Dice[C], mean Recall[C], mean Precision[C], 1 - mean foreground Dice, mean
 *             LocalizationLoss (means over the batch).  Two calls give bit-identical results.
 * scratch: ltu_class_metrics_ws_elems(B, C, H, W, D) doubles (0 for a shape the entry points refuse), written by the pass
 * and read by finalize. */
long long ltu_class_metrics_ws_elems(int B, int C, int H, int W, int D);
int ltu_class_metrics_pass(const float* pred, const uint8_t* target, uint8_t* label_map, double* scratch, long long scratch_elems,
                           int B, int C, int H, int W, int D, float threshold, ltu_stream_t s);
int ltu_class_metrics_finalize(const double* scratch, long long scratch_elems, float* out, int B, int C, int H, int W, int D,
                               ltu_stream_t s);

/* connected components and lesion-wise detection metrics of the evaluation (no reference counterpart; csrc/components.hip).
 * Connectivity c = 1, 2, 3 (6, 18, 26 neighbours: coordinates differ by at most 1 on at most c axes); voxels beyond the volume
 * are background; every sample is labelled on its own; S = H W D < 2^31 (else LTU_E_SHAPE), c outside 1 .. 3 is LTU_E_ARG.
 * Union-find over voxel indices in a fixed number of launches (no host loop, capturable): the root of a component is its
 * smallest (raster-first) voxel, so the numbering does not depend on scheduling.
 *   label:   mask u8 [B][H][W][D] (nonzero = foreground) -> labels int32 [B][H][W][D], 0 background, components numbered
 *            1 .. n_b in raster order of their first voxel (= scipy.ndimage.label with generate_binary_structure(3, c)), counts
 *            int32 [B] = n_b.  scratch: ltu_label_ws_elems(B, H, W, D) int32.
 *   remove_small: pred f32 [B][C][H][W][D] (2 <= C <= 31, rounded values) in place: for each class k with bit k of `classes` set
 *            (bit 0 must be clear), every component of pred[b][k] > 0 with fewer than min_voxels voxels is cleared in channel k;
 *            then channel 0 = 1 - the sum of the others.  scratch: ltu_remove_small_ws_elems(B, H, W, D) int32.
 *   keep_largest: the post-processing of inference_multi_classes.py:104,148-151 = monai KeepLargestConnectedComponent(
 *            applied_labels = all foreground channels, independent=False, connectivity=3) for connectivity 3: pred f32
 *            [B][C][H][W][D] (2 <= C <= 31, rounded values) in place: the foreground union (the fp32 sum of channels 1 .. C-1 in
 *            channel order > 0) of every sample is labelled, channels 1 .. C-1 are cleared at the foreground voxels outside its
 *            largest component (among equally large ones the raster-first, as bincount / argmax pick it; a sample without
 *            foreground keeps its values), then channel 0 = 1 - the sum of the others.  One call for the batch, no host read.
 *            scratch: ltu_keep_largest_ws_elems(B, H, W, D) int32, 8-byte aligned.
 *            Both in-place calls: B outside 1 .. 65535 or C outside 2 .. 31 is LTU_E_SHAPE; a NULL or short scratch is LTU_E_ARG.
 *   lesion:  for sample b and class k, P = pred[b][k] >= threshold (pred f32 [B][C][H][W][D]) and G = target[b] == k (target u8
 *            [B][H][W][D]) are labelled into P_1 .. P_m and G_1 .. G_n; o_j = |G_j n P|, G_j is detected iff o_j >= 1, P_i is a
 *            false positive iff P_i n G is empty, U_j = the union of the P_i touching G_j, Dice_j = 2 o_j / (|G_j| + |U_j|).
 *            heads: heads int32 [B] = the voxels of P n G with no half-neighbour in P n G (a bound on the distinct (P_i, G_j)
 *            pairs).  stats: with pairs >= max_b heads[b], writes column kk of ints int32 [5][B][K] = NumTrue n, NumPred m,
 *            TruePositives, FalseNegatives, FalsePositives and rates f32 [4][B][K] = Sensitivity TP / n (1 if n = 0),
 *            Precision (m - FP) / m (1 if m = 0), F1 = 2 S P / (S + P) (0 if S + P = 0), LesionDice = sum_j Dice_j / (n + FP)
 *            (1 if n + FP = 0); a pair bound found short gives -1 / NaN for that sample instead.  Integer counts and a fixed-order
 *            fp64 fold: two calls are bit-identical.  scratch: ltu_lesion_ws_elems(B, H, W, D, pairs) 4-byte elements. */
long long ltu_label_ws_elems(int B, int H, int W, int D);
int ltu_label_components(const uint8_t* mask, int* labels, int* counts, int* scratch, long long scratch_elems, int B, int H, int W,
                         int D, int connectivity, ltu_stream_t s);
long long ltu_remove_small_ws_elems(int B, int H, int W, int D);
int ltu_remove_small_components(float* pred, int* scratch, long long scratch_elems, int B, int C, int classes, int H, int W, int D,
                                int min_voxels, int connectivity, ltu_stream_t s);
long long ltu_keep_largest_ws_elems(int B, int H, int W, int D);
int ltu_keep_largest_component(float* pred, int* scratch, long long scratch_elems, int B, int C, int H, int W, int D, int connectivity,
                               ltu_stream_t s);
long long ltu_lesion_ws_elems(int B, int H, int W, int D, long long pairs);
int ltu_lesion_heads(const float* pred, const uint8_t* target, int* heads, int B, int C, int k, int H, int W, int D, float threshold,
                     int connectivity, ltu_stream_t s);
int ltu_lesion_stats(const float* pred, const uint8_t* target, int* ints, float* rates, void* scratch, long long scratch_elems,
                     long long pairs, int B, int C, int k, int kk, int K, int H, int W, int D, float threshold, int connectivity,
                     ltu_stream_t s);
/* fill_holes (scipy.ndimage.binary_fill_holes(mask[b], generate_binary_structure(3, connectivity)); monai FillHoles): mask u8
 * [B][H][W][D] (nonzero = set) -> out u8 [B][H][W][D] = 1 on the mask and on every background voxel whose background component
 * (adjacency of `connectivity`, as above) touches no face of the volume, 0 elsewhere.  The complement is labelled with the
 * union-find above, one pass over the six faces marks the roots of the components that reach a face (plain stores of one value),
 * one pass writes out: five launches, no host read, capturable; integer work only, two calls are bit-identical.  out == mask (in
 * place) is allowed: the mask is read by the labelling only.  scratch: ltu_fill_holes_ws_elems(B, H, W, D) int32 (0 for a refused
 * shape).  Shape rules and error codes as ltu_label_components; nothing is launched on a refusal. */
long long ltu_fill_holes_ws_elems(int B, int H, int W, int D);
int ltu_fill_holes(const uint8_t* mask, uint8_t* out, int* scratch, long long scratch_elems, int B, int H, int W, int D,
                   int connectivity, ltu_stream_t s);
/* The cavities of a mask: counts int32 [B] = the 6-connected background components of mask[b] that reach no face of the volume
 * (the second Betti number of the object under 26-connectivity).  The labelling and face marking of ltu_fill_holes at
 * connectivity 1, counted instead of filled; scratch: ltu_fill_holes_ws_elems(B, H, W, D) int32.  Same refusals. */
int ltu_count_cavities(const uint8_t* mask, int* counts, int* scratch, long long scratch_elems, int B, int H, int W, int D,
                       ltu_stream_t s);

/* ---- topology: curve skeleton, clDice overlap counts, Euler characteristic (csrc/thinning.hip) ---------------------------------
 * Volumes are u8 [N][H][W][D], nonzero = object, everything beyond a volume is background.  N in 1 .. 65535, H W D < 2^31 and
 * N H W D < 2^32, else LTU_E_SHAPE; a NULL pointer or a short scratch is LTU_E_ARG; nothing is launched on a refusal.  Integer
 * work only: two calls give the same bytes.
 *   code     of a voxel p: bit 9 (dh + 1) + 3 (dw + 1) + (dd + 1) is set when p + (dh, dw, dd) is object; bit 13 is ignored.
 *   simple_codes: flags[i] bit 0 = codes[i] is simple for the (26, 6) pair (its 26 neighbours hold exactly one 26-component of
 *            object, and exactly one 6-component of the background of its 18-neighbourhood holds a face neighbour), bit 1 = it is
 *            an endpoint (exactly one object neighbour).  The device function the thinning calls.
 *   thinning: 8-subfield sequential curve thinning.  One iteration marks the object voxels with a background face neighbour as
 *            candidates, then for s = 0 .. 7 deletes, in place, every candidate of subfield (h & 1) | (w & 1) << 1 | (d & 1) << 2
 *            == s that is simple and not an endpoint in the current image.  The result does not depend on scheduling.
 *            count: counts int64 [8] (device) = the object voxels per subfield over all N volumes; their sum sizes the scratch.
 *            iterate: enqueues `iters` (1 .. 64) iterations on vol, 10 launches each; deleted int64 [iters] (device) receives the
 *            voxels each of them deleted.  An iteration on a converged volume deletes nothing, so the host may read `deleted` as
 *            rarely as it likes and stop at the first zero.  counts must be ltu_thin_count's of vol before its first iteration,
 *            objects their sum.  scratch: ltu_thin_ws_elems(N, H, W, D, objects) int32 (0 for what the call refuses).
 *   clDice   for column kk of K and class k: binarize writes out u8 [2][B][K][H][W][D], side 0 = pred[b][k] >= threshold (pred
 *            f32 [B][C][H][W][D]), side 1 = target[b] == k (target u8 [B][H][W][D]); overlap takes the thinned copy of that
 *            array and writes counts int32 [B][K][4] = |S_P|, |S_P n G|, |S_G|, |S_G n P| and rates f32 [3][B][K] = clDice
 *            2 Tp Ts / (Tp + Ts) (0 when Tp + Ts = 0), Tprec |S_P n G| / |S_P|, Tsens |S_G n P| / |S_G| (quotients in fp64, one
 *            rounding to f32); both skeletons empty: 1, 1, 1; exactly one empty: 0, 0, 0.  2 B K volumes follow the rules above.
 *   euler    chi int64 [N] (device) = V - E + F - C of the union of the closed unit cubes of the object voxels: the cell complex of
 *            26-connectivity, so chi = b0 - b1 + b2. */
int ltu_thin_simple_codes(const uint32_t* codes, uint8_t* flags, long long n, ltu_stream_t s);
int ltu_thin_count(const uint8_t* vol, long long* counts, int N, int H, int W, int D, ltu_stream_t s);
long long ltu_thin_ws_elems(int N, int H, int W, int D, long long objects);
int ltu_thin_iterate(uint8_t* vol, const long long* counts, long long* deleted, int iters, int* scratch, long long scratch_elems,
                     long long objects, int N, int H, int W, int D, ltu_stream_t s);
int ltu_topology_binarize(const float* pred, const uint8_t* target, uint8_t* out, int B, int C, int k, int kk, int K, int H, int W,
                          int D, float threshold, ltu_stream_t s);
int ltu_topology_overlap(const float* pred, const uint8_t* target, const uint8_t* skel, int* counts, float* rates, int B, int C, int k,
                         int kk, int K, int H, int W, int D, float threshold, ltu_stream_t s);
int ltu_euler_characteristic(const uint8_t* vol, long long* chi, int N, int H, int W, int D, ltu_stream_t s);

/* ---- optimizer (train3D.py:193: torch.optim.AdamW(lr=1e-4)) -----------------------------------------------------
 * One AdamW step on flat, 16-byte aligned fp32 buffers (a gradient bucket and the parameters / moments laid out the same way):
 * decoupled weight decay, bias correction with `step` (>= 1), gradient multiplied by grad_scale on load. */
int ltu_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
              float weight_decay, long long step, float grad_scale, ltu_stream_t s);
/* The guarded step (csrc/optim.hip): clipping by the global gradient norm, skipping a step whose gradient is not finite (what
 * GradScaler.step does in utils/utils_3D_monai.py:103-105) and an exponential moving average of the weights, in
 * 2 x buckets + 1 launches with no host read and no atomics.  All buffers are 16-byte aligned fp32 unless stated.
 *   sequence    for each bucket b: ltu_grad_sumsq(g_b, n_b, grad_scale, scratch + off_b, cap - off_b) with off_b = the sum of
 *               ltu_grad_sumsq_parts(n) over the buckets before b, then ONE ltu_adamw_guard(scratch, sum of all parts, state, ...),
 *               then for each bucket ltu_adamw_guarded(..., state).
 *   sumsq       one fp32 partial per workgroup = the sum of (g[i] * grad_scale)^2 over the workgroup's elements.  The number of
 *               partials, ltu_grad_sumsq_parts(n), depends on n ONLY (no knob, no environment), so the query and the launch
 *               cannot disagree.  scratch needs 4-byte alignment only (rows of several buckets lie next to each other).
 *   guard       folds `parts` partials in index order in fp64 and updates the GUARD STATE, LTU_GUARD_STATE_BYTES = 48 bytes that
 *               the caller zero-fills once and the kernels own from then on.  32-bit words:
 *                 0  norm     f32  sqrt of the sum: the norm of the scaled gradient before clipping (clip_grad_norm_'s return value)
 *                 1  coef     f32  grad_scale * min(1, max_norm / (norm + 1e-6)); grad_scale when max_norm <= 0; 0 on a skipped step
 *                 2  bc1      f32  1 - beta1^applied, computed in double
 *                 3  bc2      f32  1 - beta2^applied, computed in double
 *                 4  skip     i32  1 iff skip_nonfinite != 0 and norm is inf or NaN (an inf / NaN anywhere in a bucket, or a
 *                                  finite gradient whose square overflows fp32, makes the sum non-finite)
 *                 5  reserved
 *                 6-7  applied  i64  steps applied so far (the t of the bias corrections); a skipped step leaves it and bc1 / bc2 alone
 *                 8-9  skipped  i64  steps skipped so far
 *                 10-11  reserved
 *               The counters live on the device so that a skipped step does not advance the bias correction and the host never
 *               has to read the decision back (the sequence can be captured into a graph and replayed).
 *   guarded     ltu_adamw's arithmetic in the same order with grad_scale = coef and the bias corrections bc1 / bc2 of the state.
 *               skip = 1: returns without writing anything.  ema (nullable): ema = ema_decay * ema + (1 - ema_decay) * p_new in
 *               the same pass; ema_decay must be in [0, 1) then.
 * Two calls on the same buckets give bit-identical results; data-parallel ranks hold identical reduced buckets and so take
 * identical decisions without communication (like every N > 1 path here this has not run on hardware).
 * LTU_E_ARG: a scratch shorter than the launch writes, a misaligned or NULL pointer, a NaN max_norm, a bad ema_decay. */
#define LTU_GUARD_STATE_BYTES 48
long long ltu_grad_sumsq_parts(long long n);
int ltu_grad_sumsq(const float* g, long long n, float grad_scale, float* scratch, long long scratch_floats, ltu_stream_t s);
int ltu_adamw_guard(const float* scratch, long long parts, void* state, float grad_scale, float max_norm /* <= 0: no clipping */,
                    int skip_nonfinite, float beta1, float beta2, ltu_stream_t s);
int ltu_adamw_guarded(float* p, const float* g, float* m, float* v, float* ema /* nullable */, long long n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float ema_decay, const void* state, ltu_stream_t s);
/* SGD with momentum / Nesterov (train3D.py:194: torch.optim.SGD(lr=1e-4, momentum=0.9); nnU-Net: momentum 0.99, Nesterov, weight
 * decay 3e-5) on the same flat, 16-byte aligned fp32 buffers, torch.optim.SGD's arithmetic per element:
 *   g' = g * coef;  weight_decay != 0: g' += weight_decay * p
 *   momentum != 0: buf = g' on the first applied step, buf = momentum * buf + (1 - dampening) * g' afterwards;
 *                  g' = g' + momentum * buf (nesterov) or g' = buf
 *   p -= lr * g';  ema = ema_decay * ema + (1 - ema_decay) * p (guarded form, ema != NULL)
 * Every multiply-add is an explicit fmaf (csrc/optim.hip states the expression), so the plain and the guarded form, with or
 * without an EMA, give the same parameter and buffer bits for the same inputs.  buf is NULL iff momentum == 0 (no buffer is read
 * or written then).
 *   ltu_sgd          coef = grad_scale, lr and first_step (!= 0: the first step) from the host, as ltu_adamw takes lr and step.
 *   ltu_sgd_guarded  after ltu_grad_sumsq per bucket and ONE ltu_adamw_guard (betas 0; bc1 / bc2 are not read) it takes coef, skip
 *                    and first = (applied == 1) from the guard state: a skipped first step leaves the first case to the next applied
 *                    one.  skip = 1: returns without writing anything.  The learning rate is read from DEVICE memory (lr_dev, one
 *                    fp32, 4-byte aligned, a uniform load), so a captured launch stays valid while a schedule moves the value.
 * LTU_E_ARG (nothing launched, nothing written): a NULL or misaligned pointer (16 bytes for buffers and state, 4 for lr_dev), buf
 * present without momentum or absent with it, a negative or NaN lr / momentum / weight_decay, a NaN dampening or grad_scale, nesterov
 * with momentum <= 0 or dampening != 0, ema_decay outside [0, 1) with an EMA buffer.  n <= 0 with valid scalars: LTU_OK. */
int ltu_sgd(float* p, const float* g, float* buf /* NULL iff momentum == 0 */, long long n, float lr, float momentum, float dampening,
            float weight_decay, int nesterov, int first_step, float grad_scale, ltu_stream_t s);
int ltu_sgd_guarded(float* p, const float* g, float* buf /* NULL iff momentum == 0 */, float* ema /* nullable */, long long n,
                    const float* lr_dev, float momentum, float dampening, float weight_decay, int nesterov, float ema_decay,
                    const void* state, ltu_stream_t s);

/* ---- data-parallel gradient exchange (replaces the reduce half of nn.DataParallel, train3D.py:119) -------------------------------
 * Direct RCCL calls: one communicator per process (= per GPU), created from a 128-byte unique id that rank 0 generates and the
 * host side distributes (lintransunet_amd/comm.py: over the gloo control group).  librccl is not linked: ltu_comm_load dlopens
 * the copy the process already holds (PyTorch's torch/lib/librccl.so, bound to the HIP runtime that owns the caller's streams).
 * The all-reduce only ENQUEUES RCCL's kernel on `s`: no thread, no event polling, no synchronisation - inside a stream capture it
 * becomes a graph node (train.GraphedStep captures every bucket's all-reduce as a side branch of the step graph).
 * `comm` is an opaque handle owned by the caller; the only process-global state are the resolved function pointers.
 *   ltu_comm_allreduce_avg: buf[i] <- mean over ranks of buf[i] (fp32, in place, ncclAvg)
 *   ltu_comm_broadcast:     nbytes of buf from rank `root` to all (initial parameter sync) */
int ltu_comm_load(const char* librccl_path);
int ltu_comm_unique_id(void* id128);
int ltu_comm_init(void** comm, const void* id128, int world, int rank);
int ltu_comm_allreduce_avg(void* comm, float* buf, long long n, ltu_stream_t s);
int ltu_comm_broadcast(void* comm, void* buf, long long nbytes, int root, ltu_stream_t s);
int ltu_comm_destroy(void* comm);

/* ---- data side (dataset/CT_pancreas_ids.py:143-173): raw scan f32 [D][H][W] -> img f32 [H][W][D] = (clamp(raw, lo, hi) - mean) / std,
 * raw label u8 [D][H][W] -> lab u8 [H][W][D] (either pair may be NULL); reference constants lo -91, hi 250, mean 86.9, std 39.4 */
int ltu_ct_preprocess(const float* raw, float* img, const uint8_t* rawlab, uint8_t* lab, int D, int H, int W, float lo, float hi,
                      float mean, float std, ltu_stream_t s);
/* patches out [n][h][w][d] cut from vol [H][W][D] (elem_bytes 4 = f32, 1 = u8) at desc int32 [n][5] = (h0, w0, d0, flip_h, flip_w):
 * the crop of monai RandCropByPosNegLabeld at host-chosen centres followed by RandFlipd over the first two spatial axes */
int ltu_crop_flip(const void* vol, void* out, const int* desc, int n, int H, int W, int D, int h, int w, int d, int elem_bytes,
                  ltu_stream_t s);

/* ---- augmentations of the training dataset (dataset/CT_pancreas_ids.py:112-134; monai 0.7.0 RandRotated, RandAdjustContrastd,
 * RandZoomd) on batches of patches [n][H][W][D] f32 (image and label alike: the reference interpolates both and casts the
 * label back to uint8 at the end).  Random draws stay on the host; a sample that skips a transform gets the identity matrix /
 * zoom 1 / gamma <= 0, all of which reproduce the input exactly.
 * affine: out[k][p] = trilinear(in[k], M_k (p,1)), M_k = mats[k] (3x4 row-major, voxel coordinates), border padding.
 * zoom:   interpolate to zsize[k] = floor(size * zoom_k) per axis (int32 [n][3], computed by the caller in double precision as
 *         torch does; trilinear, align_corners) + centred edge pad / crop back to [H][W][D].
 * contrast: ((x - min)/(max - min + 1e-7))^gamma[k] * (max - min) + min over each patch; minmax_ws: 2 n ints. */
int ltu_affine_sample(const float* in, float* out, const float* mats, int n, int H, int W, int D, ltu_stream_t s);
int ltu_zoom_sample(const float* in, float* out, const int* zsize, int n, int H, int W, int D, ltu_stream_t s);
int ltu_adjust_contrast(const float* in, float* out, const float* gamma, int* minmax_ws, int n, long long per, ltu_stream_t s);

/* ---- data side of the monai driver (dataset/CT_pancreas_monai.py:37-58, 91-105; monai 0.7.0 Spacingd + Orientationd('RAS'),
 * RandCropByPosNegLabeld, RandFlipd(spatial_axis 0), RandRotate90d(spatial_axes (0, 1))); csrc/resample.hip.
 * resample_grid: for every output voxel p (shape O0 x O1 x O2, element strides os0..2) the source coordinate is c = M (p, 1), M =
 *   mat, a float64 [3][4] pull matrix in device memory (row s = source axis s of the source of shape S0 x S1 x S2, element strides
 *   ss0..2).  c is clamped to [0, size - 1] per axis (grid_sample border padding, align_corners False, in voxel units).
 *   image: trilinear over the 8 taps, each tap mapped first: clamp(alpha * v + beta, lo, hi) (NIfTI slope / intercept, then
 *          ScaleIntensityRange and its clip folded into one affine map by the caller); src_dtype LTU_U8 / LTU_I16 / LTU_F32, out f32.
 *   label: u8 source voxel at the round-half-even of the clamped c (grid_sample nearest), out u8.
 *   Either pair (src_img, out_img) / (src_lab, out_lab) may be NULL, not both; given both, one launch writes both outputs.
 *   lane_axis: the output axis whose step moves the source address least (the caller knows M); the kernel walks it across the lanes
 *   of a wave and, when it is not the output's fastest axis, transposes 64 x 64 tiles through LDS before the store.
 *   No workspace.  LTU_E_ARG: NULL mat, unpaired pointers, lane_axis outside 0..2; LTU_E_DTYPE: src_dtype; LTU_E_SHAPE: a size or
 *   stride < 1. */
enum { LTU_U8 = 2, LTU_I16 = 3 };
int ltu_resample_grid(const void* src_img, int src_dtype, const uint8_t* src_lab, int S0, int S1, int S2, long long ss0, long long ss1,
                      long long ss2, float* out_img, uint8_t* out_lab, int O0, int O1, int O2, long long os0, long long os1,
                      long long os2, const double* mat, int lane_axis, float alpha, float beta, float lo, float hi, ltu_stream_t s);
/* resample_argmax: the way back of a prediction.  probs: C planar f32 channels (channel c at probs + c * cs) of one volume of shape
 *   S0 x S1 x S2 (element strides ss0..2), C = 2 .. 8.  Every output voxel p gets the coordinate, the clamp, the taps and the
 *   weights of resample_grid once; class c's value there is the trilinear sum of channel c, bit for bit what resample_grid gives
 *   for that channel as an LTU_F32 source with alpha 1, beta 0, lo -inf, hi +inf.  out_lab (u8, shape O0 x O1 x O2, strides
 *   os0..2) = the first maximal class (strict > scanning c = 0 .. C-1: torch.argmax, class_metrics_pass's label map).
 *   class_mask: bit c set stores class c's resampled value too, into plane j of out_prob (f32, plane stride ocs, each plane laid
 *   out as out_lab), j = the number of set bits below c; 0 stores labels only (out_prob and ocs are then ignored).
 *   lane_axis and the 64 x 64 tile as for resample_grid; both outputs go through LDS when lane_axis is not the output's fastest
 *   axis.  Tap offsets inside a channel are 32-bit while (S - 1) . ss < 2^31, the channel base is a 64-bit pointer offset.
 *   No workspace, no atomics: two calls give the same bytes.  LTU_E_ARG: NULL probs, mat or out_lab, lane_axis outside 0..2,
 *   class_mask negative or with a bit >= C, class_mask != 0 with NULL out_prob; LTU_E_SHAPE: C outside 2..8, a size or stride < 1
 *   (cs always, ocs when class_mask != 0). */
int ltu_resample_argmax(const float* probs, int C, long long cs, int S0, int S1, int S2, long long ss0, long long ss1, long long ss2,
                        uint8_t* out_lab, float* out_prob, int class_mask, long long ocs, int O0, int O1, int O2, long long os0,
                        long long os1, long long os2, const double* mat, int lane_axis, ltu_stream_t s);
/* resample_vote: the label by class vote, nnU-Net's label resampling ("one-hot, order 1": every class's indicator map interpolated
 *   linearly, then the arg-max) without a one-hot volume, a class count or a float volume.  src_lab (u8, shape S0 x S1 x S2, element
 *   strides ss0..2), out_lab (u8, shape O0 x O1 x O2, strides os0..2), mat and lane_axis as resample_grid's.  The rule, for one
 *   output voxel: the coordinate c = M (p, 1), its clamp to [0, size - 1], the lower tap index floor(c) and the fp32 upper weights
 *   t[s] = (float)(c[s] - floor(c[s])) are resample_grid's image path; the 8 taps are taken in its order k = 0 .. 7 (bit 0 of k:
 *   source axis 0, bit 1: axis 1, bit 2: axis 2; the upper tap of an axis at its last index is that index again, weight t).
 *     tap k has the weight w_k = (k & 1 ? t[0] : 1 - t[0]) * (k & 2 ? t[1] : 1 - t[1]) * (k & 4 ? t[2] : 1 - t[2]) in fp32, rounded
 *       before it is added, and the label l_k, the u8 voxel at the tap (the coordinate is clamped: there is no outside);
 *     the score of a value v is s_v = sum of w_k over the taps with l_k == v, added in tap order with plain fp32 adds;
 *     out_lab = the SMALLEST v whose score is maximal, compared exactly on the fp32 scores (torch.argmax's first maximum).
 *   Every u8 value 0 .. 255 is a class of its own.  s_c has the bits of resample_argmax's value on the float32 one-hot channel of c
 *   (each w * 1 rounded, then added; added zeros change nothing): the label equals resample_argmax's on the one-hot channels byte
 *   for byte.  A matrix that lands on integer coordinates gives weights 1 and 0: the nearest label.  The same 64 x 64 LDS transpose
 *   when lane_axis is not the output's fastest axis; 8 byte loads per voxel, the vote in registers: no workspace, no atomics, two
 *   calls give the same bytes.  LTU_E_ARG: NULL src_lab, out_lab or mat, lane_axis outside 0..2; LTU_E_SHAPE: a size or stride < 1. */
int ltu_resample_vote(const uint8_t* src_lab, int S0, int S1, int S2, long long ss0, long long ss1, long long ss2, uint8_t* out_lab,
                      int O0, int O1, int O2, long long os0, long long os1, long long os2, const double* mat, int lane_axis,
                      ltu_stream_t s);
/* ---- cubic B-spline resampling (csrc/spline.hip; nnU-Net's image interpolation, no reference counterpart: the driver's Spacingd is
 * trilinear).  Two calls: spline_prefilter turns a stored scan into B-spline coefficients, resample_spline gathers them through the
 * pull matrix of resample_grid.  order0..2 (one per SOURCE axis, each 0, 1 or 3) mean the same in both calls.
 * spline_prefilter: src as resample_grid's src_img (src_dtype LTU_U8 / LTU_I16 / LTU_F32, shape S0 x S1 x S2, element strides
 *   ss0..2); every voxel is mapped as it is loaded, clamp(alpha * v + beta, lo, hi).  coef: dense f32, S0 S1 S2 elements, axis 0
 *   fastest (strides 1, S0, S0 S1).  An axis of order 3 and length > 1 is filtered along itself as scipy.ndimage.spline_filter1d(
 *   order 3, mode 'mirror'): pole z = sqrt(3) - 2, the samples times the gain 6, a causal recursion c+[i] = s[i] + z c+[i-1] from
 *   c+[0] = sum_k z^k s[mirror(k)] (whole-sample mirror, period 2 n - 2: the exact periodic sum for n <= 24, cut after 24 terms
 *   above that, |z|^24 = 1.9e-14), then c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]), c[i] = z (c[i+1] - c+[i]).  An axis of order
 *   0 or 1, or of length 1, is left alone.  Axis 0 goes through 16 x 64 LDS tiles with the recursion state carried along the line,
 *   axes 1 and 2 are walked in place with the lanes along axis 0.  fp32, explicit fused multiply-adds in a fixed order, no atomics,
 *   no workspace: two calls give the same bytes.  LTU_E_ARG: NULL src or coef, an order outside {0, 1, 3}, a NaN in the map;
 *   LTU_E_DTYPE: src_dtype; LTU_E_SHAPE: a size or stride < 1, a volume of 2^31 voxels or more. */
int ltu_spline_prefilter(const void* src, int src_dtype, int S0, int S1, int S2, long long ss0, long long ss1, long long ss2,
                         float* coef, int order0, int order1, int order2, float alpha, float beta, float lo, float hi,
                         ltu_stream_t s);
/* resample_spline: out[p] = clamp(sum_ijk w0[i] w1[j] w2[k] coef[tap0[i]][tap1[j]][tap2[k]], lo, hi) at c = M (p, 1), formed and
 *   clamped to [0, size - 1] exactly as resample_grid does (mat, out shape O0 x O1 x O2, strides os0..2, lane_axis and the two tile
 *   paths as there).  coef: what spline_prefilter wrote for the same orders (dense, axis 0 fastest).  Per source axis, f = floor(c),
 *   t = c - f: order 3 taps f-1 .. f+2 with weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6; order 1 taps f, f+1
 *   with (1-t, t); order 0 the tap floor(c + 1/2).  A tap index outside [0, n-1] is mirrored (whole-sample, period 2 n - 2; 0 when
 *   n = 1).  The sum runs in fp32 in a fixed order: axis 0 innermost as a fused multiply-add chain, then (w2 w1) row added by one
 *   fused multiply-add, axis 1 inside axis 2.  lo / hi: the intensity map's clip (the spline rings past a clipped window); -inf /
 *   +inf leave the sum as it is.  Orders built: (3, 3, 3), and 3 on two axes with 0 or 1 on the third; any other triple of
 *   {0, 1, 3} is LTU_E_ARG, as are a NULL pointer, lane_axis outside 0..2 and a NaN bound.  LTU_E_SHAPE: a size or stride < 1, a
 *   coefficient volume of 2^31 elements or more (tap offsets are 32-bit). */
int ltu_resample_spline(const float* coef, int S0, int S1, int S2, int order0, int order1, int order2, float* out, int O0, int O1,
                        int O2, long long os0, long long os1, long long os2, const double* mat, int lane_axis, float lo, float hi,
                        ltu_stream_t s);
/* crop_orient: patches [n][h][w][d] (f32 and / or u8, either pair NULL, not both) cut from vol [H][W][D] at desc, a HOST int32 array
 * [n][6] = (h0, w0, d0, flip_h, flip_w, swap_hw): out[k][x][y][z] = vol[h0 + a][w0 + b][d0 + z] with (u, v) = swap_hw ? (y, x) :
 * (x, y), a = flip_h ? h-1-u : u, b = flip_w ? w-1-v : v - a signed permutation of the (h, w) plane, which expresses "flip along
 * axis 0, then rot90(k, axes (0, 1))" for every k.  n <= LTU_CROP_ORIENT_MAX (the descriptors travel as kernel arguments).
 * LTU_E_SHAPE: a crop outside the volume, swap_hw with h != w; LTU_E_ALIGN: d % 4 == 0 with out_img not 16-byte or out_lab not
 * 4-byte aligned. */
#define LTU_CROP_ORIENT_MAX 64
int ltu_crop_orient(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const int* desc, int n, int H, int W,
                    int D, int h, int w, int d, ltu_stream_t s);

/* ---- crop index: crop centres from the label on the device (csrc/crop_index.hip; no reference counterpart - monai keeps np.nonzero
 * index lists of the whole label on the host).  lab: u8, n_voxels contiguous voxels in raster order of [H][W][D], 16-byte aligned
 * (else LTU_E_ALIGN).  A voxel belongs to one of 9 bins: its value 0 .. 7, or bin 8 for every value >= 8.
 *   elems:  the uint32 elements of the index buffer of a label of n_voxels, 9 * (ceil(n_voxels / 4096) + 1); 0 for a size that
 *           build refuses.
 *   build:  index = per bin the exclusive prefix of the bin's voxels before every block of 4096 voxels, then its population;
 *           totals, device u64 [9] = the 9 populations (the caller reads them back once per scan).  Two launches, integer
 *           arithmetic, no atomics: two builds of one label are byte-identical.
 *   select: queries, device uint32 [n][2] = (mask, rank): bit b of mask (b = 0 .. 8; higher bits are ignored) puts bin b into
 *           the set - bit 0 is the background, bits 1 .. 8 together the foreground, one bit one class.  out, device int64 [n] =
 *           the linear voxel index of the rank-th member (from 0) of the set in ascending raster order, = np.nonzero of the
 *           set's predicate at [rank]; -1 when rank is not below the set's population.  One wave per query: a 64-way search
 *           over the blocks' prefixes (3 - 4 rounds of loads), then one block of the label is read.  n = 0 launches nothing.  lab and index are those
 *           of the build; a label changed since gives -1 or a member of another rank, never an access outside lab.
 *   Voxels at or beyond n_voxels are neither loaded nor counted.  Nothing is allocated, set or synchronised: capturable.
 *   Refused before any launch: n_voxels outside 1 .. 2^32 - 1 LTU_E_SHAPE; a NULL pointer, index_elems below elems(n_voxels),
 *   n < 0 LTU_E_ARG; lab not 16-byte, totals / out not 8-byte, index / queries not 4-byte aligned LTU_E_ALIGN. */
long long ltu_crop_index_elems(long long n_voxels);
int ltu_crop_index_build(const uint8_t* lab, long long n_voxels, uint32_t* index, long long index_elems, unsigned long long* totals,
                         ltu_stream_t s);
int ltu_crop_index_select(const uint8_t* lab, long long n_voxels, const uint32_t* index, long long index_elems,
                          const uint32_t* queries, long long* out, int n, ltu_stream_t s);

/* ---- intensity fingerprint: the value histogram of a stored scan (csrc/intensity.hip; nnU-Net's dataset fingerprint and
 * CTNormalization statistics, which it takes with np.percentile on the host).  img: n_voxels contiguous voxels of dtype LTU_U8 /
 * LTU_I16 / LTU_F32, lab: u8 of the same count or NULL, both 16-byte aligned.  A voxel is selected when lab is NULL or bit
 * min(lab[i], 8) of mask_bits is set (the bin sets of crop_index_select).
 *   hist:    every selected voxel gets a 16-bit key and adds 1 to hist[key], hist device uint32 [65536]; counts, device u64 [2], gets
 *            {voxels binned, voxels rejected} ADDED; the caller zeroes both.  mode (must match dtype, else LTU_E_ARG):
 *              LTU_HIST_U8       key = v
 *              LTU_HIST_I16      key = v + 32768
 *              LTU_HIST_F32_INT  an f32 holding an integer of -32768 .. 32767: key = (int)v + 32768; any other voxel is rejected
 *              LTU_HIST_F32_HI   key = the top 16 bits of the float's ordered key: the bit pattern with all bits flipped when the
 *                                sign is set and the sign bit set otherwise (-0.0 counts as +0.0), so keys order as the values do
 *              LTU_HIST_F32_LO   key = the low 16 bits of the ordered key of the voxels whose top 16 bits equal `prefix`; the others
 *                                are skipped (neither binned nor rejected)
 *            In the three F32 modes a non-finite voxel is rejected.  Integer adds only: two calls give the same bytes; n_voxels <=
 *            2^32 - 1, so no bin overflows.  One launch.
 *   moments: out, device double [2] = {sum (v - centre), sum (v - centre)^2} over the selected finite voxels of an f32 scan, in fp64:
 *            one pair per workgroup into parts (device double, parts_elems >= 2 * LTU_INTENSITY_MOMENT_PARTS), folded in index order by
 *            a second launch.  The workgroup count depends on n_voxels alone and there are no floating-point atomics: two calls
 *            give the same bits.
 *   Voxels at or beyond n_voxels are neither loaded nor counted.  Nothing is allocated, set or synchronised: capturable.
 *   Refused before any launch: n_voxels outside 1 .. 2^32 - 1 LTU_E_SHAPE; a NULL img / hist / counts / parts / out, a mode that
 *   does not match dtype, mask_bits outside 0 .. 0x1ff, prefix outside 0 .. 0xffff, a short parts, a non-finite centre LTU_E_ARG;
 *   img / lab not 16-byte, counts / parts / out not 8-byte, hist not 4-byte aligned LTU_E_ALIGN. */
enum { LTU_HIST_U8 = 0, LTU_HIST_I16 = 1, LTU_HIST_F32_INT = 2, LTU_HIST_F32_HI = 3, LTU_HIST_F32_LO = 4 };
#define LTU_INTENSITY_MOMENT_PARTS 512
int ltu_intensity_hist(const void* img, int dtype, const uint8_t* lab, long long n_voxels, int mask_bits, int mode, int prefix,
                       uint32_t* hist, unsigned long long* counts, ltu_stream_t s);
int ltu_intensity_moments(const float* img, const uint8_t* lab, long long n_voxels, int mask_bits, double centre, double* parts,
                          long long parts_elems, double* out, ltu_stream_t s);

/* ---- nonzero cropping and masked normalisation of a stored scan (csrc/nonzero.hip; nnU-Net's crop_to_nonzero and
 * ZScoreNormalization under the nonzero mask, which it runs on host copies).  With ltu_fill_holes between the first two:
 *   nonzero_mask:     mask[i] = (accumulate ? mask[i] : 0) | (fmaf(v, slope, inter) != 0) for the n_voxels voxels of img as stored
 *                     (dtype LTU_U8 / LTU_I16 / LTU_F32, aligned to its element; mask u8, any alignment): one call per channel ORs
 *                     the channels together.  A NaN counts as nonzero, -0.0 as zero.  16-byte loads and stores from the mask's
 *                     first 16-byte boundary on where the image is aligned there too, element by element otherwise and at both ends.
 *   mask_box:         mask u8 [B][H][W][D] (nonzero = set, any alignment) -> box int32 [B][6] = (h0, h1, w0, w1, d0, d1), the
 *                     inclusive bounds of the set voxels, and count (device u64 [B]) their number; an empty mask gives h0 = H,
 *                     h1 = -1, w0 = W, ... and count 0.  The call initialises both.  B <= 65535, H W D < 2^31.
 *   normalize_masked: img (dtype as above) and mask u8 are volumes [S2][S1][S0] (x fastest); out f32 [n2][n1][n0], dense, =
 *                     mask ? fmaf(v, alpha, beta) : 0 over the box that begins at (l0, l1, l2): the crop, the intensity map and
 *                     the zeroing outside the mask in one launch.  The box must lie inside the volume (LTU_E_SHAPE).
 *   Integer atomics only (min, max, add), no floating-point atomics: two calls give the same bytes.  Nothing is allocated or
 *   synchronised: capturable.  n_voxels / S0 S1 S2 outside 1 .. 2^32 - 1 LTU_E_SHAPE, another dtype LTU_E_DTYPE, a NULL pointer
 *   LTU_E_ARG, img not aligned to its element / box, out not 4-byte / count not 8-byte aligned LTU_E_ALIGN. */
int ltu_nonzero_mask(const void* img, int dtype, long long n_voxels, float slope, float inter, uint8_t* mask, int accumulate,
                     ltu_stream_t s);
int ltu_mask_box(const uint8_t* mask, int B, int H, int W, int D, int* box, unsigned long long* count, ltu_stream_t s);
int ltu_normalize_masked(const void* img, int dtype, const uint8_t* mask, int S0, int S1, int S2, int l0, int l1, int l2, int n0,
                         int n1, int n2, float alpha, float beta, float* out, ltu_stream_t s);

/* ---- augmentation of the NIfTI pipeline's patches (csrc/augment.hip; no reference counterpart: the monai driver crops, flips and
 * rot90s only).
 * sample_affine: patches [n][h][w][d] (f32 and / or u8, either pair NULL, not both) gathered from the scan [H][W][D] (the layout of
 *   SpacedScan.img / .lab) through one float64 3x4 pull matrix per patch, mats a HOST array [n][12]: patch voxel (x, y, z) reads the
 *   scan coordinate c = M (x, y, z, 1).  n <= LTU_SAMPLE_AFFINE_MAX (matrices, sigmas and seeds travel as kernel arguments).
 *   image: trilinear, out = sum of w * (tap inside the scan ? voxel : fill) over the 8 taps; a tap outside is never loaded; a matrix
 *          of integer coordinates reproduces the source voxels exactly (bit for bit, except that a source -0.0 comes out as +0.0).
 *   label: the voxel at the round-half-even coordinate, 0 when that voxel is outside the scan.
 *   The patch need not lie inside the scan.  Coordinates: an fp64 origin per workgroup tile (at most 256 voxel steps wide), split into
 *   integer and fraction, fp32 increments inside the tile (within ~2e-5 voxel of fp64), clamped to [-2, S + 1] before the float -> int
 *   conversion, which is therefore defined for every finite matrix.  When every matrix of the call has the form
 *   [[a, b, 0, .], [c, e, 0, .], [0, 0, g, .]] (rotation about D only) a z-decoupled kernel runs: in-plane taps once per D column.
 *   noise: noise_sigma (HOST float [n], NULL = none) and seeds (HOST uint64 [n], required with noise_sigma): with sigma_k > 0 the
 *          image store adds sigma_k * z, z ~ N(0, 1) from the counter-based generator defined in csrc/augment.hip's header comment,
 *          keyed by (seed_k, linear voxel index in the patch); sigma_k == 0 or NULL gives the bits of a call without noise.
 *   Refused before any launch: NULL mats, unpaired pointers, n outside 0 .. LTU_SAMPLE_AFFINE_MAX, noise_sigma without seeds, a
 *   non-finite matrix entry or fill, a negative or non-finite sigma LTU_E_ARG; a size < 1, a scan extent > 2^22, h > 65535, a patch of
 *   2^32 voxels or more LTU_E_SHAPE; d % 4 == 0 with out_img not 16-byte or out_lab not 4-byte aligned LTU_E_ALIGN.
 * sample_elastic: sample_affine with a uniform cubic B-spline free-form deformation applied in patch space ahead of M.  phi: a DEVICE
 *   array [n][3][gh][gw][gd] f32 (at most 6 KB per patch: too large for kernel arguments at n = 32), the control lattice of patch k:
 *   displacements in PATCH voxels along the patch axes H, W, D, 4 <= gh, gw, gd <= LTU_ELASTIC_MAX_GRID.  For the patch voxel
 *   p = (x, y, z) and, per axis a with patch coordinate t and patch extent n_a,
 *     s = t * (g_a - 3) / (n_a - 1)   (s = 0 when n_a == 1),   i = min(floor(s), g_a - 4),   f = s - i,
 *     B(f) = ((1-f)^3, 3f^3 - 6f^2 + 4, -3f^3 + 3f^2 + 3f + 1, f^3) / 6,
 *     u_c(p) = sum_{l,m,n in 0..3} B_l(fx) B_m(fy) B_n(fz) * phi[c][ix+l][iy+m][iz+n],   scan coordinate c = M (p + u(p), 1):
 *   C2-smooth, exactly 0 for a zero lattice (the output then has sample_affine's bits), and the crop, flip, rot90, rotation and zoom
 *   of M keep their meaning.  Each component of u is clamped to +-LTU_ELASTIC_MAX_DISP voxels (a NaN to -LTU_ELASTIC_MAX_DISP), so
 *   any lattice content gives defined coordinates; M[:, :3] u is added in fp32 inside sample_affine's coordinate bracket.  The
 *   lattice enters LDS once per workgroup, contracted with the tile's x weights; a lane contracts its y weights into the few
 *   lattice columns along z that its run of voxels needs, then 4 multiply-adds per voxel and component.  Image, label, fill, noise,
 *   mats, n as in sample_affine; no atomics, no workspace, no synchronisation: capturable.
 *   Refused before any launch: everything sample_affine refuses, with its codes; NULL phi LTU_E_ARG; a lattice extent outside
 *   4 .. LTU_ELASTIC_MAX_GRID LTU_E_SHAPE; phi not 4-byte aligned LTU_E_ALIGN.
 * sample_channels: either gather for a scan of K channels on one grid, img f32 [K][H][W][D], 1 <= K <= LTU_MAX_INPUT_CHANNELS, with
 *   the one label [H][W][D]: out_img [n][K][h][w][d], out_lab [n][h][w][d].  phi NULL runs sample_affine's kernels (gh, gw, gd are
 *   then ignored), otherwise sample_elastic's.  fill: HOST float [K]; noise_sigma: HOST float [n][K] or NULL; seeds: HOST uint64
 *   [n][K].  The coordinate, the spline displacement, the tap indices, weights and bounds tests and the label voxel are formed once
 *   per output voxel; every channel then sums its own 8 taps.  Channel c of out_img has the bits of the single-channel entry point
 *   called with img + c H W D, fill[c], noise_sigma[.][c] and seeds[.][c] and the same matrices (and lattice); out_lab has that
 *   call's bits.  Refused as the single-channel calls refuse, and NULL fill or a non-finite fill[c] LTU_E_ARG, K outside its range
 *   LTU_E_SHAPE.
 * sample_spline: sample_channels with a cubic B-spline image interpolation for the patches that ask for it (nnU-Net's spatial
 *   transform: scipy.ndimage.map_coordinates(order=3, mode='constant', cval=fill)).  coef: f32 [K][H][W][D] like img, the B-spline
 *   coefficients of each channel from ltu_spline_prefilter (mirror boundaries): the scan axes H and W filtered, D filtered for
 *   order_d == 3 and left as it is for order_d == 1 (any other order_d LTU_E_ARG).  fill, lo, hi: HOST float [K]; cubic: HOST bytes
 *   [n].  mats, phi, noise_sigma, seeds, the label and n per launch as in sample_channels; the coordinates are formed by the same
 *   code (fp64 origin per tile, fp32 bracket within ~2e-5 voxel of fp64, the deformation's M[:, :3] u added inside the bracket).
 *   cubic[k] == 0: patch k is gathered from img by the trilinear expressions; its image and label have the bits of sample_channels
 *     on the same arguments (the kernel variant is chosen from the whole call in the same way), so a patch of integer coordinates
 *     stays the source voxels.
 *   cubic[k] != 0, per channel c: where every component of the coordinate lies in [0, S - 1] of its axis, ends included, the voxel is
 *     clamp(sum of w * coef[c][taps], lo[c], hi[c]): per axis f = floor(coordinate), t = coordinate - f, an order-3 axis has the taps
 *     f-1 .. f+2 with the weights of resample_spline, axis D at order_d == 1 the taps f, f+1 with (1-t, t); tap indices are
 *     whole-sample mirrored (the zero-weight tap above the top edge is a valid address): 64 or 32 taps.  Everywhere else the voxel
 *     is fill[c], unclamped: there is no blending across the edge (what mode='constant' does at order 3).  lo / hi: the intensity
 *     window's clip (the spline rings past it), -inf / +inf for none.  The sum runs in fp32 in a fixed order: the taps along D as
 *     the inner fused multiply-add chain, then (wx wy) row added by one fused multiply-add, W inside H.  Tap indices, weights and
 *     the inside test are formed once per output voxel; channel c has the bits of a K == 1 call on img + c H W D, coef + c H W D
 *     and that channel's fill, lo, hi, sigma and seed.  Noise is added in the store, after the clamp; the label is sample_affine's.
 *   No atomics, no workspace, no synchronisation: capturable; two calls give the same bytes.
 *   Refused before any launch: everything sample_channels refuses, with its codes; NULL coef, cubic, lo or hi, lo[c] > hi[c] or a
 *   NaN bound LTU_E_ARG; a scan of 2^31 voxels or more per channel LTU_E_SHAPE (tap offsets are 32-bit, and spline_prefilter builds
 *   no larger volume).
 * sample_vote: the label half of sample_channels with the label taken by class vote instead of nearest (nnU-Net's spatial transform
 *   interpolates the label "one-hot, order 1"): lab u8 [H][W][D] -> out_lab u8 [n][h][w][d] through mats and, with phi != NULL, the
 *   lattice, both as in sample_channels (phi NULL: the affine kernels, gh, gw, gd ignored).  The coordinate, its fp32 bracket, the
 *   lower tap index i0 and the upper weights t are formed by the code of the trilinear image path (the z-decoupled and the general
 *   affine kernel, the elastic kernel; 4 voxels per lane when d % 4 == 0; 32- or 64-bit offsets), and the 8 taps are taken in its
 *   order r = 0 .. 7 (bit 2 of r: axis H, bit 1: W, bit 0: D).  The rule is resample_vote's:
 *     tap r has the weight w_r = (r & 4 ? t[0] : 1 - t[0]) * (r & 2 ? t[1] : 1 - t[1]) * (r & 1 ? t[2] : 1 - t[2]) in fp32, rounded
 *       before it is added, and the label l_r, the u8 voxel at the tap, 0 for a tap outside the scan (the nearest path's "0
 *       outside" and the image's fill; its load goes to the nearest voxel inside the scan and is discarded);
 *     the score of a value v is s_v = sum of w_r over the taps with l_r == v, in tap order, plain fp32 adds;
 *     out_lab = the smallest v of maximal score, compared exactly.  Every u8 value is a class.
 *   A matrix with integer entries (crop, flip, rot90, axis permutation) and no or an all-zero lattice gives weights 1 and 0: the
 *   label of sample_channels byte for byte.  The bracket is the trilinear one whatever interpolates the image of the same patches
 *   (sample_spline).  The coordinate lies within ~2e-5 voxel of fp64 (sample_affine), so a margin between the two best scores moves
 *   by at most 1.2e-4 against an fp64 evaluation of the rule.  The vote runs in registers (8 x 8 compares): no LDS beyond the elastic
 *   kernel's lattice, no atomics, no workspace, no synchronisation: capturable; two calls give the same bytes.
 *   Refused before any launch as sample_channels refuses a K == 1 label-only call; NULL lab or out_lab LTU_E_ARG.
 * gauss_blur3: out [n][H][W][D] f32 = mul_k * (3-D Gaussian blur of x [n][H][W][D]), out of place, one launch.  weights: HOST float
 *   [n][3][LTU_BLUR_MAX_RADIUS + 1], the half tables w[0 .. r] of the axes H, W, D (normalised so that w[0] + 2 sum w[t] = 1; entries
 *   beyond r are ignored); radii: HOST int [n][3], 0 = that axis untouched; mul: HOST float [n] or NULL (= 1), applied in the store.
 *   Boundaries reflect (d c b a | a b c d | d c b a), the semantics of scipy.ndimage.gaussian_filter(mode='reflect').  A patch with
 *   three radii 0 is copied as x * mul (mul == 1: bit-exact).  The three passes run inside a workgroup (pass D from memory into LDS,
 *   pass W LDS to LDS, pass H LDS to memory): no intermediate volume, no workspace.  n <= LTU_BLUR_MAX_N.
 *   Refused before any launch: NULL x / out / weights / radii, x == out, n outside 0 .. LTU_BLUR_MAX_N, a negative radius, a
 *   non-finite weight or mul LTU_E_ARG; a radius above LTU_BLUR_MAX_RADIUS or >= that axis's extent, a size < 1 LTU_E_SHAPE. */
#define LTU_SAMPLE_AFFINE_MAX 32
#define LTU_ELASTIC_MAX_GRID 8
#define LTU_ELASTIC_MAX_DISP 64
#define LTU_BLUR_MAX_N 16
#define LTU_BLUR_MAX_RADIUS 8
int ltu_sample_affine(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats,
                      const float* noise_sigma, const unsigned long long* seeds, int n, int H, int W, int D, int h, int w, int d,
                      float fill, ltu_stream_t s);
int ltu_sample_elastic(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats, const float* phi,
                       int gh, int gw, int gd, const float* noise_sigma, const unsigned long long* seeds, int n, int H, int W, int D,
                       int h, int w, int d, float fill, ltu_stream_t s);
int ltu_sample_channels(const float* img, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats, const float* phi,
                        int gh, int gw, int gd, const float* noise_sigma, const unsigned long long* seeds, const float* fill, int n,
                        int K, int H, int W, int D, int h, int w, int d, ltu_stream_t s);
int ltu_sample_spline(const float* img, const float* coef, const uint8_t* lab, float* out_img, uint8_t* out_lab, const double* mats,
                      const float* phi, int gh, int gw, int gd, const float* noise_sigma, const unsigned long long* seeds,
                      const float* fill, const float* lo, const float* hi, const unsigned char* cubic, int n, int K, int H, int W,
                      int D, int h, int w, int d, int order_d, ltu_stream_t s);
int ltu_sample_vote(const uint8_t* lab, uint8_t* out_lab, const double* mats, const float* phi, int gh, int gw, int gd, int n, int H,
                    int W, int D, int h, int w, int d, ltu_stream_t s);
int ltu_gauss_blur3(const float* x, float* out, const float* weights, const int* radii, const float* mul, int n, int H, int W, int D,
                    ltu_stream_t s);

/* ---- intensity augmentation of a batch of patches (csrc/intensity_aug.hip; nnU-Net's ContrastAugmentation, GammaTransform with
 * invert_image / retain_stats and SimulateLowResolution; no reference counterpart).  x: n volumes of `per` contiguous f32, one per
 * (patch, channel), 16-byte aligned at its base; a volume that does not begin on a 16-byte boundary is read and written with a scalar
 * head and tail around whole 16-byte quads.  1 <= per < 2^31.
 *   patch_stats:       stats, device double [n][4] = {min, max, sum x, sum x^2} of every volume, the sums in fp64.  One record of 4
 *                      doubles per workgroup into parts (device double, parts_elems >= ltu_patch_stats_parts_elems(n, per) = 4 n
 *                      blocks(per), blocks <= LTU_PATCH_STATS_MAX_PARTS), folded per volume in index order by a second launch.  The
 *                      workgroup count depends on per alone and there are no floating-point atomics: two calls give the same bytes.
 *                      n <= 65535.
 *   intensity_apply:   out[k] = op_k(x[k]) with ops, params HOST arrays [n] (n <= LTU_INTENSITY_AUG_MAX_N: they travel as kernel
 *                      arguments) and stats the patch_stats of x on the device:
 *                        LTU_IAUG_NONE       out = x, bit for bit (also any op with a parameter <= 0)
 *                        LTU_IAUG_CONTRAST   out = clip((x - m) f + m, min, max), m = (float)(sum / per), f = params[k]
 *                        LTU_IAUG_GAMMA      out = ((x - min) / max(r, 1e-7))^g r + min, r = max - min, g = params[k]
 *                        LTU_IAUG_GAMMA_INV  the same on u = -x, negated back: out = -(((u - min u) / max(r, 1e-7))^g r + min u)
 *                      t^g is exp2(g log2 t) on the hardware transcendentals, t = 0 gives 0; a gamma volume with max == min is copied.
 *                      out_stats non-NULL: the same pass writes the records of what it stored into parts (capacity as above) and a
 *                      second launch folds them into out_stats, device double [n][4]: the patch_stats of out without reading it
 *                      again.  out_stats NULL: one launch, parts is not touched and may be NULL.  out may be x.
 *   intensity_rescale: nnU-Net's retain_stats, in place: y[k] = (y[k] - mean y) * std x / max(std y, 1e-7) + mean x for the volumes
 *                      with on[k] != 0 (HOST bytes [n], n <= LTU_INTENSITY_AUG_MAX_N), means and population standard deviations
 *                      from stats_x and stats_y (device, patch_stats records) in fp64, the voxel in fp32 as one fused multiply-add.
 *                      The formula commutes with the inversion, so it serves both gammas.  A volume with on[k] == 0, or whose
 *                      stats_x has max == min, is not touched; no volume asking launches nothing.
 *   lowres_gather:     out [n][H][W][D] = trilinear_up(nearest_exact_down(x [n][H][W][D])), out of place, as one 8-tap gather; no
 *                      low-resolution volume exists.  tables: device int32 [n][3][H + W + D], per volume three planes over the
 *                      output indices of axis H, then W, then D: the source index of the lower tap, of the upper tap, and the bits
 *                      of the f32 weight l of the upper tap (built on the host in float64, lintransunet_amd/data.py::
 *                      lowres_tables).  A workgroup stages its tables in LDS, the indices clamped into their axis (any content gives
 *                      addresses inside the volume); a wave stores 64 consecutive floats.  out = sum of w v over the taps, w = (wx wy) wz with (1 - l | l) per axis, in the
 *                      fixed order x, y, z: the first product, then one fused multiply-add per tap, a tap of weight 0 left out, so
 *                      l = 0 on every axis returns the input's bits.  Extents <= LTU_LOWRES_MAX_EXTENT, n <= 65535.
 *   Nothing is allocated or synchronised and nothing is read back: capturable.
 *   Refused before any launch: a NULL pointer (parts only with out_stats), x == out in lowres_gather, n < 0 or above its limit in
 *   apply / rescale, an op outside the enum, a non-finite parameter, a parts_elems below what the launch writes LTU_E_ARG; per or an
 *   extent outside its range, n > 65535 LTU_E_SHAPE; x / out / y not 16-byte (lowres_gather: 4-byte),
 *   parts / stats not 8-byte, tables not 4-byte aligned LTU_E_ALIGN. */
enum { LTU_IAUG_NONE = 0, LTU_IAUG_CONTRAST = 1, LTU_IAUG_GAMMA = 2, LTU_IAUG_GAMMA_INV = 3 };
#define LTU_INTENSITY_AUG_MAX_N 64
#define LTU_PATCH_STATS_MAX_PARTS 256
#define LTU_LOWRES_MAX_EXTENT 1024
long long ltu_patch_stats_parts_elems(int n, long long per);
int ltu_patch_stats(const float* x, int n, long long per, double* parts, long long parts_elems, double* stats, ltu_stream_t s);
int ltu_intensity_apply(const float* x, float* out, const int* ops, const float* params, const double* stats, int n, long long per,
                        double* parts, long long parts_elems, double* out_stats, ltu_stream_t s);
int ltu_intensity_rescale(float* y, const unsigned char* on, const double* stats_x, const double* stats_y, int n, long long per,
                          ltu_stream_t s);
int ltu_lowres_gather(const float* x, float* out, const int* tables, int n, int H, int W, int D, ltu_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* LTU_HIP_H */
