/* re2e.h -- C ABI of libre2e_hip.so: MI355X (gfx950) kernels for the joint_train hot path of
 * bliunlpr/Robust_e2e_gan.
 *
 * The reference has NO native interface on this path (all arithmetic is stock PyTorch-0.4 ATen
 * ops plus warp-ctc, model/e2e_ctc.py:63), so each entry point cites the reference CALL SITE
 * whose ATen/warp-ctc op it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (fp32 unless named *_i32 / *_u8);
 *     the library never allocates, frees or retains device memory; scratch is caller-provided;
 *     `lens_host` arguments (where present) are HOST int32 arrays read during the call only;
 *   - asynchronous: work is enqueued on `stream`; no device synchronisation, no host read-back;
 *   - returns RE2E_OK (0) or a negative RE2E_E* code; never throws/exits; the message for the
 *     last failure on the calling thread is re2e_last_error();
 *   - reductions feeding parity-checked outputs are fixed-tree (bitwise reproducible run to run);
 *   - activations: NHWC for the conv stacks, (T,B,F) time-major inside the recurrent stacks,
 *     (B,T,F) batch-first at the module boundary, exactly as the reference lays them out.
 */
#ifndef RE2E_H
#define RE2E_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* re2e_stream_t; /* == hipStream_t */

#define RE2E_OK 0
#define RE2E_EINVAL (-1)
#define RE2E_EUNSUPPORTED (-2)
#define RE2E_EHIP (-3)

#define RE2E_ACT_NONE 0
#define RE2E_ACT_TANH 1
#define RE2E_ACT_RELU 2
#define RE2E_ACT_LRELU 3 /* slope 0.2 (model/gan_model.py:65) */
#define RE2E_ACT_SIGMOID 4
#define RE2E_ACT_SIGMOID_MASK_MUL 5 /* sigmoid -> length mask -> * mix (model/enhance_model.py:156-164) */

#define RE2E_LOSS_L2 0
#define RE2E_LOSS_L1 1
#define RE2E_LOSS_SMOOTH_L1 2
#define RE2E_STREAM_DEFAULT 0
#define RE2E_STREAM_FILLER 1 /* bulk work overlapped with resident recurrences: see re2e_stream_role */

#define RE2E_LOSS_BCE 3 /* nn.BCELoss on probabilities, logs clamped at -100 (model/gan_model.py:157-160, --no_lsgan) */

/* ABI version of this header: bumped whenever an entry point is added or a signature changes (positional arguments carry no
 * names across the boundary).  re2e_version() returns the value the library was built with; a binding written for another value
 * must refuse to call (robust_e2e_gan_amd/lib.py load()). */
#define RE2E_ABI_VERSION 339
int re2e_version(void);
const char* re2e_last_error(void);
/* 1 when device 0 is gfx950, 0 when another arch, <0 on HIP error. */
int re2e_device_ok(void);
/* Optional, no reference counterpart: prepares every persistent-recurrence kernel (code object loaded, dynamic-LDS limit raised) so
 * that the first sequence of a process is not a ~28 ms launch.  No stream, no device work, idempotent; needs a current HIP device. */
int re2e_warmup(void);
/* Scheduling hint, no reference counterpart (the reference runs one stream).  role = RE2E_STREAM_FILLER marks a stream whose
 * kernels run BESIDE the persistent recurrences of another stream (JointTrainer's side / weight-gradient streams,
 * joint_train.py step): the MFMA engine then launches 4-wave tiles there, which fit the registers a resident recurrence
 * leaves free on a CU; RE2E_STREAM_DEFAULT removes the mark.  Results do not depend on it.  At most 64 filler streams at a time. */
int re2e_stream_role(re2e_stream_t stream, int role);

/* ---- K3 dense GEMM (fp32 MFMA).  C[M,N] = act(op(A) op(B) + bias + bias2) + beta*C.
 * Row-major; transa=0: A stored [M,K], transa=1: A stored [K,M]; transb=0: B stored [K,N],
 * transb=1: B stored [N,K].
 *   (0,1)  x W^T     -- torch.nn.Linear forward  (e2e_encoder.py:145,173)
 *   (0,0)  dy W      -- input gradient
 *   (1,0)  dy^T x    -- weight gradient (split-K over rows, needs workspace)
 *   (1,1)  unsupported (RE2E_EUNSUPPORTED)
 * act=RE2E_ACT_SIGMOID_MASK_MUL writes mask_out=sigmoid(.)*[t<lens[b]] and C=mask_out*mul,
 * rows being (b,t) batch-first with T frames per utterance. */
size_t re2e_gemm_workspace_bytes(int transa, int transb, int M, int N, int K);
int re2e_gemm(int transa, int transb, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
              float* C, long ldc, const float* bias, const float* bias2, int act, float beta, const float* mul,
              float* mask_out, const int* lens_dev, int T, void* workspace, size_t workspace_bytes,
              re2e_stream_t stream);
/* Which kernel re2e_gemm (rowmap != 0: re2e_gemm_nt_rows / re2e_gemm_tn_rows) would run for this product, as one line of space-separated
 * key=value pairs in `out`; nothing is launched.  The same host function (csrc/igemm.hip plan_gemm) makes the choice for the entry points.
 * a16 / b16: A / B is 16-byte aligned with a leading dimension that is a multiple of 4; c16: so are C and the biases, and every operand spans
 * less than 2 GiB.  filler: the stream carries RE2E_STREAM_FILLER.
 *   route=skinny_wg vec=..                                          the K split inside the workgroup (M <= 32)
 *   route=pipeline vec=1 variant=.. tile=BMxBNxBK n_dp=.. g_sk=..   the LDS-DMA pipeline: n_dp whole tiles + g_sk workgroups of stream-K tail
 *   route=engine vec=.. tile=BMxBNxBK splits=.. m1=..               the tiled engine; rows [m1, M) run as a second launch of 64x64 tiles
 * followed by need=<workspace bytes the route uses> ws=<what re2e_gemm_workspace_bytes answers: the same on either stream role>.
 * cus > 0: plan for a chip of that many CUs (no device is touched); cus == 0: the current device's count. */
int re2e_gemm_plan(int transa, int transb, int M, int N, int K, int a16, int b16, int c16, int act, int rowmap, int filler, int cus, char* out,
                   size_t out_bytes);
/* x W^T over the VALID rows of a ragged time-major batch (the reference packs its sequences: e2e_encoder.py:129-131, enhance_model.py:120-123):
 *   C[map[r]][:] = act(A[map[r]][:] . B[N,K]^T + bias + bias2) + beta C[map[r]][:]   for r < Mv,
 * A (phys_rows x K, lda) and C (phys_rows x N, ldc) in the padded layout, rowmap[Mv] the physical rows with t < len_b.  Rows outside the map are
 * not touched (re2e_fill_rows).  Workspace as re2e_gemm(0, 1, Mv, N, K).  RE2E_EUNSUPPORTED when the shape is not one the LDS-DMA pipeline
 * takes (K, N, lda, ldb, ldc multiples of 4, 16-byte aligned operands, Mv >= 256): the caller runs re2e_gemm over all rows instead.
 * ident_rows (0 .. Mv, both entry points): the caller's promise that rowmap[r] == r for r < ident_rows (every utterance is at least that long:
 * min(len) * B rows of a time-major batch) -- tiles / k-tiles below it skip the table; 0 is always correct. */
int re2e_gemm_nt_rows(int Mv, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc, const float* bias,
                      const float* bias2, int act, float beta, const int* rowmap, int ident_rows, int phys_rows, void* workspace,
                      size_t workspace_bytes, re2e_stream_t stream);
/* The weight gradient over the same rows: C[M,N] = sum_{r < Kv} A[map[r]][:M]^T B[map[r]][:N] + beta C, A (dy) and B (x) padded
 * (phys_rows x ., lda / ldb).  Workspace as re2e_gemm(1, 0, M, N, Kv).  RE2E_EUNSUPPORTED unless both operands are 16-byte loadable. */
int re2e_gemm_tn_rows(int M, int N, int Kv, const float* A, long lda, const float* B, long ldb, float* C, long ldc, float beta,
                      const int* rowmap, int ident_rows, int phys_rows, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* C[rows[i]][0 .. N) = row_vec ? act(row_vec[0 .. N)) : value, i < nrows (N, ldc multiples of 4; row_vec 16-byte aligned, act one of
 * RE2E_ACT_NONE .. RE2E_ACT_SIGMOID).  With row_vec = the product's bias the padded rows hold what the reference's Linear + activation over
 * zero-padded frames leaves there: tanh(bias), e2e_encoder.py:145-147,173-176. */
int re2e_fill_rows(float* C, long ldc, int N, const int* rows, int nrows, float value, const float* row_vec, int act, re2e_stream_t stream);

/* ---- K5/K9 convolution as implicit GEMM over NHWC (nn.Conv2d: e2e_encoder.py:234-237,
 * gan_model.py:63-90).  `wg` is the gathered weight [Cout][KH][KW][C] from
 * re2e_conv_weight_gather.  Pixel (n,py,px) of the logical PHxPW grid reads
 * in[n][py*SY+kh*DY+OY0][px*SX+kw*DX+OX0][:] and is written at
 * out[n][py*osy+ooy][px*osx+oox][:] of an (NI,OHF,OWF,Cout) tensor -- forward: S=stride,D=1,
 * O0=-pad; stride-1 data gradient: S=1,D=-1,O0=+pad with transposed weights; stride-2 data
 * gradient: one call per output parity class. */
int re2e_conv_igemm(const float* in, int NI, int H, int W, int C, const float* wg, int Cout, int KH, int KW, int PH,
                    int PW, int SY, int SX, int DY, int DX, int OY0, int OX0, float* out, int OHF, int OWF, int osy,
                    int osx, int ooy, int oox, const float* bias, int act, float beta, re2e_stream_t stream);
/* The same product (no bias, no activation, dense output) followed by out = relu_out > 0 ? out : 0, `relu_out` an (NI,PH,PW,Cout)
 * tensor: the data gradient of a convolution whose INPUT was the ReLU output `relu_out` of the layer in front, taken through that
 * ReLU in the same launch (e2e_encoder.py:259-265: conv1_1 -> ReLU -> conv1_2, conv2_1 -> ReLU -> conv2_2), so the layer in front
 * needs no activation-backward pass.  3x3 / stride-1 geometries apply the mask in the kernel's epilogue, others in a second pass. */
int re2e_conv_igemm_masked(const float* in, int NI, int H, int W, int C, const float* wg, int Cout, int KH, int KW, int PH,
                           int PW, int SY, int SX, int DY, int DX, int OY0, int OX0, float* out, int OHF, int OWF, int osy,
                           int osx, int ooy, int oox, const float* relu_out, re2e_stream_t stream);
/* 3x3 / stride-1 / pad-1 convolution -> ReLU -> 2x2 / stride-2 ceil-mode max pool in ONE launch (e2e_encoder.py:260-262, 264-266): only the
 * pooled tensor (NI, ceil(H/2), ceil(W/2), Cout) and its index bytes (re2e_maxpool2_fwd's, with relu_in = 1) are written, the
 * full-resolution activation never reaches memory.  RE2E_EUNSUPPORTED unless C % 16 == 0, Cout % 64 == 0 and the tensors are 16-byte
 * aligned and < 2 GiB (the caller then runs re2e_conv_igemm + re2e_maxpool2_fwd). */
int re2e_conv3x3_relu_pool(const float* in, int NI, int H, int W, int C, const float* wg, int Cout, const float* bias, float* pooled,
                           unsigned char* idx_u8, re2e_stream_t stream);
/* 3x3 / stride-1 / pad-1 convolution as a fused Winograd F(2x2,3x3) on the fp32 matrix core (2.25x fewer matrix instructions than the
 * direct form; the transforms only add and halve, results agree with re2e_conv_igemm to a few ulp).  `w` is the layer's weight in
 * PyTorch's (Cout_f, Cin_f, 3, 3) layout -- no gathered copy is needed.  dgrad = 0: forward, in (NI,H,W,C = Cin_f) -> out
 * (NI,H,W,Cout = Cout_f), optional bias (Cout) and ReLU (relu = 1).  dgrad = 1: data gradient, in = dy (NI,H,W,C = Cout_f) -> out = dx
 * (NI,H,W,Cout = Cin_f).  `mask` (optional, shape of out): out = mask > 0 ? value : 0 (re2e_conv_igemm_masked's epilogue).
 * `pool_out` / `pool_idx` (optional, forward + relu): ONLY maxpool2(relu(conv)) (NI, ceil(H/2), ceil(W/2), Cout) and its index bytes are
 * written (re2e_conv3x3_relu_pool's contract), `out` may then be NULL.  The workspace holds the transformed weights (prepared by the
 * call itself).  RE2E_EUNSUPPORTED unless C % 8 == 0, Cout % 64 == 0, 16-byte aligned operands and tensors < 2 GiB: the caller then
 * uses re2e_conv_igemm / re2e_conv_igemm_masked / re2e_conv3x3_relu_pool (e2e_encoder.py:234-237,258-266 and their autograd gradients). */
size_t re2e_conv3x3_wino_workspace_bytes(int C, int Cout);
int re2e_conv3x3_wino(const float* in, int NI, int H, int W, int C, const float* w, int Cout, int dgrad, const float* bias, int relu,
                      const float* mask, float* out, float* pool_out, unsigned char* pool_idx, void* workspace, size_t workspace_bytes,
                      re2e_stream_t stream);

/* Weight gradient of the same layers the same way (csrc/wino_wgrad.hip): gw (Cout, C, 3, 3) (+)= G^T [ sum over 2x2 output tiles of
 * (B^T d B)[c] (x) (A dy A^T)[o] ] G -- transform + product in one kernel (split over patch ranges into `workspace` slabs), a second
 * one sums the slabs and applies G^T . G.  in (NI,H,W,C), dout (NI,H,W,Cout) NHWC, beta 0 / 1; C % 64 == 0, Cout % 32 == 0,
 * tensors < 2 GiB and 16-byte aligned, else RE2E_EUNSUPPORTED (the caller uses re2e_conv_wgrad). */
size_t re2e_conv3x3_wino_wgrad_workspace_bytes(int NI, int H, int W, int C, int Cout);
int re2e_conv3x3_wino_wgrad(const float* in, int NI, int H, int W, int C, const float* dout, int Cout, float* gw, float beta,
                            void* workspace, size_t workspace_bytes, re2e_stream_t stream);

/* The three over a RAGGED image batch (the VGG front end convolves zero-padded utterances and cuts each at its pooled length afterwards,
 * e2e_encoder.py:259-278: what it computes further beyond an utterance's end than the stack reaches is never read).  row_lim[n], int32 on
 * the device: output rows y >= row_lim[n] of image n (full-resolution rows, also with the fused pool) are neither computed nor written by
 * re2e_conv3x3_wino_rows -- patches of 8 / 16 rows that START there are skipped, so limits are multiples of 16; the weight gradient skips
 * the patches that start there (its dout is zero there: the caller's promise).  re2e_fill_image_rows writes `value` into rows
 * r >= ceil(lim[n] / div) of a (N, H, row_floats) tensor (div = 2: the pooled output of a layer whose limits count full-resolution rows);
 * max_tail_rows bounds H - lim / div over the batch.  The caller keeps the limits of consecutive layers consistent (VGG2L.conv_stack). */
int re2e_conv3x3_wino_rows(const float* in, int NI, int H, int W, int C, const float* w, int Cout, int dgrad, const float* bias, int relu,
                           const float* mask, float* out, float* pool_out, unsigned char* pool_idx, const int* row_lim, void* workspace,
                           size_t workspace_bytes, re2e_stream_t stream);
int re2e_conv3x3_wino_wgrad_rows(const float* in, int NI, int H, int W, int C, const float* dout, int Cout, float* gw, float beta,
                                 const int* row_lim, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
int re2e_fill_image_rows(float* t, int N, int H, long row_floats, const int* lim, int div, int max_tail_rows, float value, re2e_stream_t stream);

/* re2e_conv3x3_wino's forward over a PADDED image batch in which image n IS an image of valid_rows[n] rows (int32 on the device,
 * 1 <= valid_rows[n] <= H) sitting in a slot of H rows -- inference over utterances of different lengths (Encoder.encode_batch).  Input rows
 * >= valid_rows[n] are never read: they read as zero, as the rows beyond H do, whatever that memory holds (NaN, Inf, uninitialised).  Output
 * rows < valid_rows[n] -- with pool_out: pooled rows < ceil(valid_rows[n] / 2) and their index bytes, a window that straddles the end taking
 * its maximum over the rows inside (ceil mode) -- are bit for bit what re2e_conv3x3_wino writes for the cropped image alone.  Output rows
 * beyond are NOT written (unspecified): a consumer is given the same lengths and never reads them, so no fill is needed between layers.
 * Strides and allocation sizes stay those of H.  Forward only: dgrad = 1 or a mask is RE2E_EUNSUPPORTED (training keeps the reference's
 * arithmetic, which convolves the zero-padded batch WITHOUT masking between the layers: re2e_conv3x3_wino / _rows). */
int re2e_conv3x3_wino_valid(const float* in, int NI, int H, int W, int C, const float* w, int Cout, int dgrad, const float* bias, int relu,
                            const float* mask, float* out, float* pool_out, unsigned char* pool_idx, const int* valid_rows, void* workspace,
                            size_t workspace_bytes, re2e_stream_t stream);

/* 4x4 / stride-1 convolution as Winograd F(2x2,4x4) (csrc/wino44.hip; the discriminator's conv4, model/networks.py NLayerDiscriminator
 * `nn.Conv2d(ndf*4, ndf*8, kernel_size=4, stride=1, padding=1)`, and its data gradient): filter / input transform, ONE K-sliced launch
 * of the GEMM engine (25 positions), output transform.  in (NI,H,W,C) NHWC, out (NI, H+2*pad-3, W+2*pad-3, Cout), no bias / activation.
 * w is the layer's weight in PyTorch layout in BOTH directions: dgrad = 0: (Cout, C, 4, 4); dgrad = 1: `in` is dy, w is (C, Cout, 4, 4),
 * pad = 3 - the layer's padding, out = dx.  C % 16 == 0, Cout % 4 == 0, 16-byte aligned tensors, else RE2E_EUNSUPPORTED. */
size_t re2e_conv4x4_wino_workspace_bytes(int NI, int H, int W, int C, int Cout, int pad);
int re2e_conv4x4_wino(const float* in, int NI, int H, int W, int C, const float* w, int Cout, int pad, int dgrad, float* out,
                      void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* Its weight gradient the same way: gw (Cout, C, 4, 4) (+)= G^T [ sum_tiles (B^T d B) (x) (A dy A^T) ] G, the sum over tiles as a K-sliced
 * A^T B launch of the engine.  in (NI,H,W,C), dout (NI, H+2*pad-3, W+2*pad-3, Cout); beta 0 / 1; C % 4 == 0, Cout % 4 == 0. */
size_t re2e_conv4x4_wino_wgrad_workspace_bytes(int NI, int H, int W, int C, int Cout, int pad);
int re2e_conv4x4_wino_wgrad(const float* in, int NI, int H, int W, int C, const float* dout, int Cout, int pad, float* gw, float beta,
                            void* workspace, size_t workspace_bytes, re2e_stream_t stream);
size_t re2e_conv_wgrad_workspace_bytes(int NI, int PH, int PW, int C, int Cout, int KH, int KW);
/* dW[Cout][C][KH][KW] = beta*dW + sum_pix dout[pix][co] * in[n][py*SY+kh+OY0][px*SX+kw+OX0][ci] */
int re2e_conv_wgrad(const float* in, int NI, int H, int W, int C, const float* dout, int Cout, int KH, int KW, int PH,
                    int PW, int SY, int SX, int OY0, int OX0, float* dW, float beta, void* workspace,
                    size_t workspace_bytes, re2e_stream_t stream);
/* Which kernels serve one convolution of a layer (N,H,W,Cin) -> Cout channels, KH x KW, stride, pad: the host function the convolution entry
 * points and ops.py choose with (csrc/igemm.hip plan_conv / plan_conv_layer), as text "key=value ...".  dir: 0 forward, 1 data gradient, 2 weight
 * gradient; OH / OW: the output map (0: derived); act: the forward's activation; flags: RE2E_CONV_*.  family=wino3x3 (images=<per launch>),
 * wino4x4 or direct, ws=<workspace bytes of that family's entry point>; for direct wino_note=<a Winograd layer declined for an image of 2 GiB
 * or more> fused_pool=<re2e_conv3x3_relu_pool applies> and the plan of the entry point the layer calls:
 *   route=cin1_fwd taps= grid= | cout1_rows grid= lds= | cout1 L= kh= kw= ch= grid= lds= | halo patch= dir= relu= items= grid= lds= |
 *         pipeline variant= tile= n_dp= | engine tile= vec=          ... mask_pass=<the separate ReLU-mask pass follows> note=<the 2 GiB note>
 *   route=wgrad_cin1 slabs= | wgrad_cout1 slabs= | wgrad_engine tile= vec= splits=          ... wide_reduce= need=<bytes the call uses>
 * (a stride-2 data gradient into one channel: the plan of parity class (0,0) of its four calls).  cus > 0: plan for a chip of that many CUs (no
 * device is touched); cus == 0: the current device's count.  RE2E_EUNSUPPORTED: a data gradient ops.conv_dgrad does not cover. */
#define RE2E_CONV_BIAS 1
#define RE2E_CONV_POOL 2
#define RE2E_CONV_MASK 4
#define RE2E_CONV_W_STRIDED 8          /* the weight / input / output-gradient tensor is not contiguous */
#define RE2E_CONV_X_STRIDED 16
#define RE2E_CONV_DZ_STRIDED 32
#define RE2E_CONV_NO_WINOGRAD 64       /* the direct kernels whatever the layer (ops.py: RE2E_NO_WINOGRAD, experiments); also: the plan of the entry point itself */
#define RE2E_CONV_NO_WINO_WGRAD 128
#define RE2E_CONV_UNALIGNED 256        /* operands are not 16-byte aligned */
#define RE2E_CONV_FILLER 512           /* the call runs on a filler stream (re2e_stream_role) */
int re2e_conv_plan(int dir, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW, int act, int flags, int cus,
                   char* out, size_t out_bytes);
/* dst[r][a][b][c] <- W[Cout][Cin][KH][KW] at tap (kh0+a*kstep, kw0+b*kstep); transpose=0: r=co,c=ci; 1: r=ci,c=co */
/* Stride-2 data gradient in one launch (all four output parity classes): dx[N][H][Wd][Cin] from
 * dz[N][OH][OW][Cout] and the PyTorch-layout weight W[Cout][Cin][KH][KW] (KH, KW even).
 * wt_ws: caller scratch of Cin*KH*KW*Cout floats (the per-class gathered weights). */
int re2e_conv_dgrad_s2(const float* dz, int N, int OH, int OW, int Cout, const float* W, int Cin, int KH, int KW, int H,
                       int Wd, int pad, float* dx, float* wt_ws, re2e_stream_t stream);
int re2e_conv_weight_gather(const float* W, float* dst, int Cout, int Cin, int KH, int KW, int transpose, int TA,
                            int TB, int kh0, int kw0, int kstep, re2e_stream_t stream);

/* ---- elementwise / layout helpers ------------------------------------------------------- */
/* out[d1][d0][:] = in[d0][d1][:]  (batch-first <-> time-major) */
int re2e_transpose01(const float* in, float* out, int D0, int D1, int W, re2e_stream_t stream);
/* y = act(x): stand-alone tanh / relu / lrelu(0.2) / sigmoid (the U-Net blocks' nn.LeakyReLU / nn.ReLU / nn.Sigmoid
 * modules, enhance_model.py:277-291; everywhere else the activation is a GEMM / conv epilogue) */
int re2e_act_fwd(const float* x, float* y, long n, int act, re2e_stream_t stream);
/* dz = dy * act'(y), y = activation OUTPUT (tanh / relu / lrelu / sigmoid); dz may alias dy */
int re2e_act_bwd(const float* dy, const float* y, float* dz, long n, int act, re2e_stream_t stream);
/* out[n] = beta*out[n] + sum_m A[m*lda+n]; workspace >= re2e_colsum_workspace_bytes */
size_t re2e_colsum_workspace_bytes(int M, int N);
int re2e_colsum(const float* A, int M, int N, long lda, float* out, float beta, void* workspace,
                size_t workspace_bytes, re2e_stream_t stream);
/* Activation backward fused with the bias gradient: dz = dy * act'(y) (rows x N, contiguous) and
 * out[N] = beta*out + column sums of dz, in one pass over dy/y.  Workspace as re2e_colsum. */
int re2e_act_bwd_colsum(const float* dy, const float* y, float* dz, int M, int N, int act, float* out, float beta,
                        void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* enhancer mask epilogue backward: dlin = dout * mix * m * (1-m)   (enhance_model.py:156-164) */
int re2e_mask_mul_bwd(const float* dout, const float* mix, const float* mask, float* dlin, long n,
                      re2e_stream_t stream);
/* the same with dlin's rows padded to ldd >= N floats (zeros): (rows, N) operands, (rows, ldd) result */
int re2e_mask_mul_bwd_ld(const float* dout, const float* mix, const float* mask, float* dlin, long rows, int N, int ldd,
                         re2e_stream_t stream);
/* out = a*b elementwise (clean*cos target of the mask-L1 loss, enhance_model.py:170) */
int re2e_mul(const float* a, const float* b, float* out, long n, re2e_stream_t stream);
/* CMVN: out[r][j] = (x[r][j] + c0[j]) * c1[j]; c0==NULL gives x*c1 (its backward)  (feat_model.py:132-134) */
int re2e_affine_cols(const float* x, const float* c0, const float* c1, float* out, long rows, int N,
                     re2e_stream_t stream);
/* Dropout with a counter-based mask (F.dropout model/e2e_ctc.py:51 -- always on, its default training=True --,
 * nn.LSTM(dropout=) between the layers of BLSTM model/e2e_encoder.py:156-157, nn.Dropout of the U-Net blocks
 * model/enhance_model.py:298): y_i = x_i / (1-p) when word (i&3) of Philox4x32-10(counter {i>>2, i>>34, call, 0}, key = seed)
 * is >= floor(p * 2^32), else 0.  The backward pass is the same call on dy with the same (seed, call): no mask is stored. */
int re2e_dropout(const float* x, float* y, long n, float p, unsigned long long seed, unsigned call, re2e_stream_t stream);
/* y = a*x + b*y elementwise (gradient accumulation) */
int re2e_axpby(float a, const float* x, float b, float* y, long n, re2e_stream_t stream);
/* dst[i][:] = src[idx[i]][:] (rows of width W); scatter is the inverse (dst[idx[i]][:] = src[i][:]) */
int re2e_gather_rows(const float* src, const int* idx_dev, float* dst, int nrows, int W, re2e_stream_t stream);
int re2e_scatter_rows(const float* src, const int* idx_dev, float* dst, int nrows, int W, re2e_stream_t stream);
/* zero rows t >= lens[b] of a (B,T,W) tensor: out = in masked (mask_by_length, e2e_common.py:190-195) */
int re2e_mask_rows(const float* in, float* out, const int* lens_dev, int B, int T, int W, re2e_stream_t stream);

/* ---- K1 batch pack/pad (data/mix_data_loader.py:264-302): ragged rows -> zero padded (B,Tmax,F) */
int re2e_pack_pad(const float* src_flat, const int* offsets_dev, const int* lens_dev, int B, int Tmax, int F,
                  float* dst, re2e_stream_t stream);

/* K1, input side (data/kaldi_io.py:376-456 + data/mix_data_loader.py:198-237): decode a batch of raw Kaldi matrix records
 * and pad them.  blob = the records' payload bytes (device); record b starts at blob + rec_off[b] and is
 *   kind 0 ('FM'): rows*F row-major fp32 (16-byte aligned start), or
 *   kind 2 ('CM'): kaldi CompressedMatrix format 1 -- {min f32, range f32, rows i32, cols i32}, F x 4 uint16
 *                  percentiles, F x rows uint8 column-major.
 * dst (B,Tmax,F) = decoded values, zero padded.  dst_log (optional) = (10*log10(max(x,1e-7)) + cmvn[0]) * cmvn[1]
 * (cmvn (2,F), optional); when dst_log is given dst is clamped at 1e-7 too, as the reference's in-place clamp does. */
int re2e_kaldi_decode_pad(const unsigned char* blob, const long* rec_off_dev, const int* kind_dev, const int* lens_dev, int B,
                          int Tmax, int F, float* dst, float* dst_log, const float* cmvn, re2e_stream_t stream);

/* ---- K0 waveform front end (csrc/stft.hip; data/prepare_feats.py: MakeMixture + librosa.stft(n_fft=512, hop 256, scipy.signal.hamming)).
 * pcm: ONE device blob of 16-bit mono samples, used as they are (no scaling).  speech_off / speech_len / noise_off / noise_len / noise_start
 * (and snr_db): HOST arrays of B entries, in samples; they are checked here and travel as kernel arguments, so nothing has to stay alive
 * after the call.  Utterance b is s = pcm[speech_off[b] .. + L), 257 <= L = speech_len[b] < 2^31; its noise file n = pcm[noise_off[b] .. + N),
 * 1 <= N < 2^31, 0 <= noise_start[b] = s0 < N.  The mixture is m[i] = s[i] + g n[(s0 + i) mod N] (the reference tiles the file and slices).
 *
 * re2e_wav_mix_scale: scale_out[b] = g = sqrt(sum s^2 / (P 10^(snr_db[b]/10))), P = sum_{i<L} n[(s0 + i) mod N]^2; the sums are taken in
 * double in a fixed order (two runs agree bit for bit), the sums the reference meant (its own square int16 arrays and overflow).  P == 0:
 * g = 0 and *zero_count (device int, optional) is incremented -- the reference draws another noise file instead.  No host synchronisation.
 *
 * re2e_wav_stft: frames T_b = 1 + L / 256, reflect padding (librosa center=True), symmetric Hamming window 0.54 - 0.46 cos(2 pi n / 511),
 * X_t[k] = sum_n w[n] y[256 t - 256 + n] exp(-2 pi i k n / 512), k = 0 .. 256, of the clean signal (C) and of the mixture (M; scale[b] = g,
 * device).  Every output is optional, (B,Tmax,257) fp32, rows t >= T_b zero:
 *   clean = max(|C|, 1e-7), clean_log = (10 log10(clean) + cmvn[0]) * cmvn[1] (cmvn (2,257) optional), mix / mix_log likewise of M,
 *   cos = cos(angle C - angle M) = Re(C conj M) / (|C| |M|), clean_ang / mix_ang = atan2f(Im, Re); a zero magnitude has angle 0.
 * noise_off == NULL: the clean stream only (recognition); the four mixture outputs must be NULL.  Refused with a message, before anything
 * is launched: L < 257, Tmax < T_b, noise without scale, an index outside its range. */
int re2e_wav_mix_scale(const short* pcm, const long* speech_off, const long* speech_len, const long* noise_off, const long* noise_len,
                       const long* noise_start, const float* snr_db, int B, float* scale_out, int* zero_count, re2e_stream_t stream);
int re2e_wav_stft(const short* pcm, const long* speech_off, const long* speech_len, const long* noise_off, const long* noise_len,
                  const long* noise_start, const float* scale, int B, int Tmax, float* clean, float* clean_log, float* mix,
                  float* mix_log, float* cos_out, float* clean_ang, float* mix_ang, const float* cmvn, re2e_stream_t stream);

/* The way back (csrc/stft.hip), librosa.istft(hop_length=256, window=scipy.signal.hamming, center=True, length=L): no reference counterpart
 * on the device (the reference's enhance_out.py stops at the enhanced features).  mag, ang: (B,Tmax,257) fp32; out_off / out_len: HOST
 * arrays of B entries, in samples, checked here and passed as kernel arguments.  For utterance b, L = out_len[b], T = 1 + L / 256:
 *   X_t[k] = mag (cos ang + i sin ang), the imaginary parts of bins 0 and 256 ignored; x_t = irfft(X_t, 512) (with the 1/512);
 *   y[i] = (w[m + 256] x_{t-1}[m + 256] + w[m] x_t[m]) / (w[m + 256]^2 + w[m]^2), t = 1 + i / 256, m = i mod 256, for i < 256 (T - 1);
 *   y[i] = 0 for 256 (T - 1) <= i < L.  Rows t >= T of mag / ang are never read.
 * Every kept sample lies under exactly two frames, so the overlap-add is a gather: no atomics, two runs agree bit for bit.
 * The samples go to wav_f32[out_off[b] .. + L) (fp32) and / or pcm_out[out_off[b] .. + L) (int16: rintf, saturated to -32768 .. 32767;
 * *clip_count, device int, optional, is incremented by the number of saturated samples); both blobs hold out_samples samples, nothing
 * outside the B ranges is written.  Refused with a message, before anything is launched: L < 257, Tmax < T, mag or ang NULL, both outputs
 * NULL, a range outside 0 .. out_samples.
 *
 * re2e_wav_sdr_sums: sums[b] = {sum s^2, sum y^2, sum s y} over i < len[b] ((B,3) double, device), s = ref_pcm[ref_off[b] + i] (int16),
 * y = est[est_off[b] + i] (fp32); taken in double in a fixed order (two runs agree bit for bit).  The host derives
 * SNR = 10 log10(sum s^2 / sum (s - y)^2) and SI-SDR = 10 log10(|a s|^2 / |a s - y|^2), a = sum s y / sum s^2, from them. */
int re2e_wav_istft(const float* mag, const float* ang, const long* out_off, const long* out_len, int B, int Tmax, long out_samples,
                   float* wav_f32, short* pcm_out, int* clip_count, re2e_stream_t stream);
int re2e_wav_sdr_sums(const short* ref_pcm, const long* ref_off, const float* est, const long* est_off, const long* len, int B,
                      double* sums, re2e_stream_t stream);

/* Reverberation (csrc/reverb.hip; data/audioparse.py:254-303 Make_Reverberation = np.convolve(rir, x)[:len(x)], Make_Noisy_Wave): a batch of
 * n_jobs independent truncated FIR filters on the exact-fp32 matrix instruction.  pcm: the device blob of 16-bit samples (pcm_samples of
 * them), used as they are; rir: a device blob of rir_floats fp32 taps.  src_off / src_len / first / count / rir_off / rir_len / dst_off:
 * HOST arrays of n_jobs entries, checked here and passed as kernel arguments (jobs go 32 to a launch, as the utterances of
 * re2e_wav_stft), so nothing has to stay alive after the call.  Job q has the source x[j] = pcm[src_off[q] + j], 0 <= j < src_len[q] (zero
 * for j < 0), the filter h[k] = rir[rir_off[q] + k], 0 <= k < K = rir_len[q], and writes, for 0 <= i < count[q],
 *   y[i] = sum_{k < K} h[k] x[first[q] + i - k]
 * to wav_f32[dst_off[q] + i] (fp32) and / or pcm_out[dst_off[q] + i] (int16: rintf of the value wav_f32 holds, saturated to
 * -32768 .. 32767; *clip_count, device int, optional, is incremented by the number of saturated samples).  Both outputs hold out_samples
 * samples; nothing outside the n_jobs destination ranges is written.  The summation order of every output is fixed (ascending taps in
 * fp32, no atomics): two runs agree bit for bit.  pcm_out may be pcm itself (the reverberant signals land behind the uploaded samples of
 * one allocation).  Refused with a message, before anything is launched: first + count > src_len, K < 1 or K > RE2E_WAV_RIR_MAX, first < 0,
 * count < 1, a source range outside 0 .. pcm_samples, a filter range outside 0 .. rir_floats, a destination range outside 0 .. out_samples,
 * both outputs NULL, n_jobs < 1, and with pcm_out == pcm a destination range that overlaps any source range [src_off, src_off + src_len)
 * of the same call.
 * re2e_wav_reverb_geometry(which): 0 the K-tile (taps staged at a time), 1 the outputs per workgroup, 2 the jobs per launch,
 * 3 RE2E_WAV_RIR_MAX, 4 the contraction steps a K-tile is rounded up to; -1 otherwise.  The kernel takes other paths at their multiples (tests place their edges there).
 *
 * re2e_wav_stft_rev: re2e_wav_stft with a mixture that has its own speech stream, mix_off (HOST, B entries): the clean stream is still
 * s = pcm[speech_off[b] ..), the dry signal, and the mixture is m[i] = pcm[mix_off[b] + i] + g n[(s0 + i) mod N] (Make_Noisy_Wave changes the
 * noisy signal only; the L samples at mix_off[b] are the reverberant speech, the noise file is the reverberated noise).  M is the spectrum
 * of m itself; every output keeps its definition.  mix_off requires the noise arrays and scale; mix_off == NULL is re2e_wav_stft, the
 * same launches bit for bit.  re2e_wav_mix_scale called with mix_off as its speech_off gives the reference's g (SNR after reverberation). */
#define RE2E_WAV_RIR_MAX 32768        /* taps: 2.048 s at 16 kHz */
int re2e_wav_reverb(const short* pcm, long pcm_samples, const float* rir, long rir_floats, const long* src_off, const long* src_len,
                    const long* first, const long* count, const long* rir_off, const long* rir_len, const long* dst_off, int n_jobs,
                    long out_samples, float* wav_f32, short* pcm_out, int* clip_count, re2e_stream_t stream);
int re2e_wav_reverb_geometry(int which);
int re2e_wav_stft_rev(const short* pcm, const long* speech_off, const long* mix_off, const long* speech_len, const long* noise_off,
                      const long* noise_len, const long* noise_start, const float* scale, int B, int Tmax, float* clean, float* clean_log,
                      float* mix, float* mix_log, float* cos_out, float* clean_ang, float* mix_ang, const float* cmvn, re2e_stream_t stream);

/* Speed perturbation (csrc/resample.hip; no reference counterpart on the device: the reference's AudioParser promises "random tempo and gain
 * perturbations" and never implements them; this is Kaldi's 3-way `sox speed 0.9 / 1.0 / 1.1` as a rational resampler): a batch of n_jobs
 * independent polyphase resamplings, scipy.signal.resample_poly(x, up, down) with its defaults.  A speed factor s, given as a decimal string,
 * is the fraction p/q in lowest terms; up = q, down = p (0.9: 10/9, 1.1: 10/11).  For an L-sample source x the resampled signal has
 * L' = ceil(L up / down) samples:
 *   half = 10 max(up, down),  fc = 1 / max(up, down)
 *   g[i] = fc sinc(fc (i - half)) kaiser_{2 half + 1, beta = 5}(i),  0 <= i <= 2 half   (sinc(t) = sin(pi t) / (pi t), symmetric Kaiser window)
 *   h[i] = up g[i] / sum g
 *   y[m] = sum_j x[j] h[half + m down - j up],  over 0 <= j < L with 0 <= half + m down - j up <= 2 half   (x is zero outside 0 .. L - 1)
 * h is built inside the library on the host, in double (I0 by its power series), rounded ONCE to fp32 and kept per (up, down);
 * re2e_wav_resample_taps writes that fp32 table (2 half + 1 floats) to h_host and half to *half (either may be NULL, not both; no device).
 * pcm: the device blob of 16-bit samples (pcm_samples of them).  src_off / src_len / up / down / first / count / dst_off: HOST arrays of
 * n_jobs entries, checked here and passed as kernel arguments (jobs go 32 to a launch; jobs of different ratios may share one), so nothing
 * has to stay alive after the call.  Job q has the source x[j] = pcm[src_off[q] + j], 0 <= j < L = src_len[q], and writes y[first[q] + i],
 * 0 <= i < count[q], to wav_f32[dst_off[q] + i] (fp32) and / or pcm_out[dst_off[q] + i] (int16: rintf of the value wav_f32 holds, saturated
 * to -32768 .. 32767; *clip_count, device int, optional, is incremented by the number of saturated samples).  Both outputs hold out_samples
 * samples; nothing outside the n_jobs destination ranges is written.  Every output is accumulated in fp32 in ascending tap order (the
 * clip counter is the only atomic): two runs agree bit for bit.  pcm_out may be pcm itself (the perturbed speech lands behind the uploaded
 * samples of one allocation).  A speed of exactly 1 is not a job: the samples pass through untouched, and up == down is refused.
 * Refused with a message, before anything is launched: up < 1 or down < 1, up == down, gcd(up, down) != 1,
 * max(up, down) > RE2E_WAV_RESAMPLE_MAX_RATE, first < 0, count < 1, first + count > L', a source range outside 0 .. pcm_samples, a
 * destination range outside 0 .. out_samples, both outputs NULL, n_jobs < 1, and with pcm_out == pcm a destination range that overlaps any
 * source range [src_off, src_off + src_len) of the same call.  The first job of a ratio in a process allocates its table on the device
 * and copies it there with a blocking copy (some 5 KB at most, kept for the life of the process).
 * re2e_wav_resample_geometry(which): 0 the outputs per workgroup, 1 the jobs per launch, 2 RE2E_WAV_RESAMPLE_MAX_RATE; -1 otherwise. */
#define RE2E_WAV_RESAMPLE_MAX_RATE 64        /* every speed on a 1/64 grid, 0.95 and 1.05 among them; its table is 1281 floats */
int re2e_wav_resample(const short* pcm, long pcm_samples, const long* src_off, const long* src_len, const int* up, const int* down,
                      const long* first, const long* count, const long* dst_off, int n_jobs, long out_samples, float* wav_f32,
                      short* pcm_out, int* clip_count, re2e_stream_t stream);
int re2e_wav_resample_geometry(int which);
int re2e_wav_resample_taps(int up, int down, float* h_host, int* half);

/* SpecAugment on the normalised filterbank features (csrc/specaug.hip; Park et al. 2019 in ESPnet's form: `time_warp`, `freq_mask`,
 * `time_mask`; no reference counterpart): y = masks(warp(x)), and dx = J^T dy for the same plan.
 * x, y: (R, Tp, F) fp32, rows zero-padded behind their valid frames.  plan: DEVICE int32, R rows of P = 3 + 2 nF + 2 nT entries
 *   [T_r, c, w, f0_1, f_1, .., f0_nF, f_nF, t0_1, t_1, .., t0_nT, t_nT]
 * Time warp, per row over its own T_r valid frames: c == 0 is no warp.  Otherwise, for a warp window W, W <= c < T_r - W and
 * c - W + 1 <= w <= c + W: the frames [0, c) are resized along time to w frames and the frames [c, T_r) to T_r - w frames, each segment as
 * torch.nn.functional.interpolate(mode='bicubic', align_corners=False) resizes it (the feature axis keeps its size).  For a segment of
 * n_in -> n_out frames and its output frame t:
 *   N = (2 t + 1) n_in - n_out,  D = 2 n_out,  i0 = floor(N / D),  tau = (N - i0 D) / D      (integers; ONE fp32 division)
 *   y[t] = sum_{k = 0..3} wk(tau) x[clamp(i0 - 1 + k, 0, n_in - 1)]
 *   w0 = ((A (tau + 1) - 5 A)(tau + 1) + 8 A)(tau + 1) - 4 A,  w1 = ((A + 2) tau - (A + 3)) tau^2 + 1,  w2 = w1(1 - tau),  w3 = w0(1 - tau),
 *   A = -0.75 (the cubic convolution).  A segment with n_in == n_out, and a row with c == 0, is copied bit for bit.
 * Masks, after the warp: the cells with f0_k <= f < f0_k + f_k and t < T_r, and the cells with t0_k <= t < t0_k + t_k, become 0.0 (the
 * feature mean after CMVN).  Widths of zero and overlapping masks are legal.  Frames t >= T_r pass through unchanged, forward and backward.
 * Backward: a gather -- source frame s sums wk dy[t] over the contiguous run of output frames t whose clamped taps hit it, found by inverting
 * i0(t) in integers, in ascending (t, k); the first and last frame of a segment collect the clamped taps; masked cells contribute nothing.
 * No atomics: two runs agree bit for bit.
 * The plan arrives from the host without a round trip, so the kernels clamp every value where they read it: T_r into 0 .. Tp; c <= 0 or
 * T_r < 2 is no warp, otherwise c into 1 .. T_r - 1 and w into 1 .. T_r - 1; f0 into 0 .. F and f into 0 .. F - f0; t0 into 0 .. T_r and t
 * into 0 .. T_r - t0.  No plan reads or writes outside row r.  (A plan outside the contract can make one source frame of the backward sum
 * many output frames: correct, and slower.)
 * One launch each, whatever R, nF and nT.  Rows go as float4 where F % 4 == 0 and both tensors are 16-byte aligned, scalar otherwise.
 * Refused with a message, before anything is launched and with nothing written: x == y (dy == dx), a null operand, R < 1, Tp < 1, F < 1,
 * nF or nT outside 0 .. RE2E_SPECAUG_MAX_MASKS.
 * re2e_spec_augment_geometry(which): 0 the output frames per forward workgroup, 1 the source frames per backward workgroup,
 * 2 RE2E_SPECAUG_MAX_MASKS, 3 the output frames a backward workgroup stages; -1 otherwise. */
#define RE2E_SPECAUG_MAX_MASKS 8
int re2e_spec_augment_fwd(const float* x, const int* plan, int R, int Tp, int F, int nF, int nT, float* y, re2e_stream_t stream);
int re2e_spec_augment_bwd(const float* dy, const int* plan, int R, int Tp, int F, int nF, int nT, float* dx, re2e_stream_t stream);
int re2e_spec_augment_geometry(int which);

/* ---- K2 fused fbank (model/feat_model.py:118-135): y = log(max((x^2) W, 1e-7)); optional
 * second output y_norm = (y + cmvn[0]) * cmvn[1]; optional third output pw_out = (x^2) W itself, which re2e_fbank_bwd takes
 * back.  W is given banded: for filter j the taps band_w[j*maxw + i] apply to bins band_off[j]+i, i<band_len[j]. */
int re2e_fbank_fwd(const float* x, long rows, int F, int NF, const int* band_off, const int* band_len,
                   const float* band_w, int maxw, float* y_raw, float* y_norm, const float* cmvn, float* pw_out,
                   re2e_stream_t stream);
/* dx = 2x * sum_j W[f][j] * (dy_raw + dy_norm*cmvn1)[j] / pw[j], zero where pw<=1e-7 (clamp).  pw (rows,NF) = the forward's pw_out.
 * Here the matrix is banded the other way round (the filters covering a bin are a contiguous run as well): bin f is covered by
 * filters bin_off[f] + i, i < bin_len[f], with weights bin_w[f*maxc + i]. */
int re2e_fbank_bwd(const float* x, long rows, int F, int NF, const int* bin_off, const int* bin_len, const float* bin_w, int maxc,
                   const float* pw, const float* dy_raw, const float* dy_norm, const float* cmvn, float* dx, re2e_stream_t stream);
/* Dense trainable filterbank (fbank_opti_type 'train', feat_model.py:105-109): x^2 W and its gradients are re2e_gemm calls;
 * these are the element-wise tail of feat_model.py:127-134: y = log(max(z,1e-7)) [-> (y + cmvn[0]) * cmvn[1]] and
 * dz = dy * cmvn[1] / z, zero where the clamp fired (cmvn (2,N) optional). */
int re2e_logclamp_fwd(const float* z, const float* cmvn, long rows, int N, float* y, re2e_stream_t stream);
int re2e_logclamp_bwd(const float* z, const float* cmvn, long rows, int N, const float* dy, float* dz, re2e_stream_t stream);
/* per-column sum and sum of squares over valid frames of y (B,T,NF): feat_model.py:62-80 on device */
int re2e_cmvn_stats(const float* y, const int* lens_dev, int B, int T, int NF, float* sum_out, float* sumsq_out,
                    re2e_stream_t stream);

/* ---- K10 reductions ---------------------------------------------------------------------- */
/* out[0] = mean_i loss(a_i - b_i) (b==NULL => constant `target`): F.mse_loss / l1 / smooth_l1
 * (joint_train.py:162-167) and GANLoss MSE-to-constant (gan_model.py:162-171) */
size_t re2e_reduce_workspace_bytes(long n);
int re2e_loss_fwd(const float* a, const float* b, float target, long n, int kind, float* out, void* workspace,
                  size_t workspace_bytes, re2e_stream_t stream);
/* da = beta*da + (*gscale_dev) * scale * dloss/da_i / n */
int re2e_loss_bwd(const float* a, const float* b, float target, long n, int kind, const float* gscale_dev,
                  float scale, float* da, float beta, re2e_stream_t stream);
/* out[0] = sum x_i^2 */
int re2e_sumsq(const float* x, long n, float* out, void* workspace, size_t workspace_bytes, re2e_stream_t stream);

/* ---- K5 pooling + VGG output packing (e2e_encoder.py:259-278) ------------------------------ */
/* 2x2/2 ceil-mode max pool over NHWC; idx_u8 stores the argmax (0..3) for the backward.  relu_in != 0: `in` is the output of the
 * ReLU of the convolution in front (e2e_encoder.py:260-261,264-265) and the pool's backward is to return the gradient of that
 * ReLU's INPUT: windows whose maximum is <= 0 get index 4, so re2e_maxpool2_bwd leaves their gradient out -- d(relu) costs no pass */
int re2e_maxpool2_fwd(const float* in, int NI, int H, int W, int C, float* out, unsigned char* idx_u8, int relu_in,
                      re2e_stream_t stream);
int re2e_maxpool2_bwd(const float* dout, const unsigned char* idx_u8, int NI, int H, int W, int C, float* din,
                      re2e_stream_t stream);
/* NHWC (NI,T,Fq,C) -> utterances [n_off, n_off+NI) of a time-major (T,NI_total,C*Fq) tensor with rows
 * t>=lens[n] zeroed (cut + re-pad); the offset lets two separately computed branches share one tensor */
int re2e_vgg_pack_fwd(const float* in, const int* lens_dev, int NI, int T, int Fq, int C, float* out, int NI_total,
                      int n_off, re2e_stream_t stream);
int re2e_vgg_pack_bwd(const float* dout, const int* lens_dev, int NI, int T, int Fq, int C, float* din, int NI_total,
                      int n_off, re2e_stream_t stream);

/* ---- K9 BatchNorm2d (train mode) + LeakyReLU(slope) over NHWC rows [P][C]: slope 0.2 = the discriminator's
 * BatchNorm2d + LeakyReLU(0.2) pairs (gan_model.py:76-88), slope 1.0 = plain BatchNorm2d (U-Net blocks,
 * enhance_model.py:281-296) */
size_t re2e_bn_workspace_bytes(long P, int C);
int re2e_bn_lrelu_fwd(const float* x, long P, int C, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float momentum, float eps, int train, float slope, float* y, float* save_mean,
                      float* save_invstd, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* dy is the gradient w.r.t. the LeakyReLU output; dgamma/dbeta may be NULL (frozen D) */
int re2e_bn_lrelu_bwd(const float* dy, const float* x, long P, int C, const float* gamma, const float* beta,
                      const float* save_mean, const float* save_invstd, float slope, float* dx, float* dgamma, float* dbeta,
                      float gbeta, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* Synchronised BatchNorm for data-parallel runs that shard ONE global batch (the same kernels, cut where the caller all-reduces):
 * re2e_bn_sync_partial: out[C] = sum over the LOCAL rows of (x - mean) (mean may be NULL) or of its square; the caller all-reduces and
 * divides by the global row count; re2e_bn_sync_finalize: global mean / biased variance -> save_mean, save_invstd, running statistics;
 * re2e_bn_apply: y = lrelu((x - mean) invstd gamma + beta); re2e_bn_sync_bwd_partial: out[2C] = local sum dz | sum dz*xhat;
 * re2e_bn_sync_bwd_apply: dx from the all-reduced sums scaled by P / Ptotal (the kernel divides by its own row count). */
int re2e_bn_sync_partial(const float* x, long P, int C, const float* mean, int square, float* out, void* workspace, size_t workspace_bytes,
                         re2e_stream_t stream);
int re2e_bn_sync_finalize(const float* mean, const float* var, long Ptotal, int C, float momentum, float eps, float* running_mean,
                          float* running_var, float* save_mean, float* save_invstd, re2e_stream_t stream);
int re2e_bn_apply(const float* x, long P, int C, const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                  float slope, float* y, re2e_stream_t stream);
int re2e_bn_sync_bwd_partial(const float* dy, const float* x, long P, int C, const float* gamma, const float* beta, const float* save_mean,
                             const float* save_invstd, float slope, float* out, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
int re2e_bn_sync_bwd_apply(const float* dy, const float* x, long P, int C, const float* gamma, const float* beta, const float* save_mean,
                           const float* save_invstd, float slope, const float* sums, float* dx, re2e_stream_t stream);

/* ---- K4 bidirectional LSTM recurrence, packed-sequence semantics (nn.LSTM call sites
 * e2e_encoder.py:128-132,168-170).  Time-major.  xg_f/xg_r [T*B,4H] hold x W_ih^T + b_ih + b_hh
 * (gate order i,f,g,o) on entry and the ACTIVATED gates on exit (saved for the backward);
 * ybuf/cbuf are [(T+2)*B, 2H] with block 0 and block T+1 zero: y[t] lives in block t+1. */
size_t re2e_lstm_workspace_bytes(int B, int H);
/* Number of sequences (since the library was loaded) that a persistent recurrence kernel gave up on because a peer
 * workgroup never published its step (bounded spin; the outputs of such a sequence are NaN).  0 in a healthy run.
 * Synchronises the device; -1 if the counter cannot be read. */
int re2e_lstm_abort_count(void);
/* Test hooks (tests/test_dp_gpu.py, tests/test_trainers_gpu.py; no reference counterpart -- the reference is single-device and has no
 * persistent kernels).  re2e_debug_force_abort(n): the next n persistent FORWARD sequences behave as given up (outputs NaN, the
 * counter above rises) without running -- what JointTrainer.fit's recovery path is tested with.  re2e_debug_occupy: a kernel of
 * `workgroups` x 256 threads that holds `lds_bytes` of LDS each and spins for `usec` microseconds on `stream`: what a ring
 * all-reduce waiting for a slow peer looks like to the workgroup scheduler. */
/* Both hooks answer RE2E_EUNSUPPORTED unless RE2E_DEBUG_HOOKS=1 is in the environment (the tests set it). */
int re2e_debug_force_abort(int n);
int re2e_debug_occupy(int workgroups, int lds_bytes, int usec, re2e_stream_t stream);
/* The trainer's step gate (joint_train.py:188-193 plus the give-up protocol above), one 1-thread kernel and no host round trip.
 * base_dev: device int, the give-up count the trainer has acknowledged (ack != 0: set it to the current count first).  delta = count - *base_dev.
 * hold_next (optional): 1.0 when delta == 0, NaN otherwise -- the next step multiplies its losses by it, so a step enqueued before the host
 * repeated an aborted one applies nothing, on any replica.  stats_main (optional; the [norm, coef, finite | norm, 1, finite] of
 * re2e_clip_coef): finite := 0 and norm := NaN when delta != 0 or *extra_sumsq (optional: another optimizer's gradient sum of squares) is not
 * finite.  stats_d (optional): finite := 0 when delta != 0 or *d_requires (optional: another gate's finite flag) is 0.  delta_out (optional):
 * delta as a float, for the step's meters. */
int re2e_step_gate(int* base_dev, int ack, const float* extra_sumsq, float* stats_main, float* stats_d, const float* d_requires, float* hold_next,
                   float* delta_out, re2e_stream_t stream);
int re2e_lstm_seq_fwd(float* xg_f, float* xg_r, const float* whh_f, const float* whh_r, float* ybuf, float* cbuf,
                      const int* lens_dev, int T, int B, int H, void* workspace, size_t workspace_bytes,
                      re2e_stream_t stream);
/* g_f/g_r: activated gates in, d(pre-activation gates) out (in place).  dy [T*B,2H].
 * whh_*: W_hh [4H,H] as stored by nn.LSTM.  dc_state [B,2H] scratch (zeroed by the call).
 * dbias (optional, [2][4H]): the column sums of d(gates) over all T*B rows, forward direction then reverse = the gradient of
 * bias_ih and of bias_hh (autograd of nn.LSTM, e2e_encoder.py:128-132) -- accumulated beside the recurrence where the kernel
 * form allows it, so that the caller needs no pass of its own over the (T*B, 4H) tensors.
 * workspace (re2e_lstm_workspace_bytes) holds the MFMA-fragment-ordered weight / state copies. */
int re2e_lstm_seq_bwd(float* g_f, float* g_r, const float* whh_f, const float* whh_r, const float* dy,
                      const float* ybuf, const float* cbuf, float* dc_state, const int* lens_dev, int T, int B, int H,
                      float* dbias, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* Which kernel re2e_lstm_seq_fwd (backward == 0) / re2e_lstm_seq_bwd would run for this shape, as one line of space-separated key=value
 * pairs in `out`; nothing is launched.  The same host functions make the choice for the two entry points above.
 *   family=fwd2_persist|fwd2_step tiles=.. nj=..   family=fwd_persist waves=.. qn=..   family=fwd_step waves=..
 *   family=bwd3 un=.. tpw=..   family=bwd_persist tpw=.. uw=..   family=bwd_step jt=..
 * followed by grid=XxYxZ lds=<dynamic LDS bytes>.  cus > 0: plan for a chip of that many CUs (no device is touched); cus == 0: the
 * current device's count.  The recurrent weights are assumed 16-byte aligned.  RE2E_EUNSUPPORTED when no kernel is built for H. */
int re2e_lstm_plan(int T, int B, int H, int backward, int cus, char* out, size_t out_bytes);

/* ---- K8 LSTMCell pointwise (decoder, e2e_decoder.py:131), embedding, cross-entropy -------- */
/* gates [B,4H] pre-activation in -> activated out; c_prev [B,H] -> c_out, h_out */
int re2e_lstm_cell_fwd(float* gates, const float* c_prev, float* c_out, float* h_out, int B, int H,
                       re2e_stream_t stream);
/* gates: activated in -> dgates (pre-activation) out; dh (+ dh2, optional: the decoder adds the direct gradient dZ[i] to
 * the carried one), dc_in -> dc_prev_out */
int re2e_lstm_cell_bwd(float* gates, const float* c_prev, const float* c_cur, const float* dh, const float* dh2,
                       const float* dc_in, float* dc_prev_out, int B, int H, re2e_stream_t stream);
/* One decoder step's LSTMCell (e2e_decoder.py:131) in one launch: gates [B,4D] (embedding half of the input projection + both
 * biases on entry) += ctx [B,E] W_ih[:, Dd:]^T + z_prev [B,D] W_hh^T (w_ctx = &W_ih[0][Dd], row pitch ldw), then the cell:
 * activated gates out, c_prev -> c_out, h_out.  E, D, ldw multiples of 4. */
int re2e_dec_gates_cell_fwd(const float* cx, const float* z_prev, const float* w_ctx, long ldw, const float* w_hh, float* gates,
                            const float* c_prev, float* c_out, float* h_out, int B, int E, int D, re2e_stream_t stream);
/* ---- upper layers of a multi-layer decoder (dlayers > 1, e2e_decoder.py:121-152; csrc/decstack.hip) ----
 * Layer l >= 1 is an LSTMCell (D -> D, torch gate order) on the state of the layer below at the same token and on its own previous state.  fp32;
 * D % 4 == 0 and D <= 1024, any row count: RE2E_EUNSUPPORTED beyond.  No kernel waits on another workgroup.
 * re2e_dec_upper_step: one token for n rows in one launch: gates = b_ih + b_hh + x W_ih^T + z_prev W_hh^T, then the cell -> z_out, c_out (n,D) and,
 * if gates != NULL, the activated gates (n,4D).  A row's result does not depend on the other rows of the launch (bit for bit).
 * re2e_dec_gates_cell_fwd was not reused for it: it needs the gates pre-filled with the biases by another launch. */
int re2e_dec_upper_step(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* z_prev,
                        const float* c_prev, float* gates, float* z_out, float* c_out, int n, int D, re2e_stream_t stream);
/* Teacher-forced recurrence of one upper layer over L1 tokens, one launch per token: gates (L1,B,4D) holds z_below W_ih^T + b_ih + b_hh on entry
 * (ONE re2e_gemm over all L1 * B rows) and the activated gates on return; per token gates[i] += z[i] W_hh^T, then the cell -> z[i+1], c[i+1].
 * z, c (L1+1,B,D) with block 0 = the initial state (zeros). */
int re2e_dec_upper_seq_fwd(float* gates, const float* w_hh, float* z, float* c, int L1, int B, int D, re2e_stream_t stream);
/* Its backward, tokens L1-1 .. 0, one launch per token: the cell backward (dh = carried + dZ[i], dc) -> dG[i] (pre-activation d gates, a buffer
 * of its own: every workgroup reads gates[i]), dc_prev, and the carried dz_prev = dG[i] W_hh in the same launch.  w_hhT (D,4D) = W_hh transposed
 * (re2e_transpose01).  The products over the whole sequence (d z_below = dG W_ih, d W_ih = dG^T z_below, d W_hh = dG^T z[0:L1], d b = column sums
 * of dG) are the caller's, on re2e_gemm / re2e_colsum.  Workspace: re2e_dec_upper_bwd_workspace_bytes(B, D). */
size_t re2e_dec_upper_bwd_workspace_bytes(int B, int D);
int re2e_dec_upper_seq_bwd(const float* gates, const float* c, const float* dZ, const float* w_hhT, float* dG, int L1, int B, int D, void* workspace,
                           size_t workspace_bytes, re2e_stream_t stream);
/* The whole teacher-forced decoder loop (e2e_decoder.py:113-152: AttLoc.forward e2e_attention.py:259-299 + LSTMCell per output token) as ONE
 * persistent launch (csrc/decloop.hip).  re2e_dec_loop_workspace_bytes returns 0 when the shape is outside the resident form's limits
 * (forward: B <= 32, D <= 320, E <= 512, D, E, A multiples of 4, C <= 12, T <= 2048; backward: E <= 512 and a multiple of 16, C <= 16,
 * 2*Fh+1 <= 255; both: every workgroup resident, one per CU -- csrc/decloop.hip dec_plan / dec_bwd_plan are the authority) or RE2E_DEC_PERSIST=0: the caller then runs the launch-per-step
 * sequence re2e_attloc_fwd + re2e_dec_gates_cell_fwd.  pre (B,T,A) = mlp_enc(enc), enc (B,T,E) masked encoder states, w_decT (D,A) = mlp_dec^T,
 * w_att (A,C), w_conv (C,2Fh+1), w_ctx = &W_ih[0][Dd] with row pitch ldw, w_hh (4D,D).  gates (L1,B,4D): embedding half of the input projection
 * + both biases on entry, activated gates on exit; z, c (L1+1,B,D) with block 0 = the initial state; w (L1,B,T), cx (L1,B,E),
 * conv (L1,B,T,C), dpj (L1,B,A): what re2e_attloc_bwd reads.  A give-up (bounded spin) is counted by re2e_lstm_abort_count. */
size_t re2e_dec_loop_workspace_bytes(int L1, int B, int T, int E, int D, int A, int C, int Fh);
int re2e_dec_loop_fwd(const float* pre, const float* enc, const int* hlens_dev, const float* w_decT, const float* w_att, const float* w_conv,
                      const float* gvec, const float* gvec_b, const float* w_ctx, long ldw, const float* w_hh, float* gates, float* z, float* c,
                      float* w, float* cx, float* conv, float* dpj, int L1, int B, int T, int E, int D, int A, int C, int Fh,
                      void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* The loop's backward as ONE persistent launch: the reverse of the above, token L1-1 .. 0.  On entry gates holds the activated gates saved by
 * the forward; on exit d(gates) (what the weight-gradient products read).  d_cx_all (L1,B,E), de_all (L1,B,T), ddp (L1,B,A) = d dec_proj and
 * d_pre (B,T,A; may be NULL) are written; the d conv rows of every token stay in the workspace for re2e_dec_loop_dwconv, which adds d W_conv to
 * partials (B, partial_floats) at float offset wconv_offset of each row (layout of re2e_attloc_partial_floats) -- a separate call so that it can
 * run on a weight-gradient stream.  dZ (L1,B,D): gradient of the decoder states.  0 bytes = shape outside the resident form (also
 * RE2E_DEC_PERSIST=0, or =2: forward only): the caller runs re2e_lstm_cell_bwd + re2e_gemm_skinny2 + re2e_attloc_bwd per token. */
size_t re2e_dec_loop_bwd_workspace_bytes(int L1, int B, int T, int E, int D, int A, int C, int Fh);
int re2e_dec_loop_bwd(const float* pre, const float* enc, const float* cx, const float* z, const float* c, const float* w, const float* conv,
                      const float* dpj, const float* dZ, const int* hlens_dev, const float* w_ctx, long ldw, const float* w_hh, const float* mlp_dec,
                      const float* w_att, const float* w_conv, const float* gvec, float* gates, float* d_cx_all, float* de_all, float* ddp,
                      float* d_pre, int L1, int B, int T, int E, int D, int A, int C, int Fh, void* workspace, size_t workspace_bytes,
                      re2e_stream_t stream);
int re2e_dec_loop_dwconv(const float* w, const int* hlens_dev, const void* workspace, size_t workspace_bytes, float* partials, int partial_floats,
                         int wconv_offset, int L1, int B, int T, int E, int D, int A, int C, int Fh, re2e_stream_t stream);
/* Two skinny products that share A (M <= 32 rows) in one launch: C1 = A[M,K] B1[K,N1], C2 = A B2[K,N2] (B row-major (K,N));
 * the decoder's backward step: d ctx = dgates W_ih[:, Dd:], d z = dgates W_hh. */
int re2e_gemm_skinny2(int M, int K, const float* A, long lda, const float* B1, long ldb1, int N1, float* C1, long ldc1,
                      const float* B2, long ldb2, int N2, float* C2, long ldc2, re2e_stream_t stream);
int re2e_embedding_fwd(const float* table, const int* ids_dev, int n, int D, float* out, long ldo,
                       re2e_stream_t stream);
/* dtable[v][:] = beta*dtable + sum_{i: ids[i]==v} dout[i][:] in index order (deterministic) */
int re2e_embedding_bwd(const float* dout, long ldo, const int* ids_dev, int n, int D, int V, float* dtable,
                       float beta, re2e_stream_t stream);
/* Row-wise arg-max (lowest index on ties) of x[R][V] (leading dimension ldx): the token that scheduled
 * sampling and Decoder.calculate_all_attentions feed back (e2e_decoder.py:123-127, :408-412 `y_i.topk(1)`). */
int re2e_argmax_rows(const float* x, int R, int V, long ldx, int* out_ids, re2e_stream_t stream);
/* out[R][V] = log_softmax(x[R][V]) row-wise (F.log_softmax of Decoder.recognize_beam e2e_decoder.py:263 and
 * CTC.log_softmax e2e_ctc.py:68-75) */
int re2e_log_softmax_rows(const float* x, int R, int V, long ldx, float* out, re2e_stream_t stream);

/* F.cross_entropy(ignore_index=-1, mean) * scale and th_accuracy (e2e_decoder.py:155-161).
 * out[0]=loss, out[1]=#correct, out[2]=#valid ; lse [R] saved for the backward */
int re2e_ce_fwd(const float* logits, const int* targets_dev, int R, int V, float scale, float* out, float* lse,
                void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* dlogits = (*gscale_dev)*scale/#valid * (softmax - onehot) on valid rows, 0 on ignored rows */
int re2e_ce_bwd(const float* logits, const int* targets_dev, const float* lse, const float* fwd_out, int R, int V,
                float scale, const float* gscale_dev, float* dlogits, re2e_stream_t stream);
/* Label-smoothing regulariser of the decoder loss (e2e_decoder.py:162-166):
 * out[0] = -(1/nutt) * sum over ALL R rows and V labels of log_softmax(logits)[r][v] * dist[v]; workspace R floats.
 * bwd: dlogits[r][v] = gscale[0] * (softmax[r][v] * sum(dist) - dist[v]) / nutt. */
int re2e_lsm_fwd(const float* logits, const float* dist, int R, int V, int nutt, float* out, void* workspace,
                 size_t workspace_bytes, re2e_stream_t stream);
int re2e_lsm_bwd(const float* logits, const float* dist, int R, int V, int nutt, const float* gscale, float* dlogits,
                 re2e_stream_t stream);

/* ---- K6 CTC (warp-ctc call site e2e_ctc.py:63): logits (T,B,V) raw activations, blank 0,
 * loss = sum_b nll_b / B.  labels_dev: flat int32; label_off_dev/label_len_dev per utterance. */
size_t re2e_ctc_workspace_bytes(int T, int B, int Lmax);
int re2e_ctc_fwd(const float* logits, int T, int B, int V, const int* hlens_dev, const int* labels_dev,
                 const int* label_off_dev, const int* label_len_dev, int Lmax, float* loss_out, float* nll_per_utt,
                 void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* dlogits = (*gscale_dev)/B * (softmax - occupancy) for t<hlens[b], 0 otherwise; uses the workspace of fwd.  dlogits has rows of
 * ldd >= V floats (columns V .. ldd-1 are written as zeros): an odd vocabulary (V = 4233) padded to a multiple of 16 lets the two
 * products of the projection's backward run on the engine's 16-byte-load path. */
int re2e_ctc_bwd(const float* logits, int T, int B, int V, const int* hlens_dev, const int* labels_dev,
                 const int* label_off_dev, const int* label_len_dev, int Lmax, const float* nll_per_utt,
                 const float* gscale_dev, float* dlogits, int ldd, const void* workspace, re2e_stream_t stream);

/* ---- N3 CTC prefix scores for joint CTC/attention beam search (CTCPrefixScore model/e2e_ctc.py:78-155 as called per
 * hypothesis at model/e2e_decoder.py:231-263), all `nh` live hypotheses of one output position in one launch.
 * lpz (T,V) CTC log posteriors; att_lsm (nh,V) attention log-probabilities; r_prev (nh,T,2) forward variables of each
 * hypothesis; last_label / out_len (labels without <sos>) / prev_score (nh).  Per hypothesis: cand_out (ctc_beam) = its top
 * labels in torch.topk order, ctc_score_out = log prefix probabilities, local_out = att_weight*att + ctc_weight*(ctc - prev), r_new
 * (nh,ctc_beam,T,2) = the candidates' new forward variables.  ctc_beam <= 64 (RE2E_EUNSUPPORTED beyond). */
int re2e_ctc_prefix_score(const float* lpz, int T, int V, const float* att_lsm, int nh, const float* r_prev, const int* last_label_dev,
                          const int* out_len_dev, const float* prev_score_dev, int ctc_beam, float att_weight, float ctc_weight, int blank,
                          int eos, int* cand_out, float* local_out, float* ctc_score_out, float* r_new, re2e_stream_t stream);
/* re2e_ctc_prefix_score for the hypotheses of SEVERAL utterances in one launch (beam search over a batch): lpz (U,Tmax,V), zero-padded;
 * tlen_dev (U) = frames T_u of each utterance; utt_dev (nh) = the utterance of each hypothesis.  r_prev (nh,Tmax,2) and r_new
 * (nh,ctc_beam,Tmax,2) are pitched Tmax.  Every loop bound, the clamp of the start frame and the <eos> score (rsum[T_u - 1]) use
 * T_u = tlen[utt[h]]: over t < T_u a row's outputs are bit for bit those of re2e_ctc_prefix_score on its utterance alone; state entries
 * at t >= T_u are written as -1e10.  ctc_beam <= 64 and (V + 3 Tmax) floats of LDS (RE2E_EUNSUPPORTED beyond). */
int re2e_ctc_prefix_score_batch(const float* lpz, int U, int Tmax, int V, const int* tlen_dev, const int* utt_dev, const float* att_lsm, int nh,
                                const float* r_prev, const int* last_label_dev, const int* out_len_dev, const float* prev_score_dev, int ctc_beam,
                                float att_weight, float ctc_weight, int blank, int eos, int* cand_out, float* local_out, float* ctc_score_out,
                                float* r_new, re2e_stream_t stream);
/* The same scores for a caller-given candidate list cand_dev (nh, ncand) -- ctc_weight == 1.0 scores all V labels in the order of their
 * attention scores (a device-side stable sort): one thread per candidate, outputs (nh, ncand) in the list's order, r_new (nh*ncand, T, 2). */
int re2e_ctc_prefix_score_cands(const float* lpz, int T, int V, const float* att_lsm, int nh, const float* r_prev, const int* last_label_dev,
                                const int* out_len_dev, const float* prev_score_dev, const int* cand_dev, int ncand, float att_weight,
                                float ctc_weight, int blank, int eos, float* local_out, float* ctc_score_out, float* r_new, re2e_stream_t stream);

/* ---- K7 location-aware attention step (model/e2e_attention.py:258-297) -------------------- */
/* per utterance b: w = softmax_t(2*(gvec . tanh(W_att conv(att_prev) + pre[b,t] + W_dec z[b]) + gb)),
 * c[b] = sum_t w[t]*enc[b,t].  att_prev==NULL => uniform 1/hlen over valid frames.
 * w_decT is mlp_dec.weight TRANSPOSED, (dunits, adim).  conv_out (B,T,chans) and dp_out (B,adim) are the
 * location-conv output and W_dec z, saved for the backward; e_scratch (B,T) is scratch.
 * The work is cut into 32-frame workgroups (grid = ceil(T/32) x B) + a per-utterance softmax/context pass. */
int re2e_attloc_fwd(const float* pre, const float* enc, const float* z, const float* att_prev, const int* hlens_dev,
                    const float* w_decT, const float* w_att, const float* w_conv, const float* gvec, const float* gvec_b,
                    int B, int T, int eprojs, int dunits, int adim, int chans, int filts, float* w_out, float* c_out,
                    long ldc_out, float* conv_out, float* dp_out, float* e_scratch, re2e_stream_t stream);
/* The same step for `nh` rows (the live hypotheses of a beam search over several utterances) that share U utterances: pre (U,T,adim) and
 * enc (U,T,eprojs) are read through utt_dev (nh) = the utterance of each row, once per utterance held and not once per row.  hlens_dev (U)
 * = the frames T_u of each utterance: a row HAS only those -- the softmax and the context run over t < T_u, att_prev reads as 0 beyond, w_out
 * and conv_out at t >= T_u are written as 0 -- so a row gets bit for bit what re2e_attloc_fwd gives for T = T_u on its utterance alone.
 * z, att_prev, w_out, c_out, conv_out, dp_out, e_scratch are per row, (nh, .) with frame pitch T.  Same kernels as re2e_attloc_fwd. */
int re2e_attloc_fwd_rows(const float* pre, const float* enc, int U, const int* hlens_dev, const int* utt_dev, const float* z, const float* att_prev,
                         const float* w_decT, const float* w_att, const float* w_conv, const float* gvec, const float* gvec_b, int nh, int T,
                         int eprojs, int dunits, int adim, int chans, int filts, float* w_out, float* c_out, long ldc_out, float* conv_out,
                         float* dp_out, float* e_scratch, re2e_stream_t stream);
size_t re2e_attloc_partial_floats(int adim, int chans, int filts);
size_t re2e_attloc_workspace_bytes(int B, int T, int adim, int chans);
/* backward of one step: writes de_out (B,T) = d(energy) of this step (kept by the caller for re2e_attloc_dpre),
 * d_att_prev (may be NULL for step 0) and d_decproj [B,adim] (for the mlp_dec GEMMs), accumulates the location-filter
 * part of the per-utterance weight-grad partials (+=), which are laid out
 * [B][gvec(adim) | gvec_b(1) | w_att(adim*chans) | w_conv(chans*(2*filts+1))].  cx_in = the forward context
 * c (B,eprojs), conv_in / dp_in = the tensors saved by re2e_attloc_fwd.  Neither the encoder-state gradient nor
 * d_pre / dgvec / dW_att are produced here: call re2e_attloc_denc and re2e_attloc_dpre once after the loop. */
int re2e_attloc_bwd(const float* pre, const float* enc, const float* att_prev, const float* w_cur, const int* hlens_dev,
                    const float* w_att, const float* w_conv, const float* gvec, const float* conv_in, const float* dp_in,
                    const float* cx_in, const float* dc, long ld_dc, const float* dw_in, int B, int T, int eprojs, int adim,
                    int chans, int filts, float* de_out, float* d_att_prev, float* d_decproj, float* partials,
                    void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* after the loop: d_pre (B,T,adim) = sum over the L1 steps of d(pre-activation) (overwritten), and the gvec / gvec_b /
 * w_att parts of the partials (+=), recomputed from pre, conv_all (L1,B,T,chans), dp_all (L1,B,adim) (the tensors saved
 * by re2e_attloc_fwd, stacked over the steps) and de_all (L1,B,T) (written by re2e_attloc_bwd). */
int re2e_attloc_dpre(const float* pre, const float* conv_all, const float* dp_all, const float* de_all, const float* w_att,
                     const float* gvec, int L1, int B, int T, int adim, int chans, int filts, float* d_pre, float* partials,
                     void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* d_enc[b,t,:] = beta*d_enc + sum_i w_all[i,b,t] * dc_all[i,b,:]  (w_all (L1,B,T), dc_all (L1,B,eprojs)) */
int re2e_attloc_denc(const float* w_all, const float* dc_all, int L1, int B, int T, int eprojs, float* d_enc, float beta,
                     re2e_stream_t stream);

/* ---- K7b content-based and coverage attention steps (AttDot, AttAdd, AttCov, AttCovLoc; csrc/attstep.hip) ----
 * The step of K7 with another energy term, selected by `kind`:
 *   RE2E_ATT_ADD       e = gvec . tanh(pre[b,t] + W_dec z[b]) + gb
 *   RE2E_ATT_COVERAGE  e = gvec . tanh(wvec_w cov[b,t] + wvec_b + pre[b,t] + W_dec z[b]) + gb
 *   RE2E_ATT_DOT       e = sum_a pre[b,t,a] q[b,a], q = tanh(W_dec z[b] + dec_b); pre is tanh(mlp_enc(enc)), made by the caller
 * w = softmax over all T frames of 2 e, c = sum_t w[t] enc[b,t].  Coverage state: cov_0[b,t] = 1/hlen_b for t < hlen_b, else 0 (cov_in == NULL
 * stands for it); the step writes cov_out = cov_in + w (B,T), padded frames included.  RE2E_ATT_COVERAGE_LOCATION is K7 with cov as att_prev:
 * re2e_attloc_fwd / _bwd / _dpre plus re2e_attstep_cov_add; these entry points refuse it, and RE2E_ATT_LOCATION, with a message.
 * Parameters a kind does not have are NULL (dot: dec_b only; add: gvec, gvec_b; coverage: wvec_w (adim), wvec_b (adim), gvec, gvec_b).
 * dp_out (B,adim) = W_dec z (dot: q), saved for the backward; e_scratch (B,T) is scratch; cov_out is written for coverage only.
 * Limits: adim <= 320, dunits <= 1024, eprojs % 4 == 0, T <= ~39000 (LDS of the softmax pass): RE2E_EUNSUPPORTED / RE2E_EINVAL otherwise. */
#define RE2E_ATT_LOCATION 0
#define RE2E_ATT_DOT 1
#define RE2E_ATT_ADD 2
#define RE2E_ATT_COVERAGE 3
#define RE2E_ATT_COVERAGE_LOCATION 4
int re2e_attstep_fwd(int kind, const float* pre, const float* enc, const float* z, const float* cov_in, const int* hlens_dev,
                     const float* w_decT, const float* dec_b, const float* wvec_w, const float* wvec_b, const float* gvec,
                     const float* gvec_b, int B, int T, int eprojs, int dunits, int adim, float* w_out, float* c_out, long ldc_out,
                     float* cov_out, float* dp_out, float* e_scratch, re2e_stream_t stream);
/* The same step for `nh` rows over U utterances, as re2e_attloc_fwd_rows: pre (U,T,adim) and enc (U,T,eprojs) are read through utt_dev (nh),
 * a row has only the T_u = hlens_dev[utt] frames of its utterance (cov_in reads as cov_0 of T_u frames when NULL; w_out and cov_out at
 * t >= T_u are written as 0), and gets bit for bit what re2e_attstep_fwd gives for T = T_u on its utterance alone. */
int re2e_attstep_fwd_rows(int kind, const float* pre, const float* enc, int U, const int* hlens_dev, const int* utt_dev, const float* z,
                          const float* cov_in, const float* w_decT, const float* dec_b, const float* wvec_w, const float* wvec_b,
                          const float* gvec, const float* gvec_b, int nh, int T, int eprojs, int dunits, int adim, float* w_out,
                          float* c_out, long ldc_out, float* cov_out, float* dp_out, float* e_scratch, re2e_stream_t stream);
/* cov_out (rows,T) = cov_in + w; cov_in == NULL: cov_0 of each row's utterance (utt_dev == NULL: row b is utterance b; hlens_dev (U)). */
int re2e_attstep_cov_add(const float* cov_in, const float* w, const int* hlens_dev, const int* utt_dev, int U, int rows, int T,
                         float* cov_out, re2e_stream_t stream);
/* floats of a row of the weight-gradient partials (B, .): [gvec(adim) | gvec_b(1) | wvec_w(adim) | wvec_b(adim)] (add: the first two; dot: 0) */
size_t re2e_attstep_partial_floats(int kind, int adim);
size_t re2e_attstep_workspace_bytes(int kind, int B, int T, int adim);
/* backward of one step: de_out (B,T) = d(energy) (kept for re2e_attstep_dpre), d_cov (B,T) = the gradient at cov_in (coverage; may be NULL),
 * d_decproj (B,adim) = the gradient at W_dec z (dot: at W_dec z + dec_b).  cov_in / dp_in / cx_in: what the forward read and saved; dw_in (B,T)
 * or NULL: the gradient arriving at this step's w from outside its own softmax / context path. */
int re2e_attstep_bwd(int kind, const float* pre, const float* enc, const float* cov_in, const float* w_cur, const int* hlens_dev,
                     const float* wvec_w, const float* wvec_b, const float* gvec, const float* dp_in, const float* cx_in, const float* dc,
                     long ld_dc, const float* dw_in, int B, int T, int eprojs, int adim, float* de_out, float* d_cov, float* d_decproj,
                     void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* after the loop: d_pre (B,T,adim) = sum over the L1 steps (overwritten; dot: the gradient at tanh(mlp_enc(enc))) and the partials (+=).
 * cov_all (L1,B,T): cov_out of every step, stacked (step s reads cov_all[s-1], step 0 cov_0); dp_all (L1,B,adim), de_all (L1,B,T).
 * d_enc: re2e_attloc_denc. */
int re2e_attstep_dpre(int kind, const float* pre, const float* cov_all, const int* hlens_dev, const float* dp_all, const float* de_all,
                      const float* wvec_w, const float* wvec_b, const float* gvec, int L1, int B, int T, int adim, float* d_pre,
                      float* partials, void* workspace, size_t workspace_bytes, re2e_stream_t stream);

/* ---- RNNLM shallow fusion at decode time (model/lm.py:125-146, e2e_decoder.py:270-285; csrc/rnnlm.hip) ----
 * Few-row kernels: n = the live hypotheses of a beam-search position, 1 <= n <= 64; any widths (the loads are as wide as the
 * operands' alignment allows).  None needs a workspace.
 * nn.LSTMCell for n rows in one launch: gates = W_ih x + b_ih + W_hh h_prev + b_hh (w_ih (4H, I), w_hh (4H, H), gate order i, f, g, o),
 * c_out = f * c_prev + i * g, h_out = o * tanh(c_out), all (n, H).  ids_dev == NULL: x is (n, I) with leading dimension ldx;
 * otherwise x is an embedding table (n_embed, I; ldx) and row r reads x[ids_dev[r]] (an id outside the table gives a NaN row).
 * h_prev / c_prev may be NULL (zeros).  h_out / c_out must not alias h_prev or x; c_out may alias c_prev. */
int re2e_lm_lstm_cell(const float* x, long ldx, const int* ids_dev, int n_embed, int I, const float* w_ih, const float* w_hh,
                      const float* b_ih, const float* b_hh, const float* h_prev, const float* c_prev, int n, int H, float* h_out,
                      float* c_out, re2e_stream_t stream);
/* re2e_lm_lstm_cell followed by zoneout in evaluation mode (the FS-RNN LM's cells, fsrnn.py:15-32): h_out = keep_h h' + (1 - keep_h) h_prev,
 * c_out = keep_c c' + (1 - keep_c) c_prev.  x == NULL (then ids_dev is NULL too; ldx, I and w_ih are ignored): a cell without input, only
 * b_ih contributes.  Every output element is written. */
int re2e_lm_lstm_cell_zo(const float* x, long ldx, const int* ids_dev, int n_embed, int I, const float* w_ih, const float* w_hh,
                         const float* b_ih, const float* b_hh, const float* h_prev, const float* c_prev, int n, int H, float keep_h,
                         float keep_c, float* h_out, float* c_out, re2e_stream_t stream);
/* logits (n, V) = h (n, H) w (V, H)^T + b */
int re2e_lm_output(const float* h, const float* w, const float* b, int n, int V, int H, float* logits, re2e_stream_t stream);
/* lsm (n, V) = log_softmax(logits) row-wise and, with att / comb (both or neither), comb = att + lm_weight * lsm in the same pass
 * (product and sum rounded separately: e2e_decoder.py:272). */
int re2e_lm_log_softmax_combine(const float* logits, int n, int V, const float* att, float lm_weight, float* lsm, float* comb,
                                re2e_stream_t stream);
/* local[k][j] += lm_weight * lm[k][cand_dev[k][j]], k < n, j < ncand (e2e_decoder.py:284-285 on re2e_ctc_prefix_score's outputs);
 * a candidate outside [0, V) gives NaN. */
int re2e_lm_add_cands(float* local, const float* lm, const int* cand_dev, int n, int ncand, int V, float lm_weight, re2e_stream_t stream);
/* The form re2e_lm_lstm_cell (kind RE2E_LM_PLAN_CELL), re2e_lm_lstm_cell_zo (RE2E_LM_PLAN_CELL_ZO) or re2e_lm_output (RE2E_LM_PLAN_OUTPUT)
 * runs a call with, as one line of space-separated key=value pairs in `out`; nothing is launched and no pointer is dereferenced (the form
 * follows from the row count and from the widest load every row of every operand is aligned for, so the query takes the call's own
 * pointers and leading dimensions).  Cell kinds: x, ldx, I, w_ih, w_hh, h_prev, n, H as in the call (V is ignored) ->
 *   family=lm_cell zo=0|1 rows=4|8|16 vi=.. vh=.. grid=Hx1x1 block=128 trips=..     (vi, vh) in (4,4), (4,2), (2,2), (1,1): floats per load of
 * the W_ih x and W_hh h products; rows: activation rows per trip of a workgroup, trips = ceil(n / rows).  RE2E_LM_PLAN_OUTPUT: h_prev = the
 * call's h, w_hh = its w, with n, H, V (x, ldx, I, w_ih are ignored) ->
 *   family=lm_out rows=4|8|16 vec=4|2|1 grid=ceil(V/4)x1x1 block=128 trips=.. */
#define RE2E_LM_PLAN_CELL 0
#define RE2E_LM_PLAN_CELL_ZO 1
#define RE2E_LM_PLAN_OUTPUT 2
int re2e_lm_plan(int kind, const float* x, long ldx, int I, const float* w_ih, const float* w_hh, const float* h_prev, int n, int H, int V,
                 char* out, size_t out_bytes);

/* ---- Word-level LMs in the beam search (model/extlm.py; extlm.py:75-216 upstream; csrc/wordlm.hip) ----
 * The lexical tree is flat int32 arrays on the device: N nodes, node 0 the root; wid[N] the word id of a word end or -1; lo[N], hi[N] the
 * word-set range of the node as indices into a row of cumulative word probabilities (mass = c[hi] - c[lo]; lo < 0 marks the root: mass 1);
 * child_off[N+1], child_label[nchild], child_node[nchild]: the children of node k are entries child_off[k] .. child_off[k+1]-1, labels
 * ascending.  A row's node is in [-1, N): -1 = no path in the tree (open-vocabulary mode).  Few-row kernels (n = the live hypotheses of a
 * position), no workspace; every output element is written.  at_space: 1 = the row's label was <space> (or the initial position), 0 = not,
 * -1 = the row's label or node was out of range -- such a row is NaN in re2e_wlm_lookahead / re2e_wlm_multilevel_fix; an index read from
 * the tree that falls outside its array gives NaN as well, never an out-of-range access.
 * Per row r < n: labels[r] == space -> node_new = 0, word_in = wid[node_prev[r]] if that node is a word end, else word_unk, at_space = 1;
 * otherwise node_new = the child of node_prev[r] with label labels[r], or -1 (also when node_prev[r] == -1), word_in = word_unk,
 * at_space = 0.  A label outside [0, Vc) or a node outside [-1, N): node_new = -1, at_space = -1.  node_prev == NULL: every row at the root. */
int re2e_wlm_transition(const int* node_prev, const int* labels, int n, int Vc, int space, int word_unk, const int* wid,
                        const int* child_off, const int* child_label, const int* child_node, int N, int nchild, int* node_new,
                        int* word_in, int* at_space, re2e_stream_t stream);
/* cumsum[dst_rows[j]][v] = sum_{u <= v} softmax(logits[j])[u] for the m rows of logits (m, Vw) into a (n, Vw) buffer (dst_rows == NULL: row
 * j; an entry outside [0, n) is skipped; other rows are left as they are).  One workgroup per row.  The probabilities are fp32
 * (expf(x - max) / sum); all running sums are fp64, rounded to fp32 once at the store.  Any Vw. */
int re2e_wlm_softmax_cumsum(const float* logits, int m, int Vw, const int* dst_rows, int n, float* cumsum, re2e_stream_t stream);
/* LookAheadWordLM's label log-probabilities (extlm.py:195-216), log_y (n, Vc), from cumsum (n, Vw), the rows' nodes and at_space flags:
 * y = unk_prob * oov_penalty by default, (c[hi] - c[lo]) / sum_prob for a child label, the word's own probability (times P(<eos>)) for
 * <space> (<eos>) at a word end, 1e-10 for both right after a <space> elsewhere; log_y = log(y), each step one fp32 operation in that
 * order.  Node -1: a row of zeros, or of -1e10 when open_vocab == 0. */
int re2e_wlm_lookahead(const float* cumsum, int n, int Vw, const int* node, const int* at_space, const int* wid, const int* lo,
                       const int* hi, const int* child_off, const int* child_label, const int* child_node, int N, int nchild, int Vc,
                       int space, int eos, int word_unk, int word_eos, float oov_penalty, int open_vocab, float* log_y,
                       re2e_stream_t stream);
/* MultiLevelLM's tail (extlm.py:120-143): log_y (n, Vc) = subwordlm_weight * lsm (the character LM's log-softmax rows) with, for a row not
 * at a <space>, log_y[space] = wlm_logprobs[wid of the node] - clm (word end) or wlm_logprobs[word_unk] + log_oov_penalty, log_y[eos] =
 * that + wlm_logprobs[word_eos]; at a <space> both are -1e10.  clm_out (n) = 0 at a <space>, else clm_prev + log_y_prev[r][labels[r]].
 * clm_prev, log_y_prev and labels all NULL: the initial position.  Node -1 with open_vocab == 0 and not at a <space>: a row of -1e10,
 * clm_out = 0.  log_y must not alias lsm or log_y_prev. */
int re2e_wlm_multilevel_fix(const float* lsm, const float* wlm_logprobs, int n, int Vw, const int* node, const int* at_space,
                            const int* wid, int N, const float* clm_prev, const float* log_y_prev, const int* labels, int Vc,
                            int space, int eos, int word_unk, int word_eos, float subwordlm_weight, float log_oov_penalty,
                            int open_vocab, float* log_y, float* clm_out, re2e_stream_t stream);

/* ---- N-gram (ARPA back-off) LMs in the beam search (model/ngram.py; NgramCharacterKenLM, extlm.py:46-72 upstream; csrc/ngram.hip) ----
 * The model is flat arrays on the device: N nodes, node 0 the root (the empty context), one node per n-gram of length 1 .. order-1.  Per
 * node: bo[N] its back-off weight, bo_node[N] the node of its longest proper suffix that is a node (the root for the root), succ_off[N+1]
 * its successors as entries succ_off[k] .. succ_off[k+1]-1 of succ_label (ascending inside a node), succ_logp and succ_next (nsucc entries
 * each; succ_next = the node of the longest suffix of context.label that is a node).  The root's successors are the dense rows uni_logp[V],
 * uni_next[V]; its CSR list is empty.  All values are natural logarithms in fp32.  order: 1 .. 8 (a back-off chain has at most order nodes,
 * the root included; chains are followed for at most 8).  No workspace; any n; every element of every output is written.
 * re2e_ngram_step, one search position.  Row r < n: s = state_in[r] (state_in == NULL: the root) advances by x[r]: along s, bo_node[s], ..,
 * root the first node that has x[r] among its successors (binary search; the root has every label) gives state_out[r] = that entry's next.
 * Then with d0 = state_out[r], d_{i+1} = bo_node[d_i]: lp_out[r][v] = (bo[d0] + .. + bo[d_{j-1}]) + logp_j(v), j the first level of that
 * chain that holds v; the back-offs are added in fp32 from the deep end, then the log-probability in one more fp32 addition (level 0:
 * 0 + logp), so a row's bits depend on nothing but its state and label.  att (n,V) and comb_out (n,V) go together (both NULL or neither):
 * comb_out = att + lm_weight * lp_out, the product rounded to fp32, then the sum (e2e_decoder.py:272).  A state outside [0, N), a label
 * outside [0, V) or an index read from the tables that falls outside its array: that row is NaN in lp_out (and comb_out) and -1 in
 * state_out, never an out-of-range access; other rows are not affected.  One workgroup per row and 4096 labels. */
int re2e_ngram_step(const float* uni_logp, const int* uni_next, const float* bo, const int* bo_node, const int* succ_off,
                    const int* succ_label, const float* succ_logp, const int* succ_next, int N, int nsucc, int V, int order,
                    const int* state_in, const int* x, int n, const float* att, float lm_weight, int* state_out, float* lp_out,
                    float* comb_out, re2e_stream_t stream);
/* The summed log-probability of S label sequences (rescoring, perplexity): labels (S, Lmax) int32, lens[S] in [0, Lmax].  Sequence q starts
 * from the context [eos] (node uni_next[eos]); its labels are scored in ascending position, then eos when append_eos != 0; every term is
 * the fp32 value re2e_ngram_step gives that label, the terms are added in double: total_out[q] (S doubles on the device).  A length or a
 * label out of range gives NaN.  One thread per sequence. */
int re2e_ngram_score_seqs(const float* uni_logp, const int* uni_next, const float* bo, const int* bo_node, const int* succ_off,
                          const int* succ_label, const float* succ_logp, const int* succ_next, int N, int nsucc, int V, int order,
                          const int* labels, int Lmax, const int* lens, int S, int eos, int append_eos, double* total_out,
                          re2e_stream_t stream);

/* ---- N3 beam pruning on the device (csrc/beamsearch.hip), several utterances per launch.  The nh rows of a position are grouped by
 * utterance: utterance u owns rows seg_off_dev[u] .. seg_off_dev[u+1]-1 (U+1 offsets; max_seg_rows = the largest group, known to the host).
 * hyp_score (nh); local (nh,ncand) = the scores of each row's continuations; cand_dev (nh,ncand) = their labels, or NULL when the label is the
 * column (ncand = V).  Per utterance the min(beam, rows * ncand) best by score = hyp_score[row] + local[row][col] (one fp32 addition), ordered
 * as recognize_beam's host loop orders them -- score descending, then row ascending, then local descending, then column ascending -- go to
 * parent_out (row index among the nh), col_out, label_out, score_out, all (U,beam), and count_out (U); entries beyond the count are -1 / -inf.
 * A NaN ranks as -inf (as in re2e_ctc_prefix_score's selection).  workspace: 2 * nh * min(beam, ncand) 4-byte words.  beam <= 64 and
 * max_seg_rows <= beam (RE2E_EUNSUPPORTED beyond). */
int re2e_beam_prune(const int* seg_off_dev, int U, int max_seg_rows, const float* hyp_score, const float* local, const int* cand_dev, int nh,
                    int ncand, int beam, int* parent_out, int* col_out, int* label_out, float* score_out, int* count_out, void* workspace,
                    size_t workspace_bytes, re2e_stream_t stream);

/* ---- K12 scoring (csrc/align.hip): weighted edit-distance alignment of n_pairs pairs of integer label sequences in one launch -- in practice
 * every n-best hypothesis of every utterance of a test set (utils/score.py).  ref_labels / hyp_labels: flat int32 arrays on the device, of
 * n_ref_labels / n_hyp_labels entries; ref_off_host (n_ref + 1) and hyp_off_host (n_pairs + 1): offsets into them; pair_ref_host (n_pairs): the
 * reference of pair n, so that an utterance's n-best shares one reference.  The three tables are HOST arrays: the call checks them (offsets
 * non-decreasing and inside the arrays, pair_ref in range, lengths within the limit), copies them to the head of the workspace and waits for
 * that copy on `stream`; a table that fails a check launches nothing and leaves the outputs untouched.
 *   D[0][0] = 0, D[i][0] = i deletions, D[0][j] = j insertions; cell (i, j) takes the best of, in this order, the diagonal (ref[i-1] == hyp[j-1]:
 *   a correct label at cost 0, else a substitution at c_sub), a deletion from (i-1, j) at c_del, an insertion from (i, j-1) at c_ins.  Best: the
 *   smallest (cost, number of errors S+D+I) pair, compared lexicographically; on a full tie the earlier candidate.  Exact integers throughout.
 * counts (n_pairs, 6) int32 = cost, errors, C, S, D, I of the path those choices define.  path (optional, with path_off_host (n_pairs + 1), host,
 * non-decreasing, pair n owning at least |ref| + |hyp| bytes, the last offset <= path_bytes): the path from its start, one byte per step
 * ('C' / 'S' / 'D' / 'I'); the rest of the pair's bytes is set to 0, nothing else is touched.  Every output is a function of its pair alone:
 * two calls give the same bytes.  Costs 1 .. 255 (RE2E_EINVAL beyond); at most 1024 labels per sequence (RE2E_EUNSUPPORTED beyond); empty
 * sequences are legal.  workspace: re2e_align_counts_workspace_bytes of the same tables (with_path: 2 bits per cell on top of the tables; 0 when
 * the tables fail the checks, with the message set), 16-byte aligned. */
size_t re2e_align_counts_workspace_bytes(const int* ref_off_host, int n_ref, const int* hyp_off_host, const int* pair_ref_host, int n_pairs,
                                         int with_path);
int re2e_align_counts(const int* ref_labels, const int* ref_off_host, int n_ref, long n_ref_labels, const int* hyp_labels,
                      const int* hyp_off_host, const int* pair_ref_host, int n_pairs, long n_hyp_labels, int c_sub, int c_ins, int c_del,
                      int* counts, unsigned char* path, const long* path_off_host, long path_bytes, void* workspace, size_t workspace_bytes,
                      re2e_stream_t stream);

/* ---- K11 optimizer (joint_train.py:131-140,188-193; Appendix A.16) ------------------------ */
/* stats[0]=||g||_2, stats[1]=clip coefficient (<=1), stats[2]=1 if finite else 0; from sumsq[0];
 * stats[3..5] = the same with coefficient 1 (NaN gate only).  stats_dev holds 6 floats. */
int re2e_clip_coef(const float* sumsq_dev, float max_norm, float* stats_dev, re2e_stream_t stream);
/* g <- coef*g applied on the fly; skipped entirely when stats[2]==0 (NaN guard, no host sync) */
int re2e_adadelta_step(float* p, const float* g, float* sq_avg, float* acc_delta, long n, float rho, float eps,
                       float lr, const float* stats_dev, re2e_stream_t stream);
/* torch.optim.Adam's step at step count `step` (>= 1).  beta1 / beta2 are doubles: 1 - beta and the bias corrections 1 - beta^step are taken
 * in double on the host, as torch takes them in Python floats (as floats, 1 - 0.999f alone is 1.3e-5 off). */
int re2e_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2,
                   float eps, int step, const float* stats_dev, re2e_stream_t stream);
/* p -= lr * stats[1] * g (plain SGD on the clipped gradient: lm_train.py); skipped entirely when stats[2]==0.  stats_dev NULL: coefficient 1. */
int re2e_sgd_step(float* p, const float* g, long n, float lr, const float* stats_dev, re2e_stream_t stream);

/* ---- L1 unidirectional LSTM over one truncated-BPTT window (csrc/lmseq.hip): the recurrence of RNNLM training (lm_train.py).  Time-major.
 * gates (T,B,4H) holds x W_ih^T + b_ih + b_hh (gate order i,f,g,o) on entry and the ACTIVATED gates on exit of re2e_lmseq_fwd;
 * re2e_lmseq_bwd overwrites them with d(pre-activation gates).  hbuf / cbuf are (T+1,B,H): block 0 is the initial state, written by the
 * caller and left untouched (the convention of re2e_dec_loop_fwd), block t+1 the state after step t.  dy (T,B,H): the gradient of every h[t];
 * dh_last / dc_last (B,H), optional (NULL = zeros): the gradient flowing in through the final state; dh0 / dc0 (B,H), optional outputs: the
 * gradient flowing out through the initial state.  Any H >= 1 and B >= 1; no alignment beyond 4 bytes is assumed of any operand; gates must
 * stay below 2^31 elements.  One launch per time step on `stream` (+ one for dh0), fp32 MFMA: every product is one k-ordered fmaf chain
 * that starts from the value it is added to.  workspace: re2e_lmseq_workspace_bytes(B, H) (the dc carry; the forward needs none). */
size_t re2e_lmseq_workspace_bytes(int B, int H);
int re2e_lmseq_fwd(float* gates, const float* w_hh, float* hbuf, float* cbuf, int T, int B, int H,
                   void* workspace, size_t workspace_bytes, re2e_stream_t stream);
int re2e_lmseq_bwd(float* gates, const float* w_hh, const float* dy, const float* dh_last, const float* dc_last,
                   const float* cbuf, float* dh0, float* dc0, int T, int B, int H,
                   void* workspace, size_t workspace_bytes, re2e_stream_t stream);
/* The form re2e_lmseq_fwd (backward == 0) / re2e_lmseq_bwd runs this window with, as one line of space-separated key=value pairs in `out`;
 * nothing is launched.   family=fwd_step|bwd_step mfma=16x16x4 rows=.. units=.. acc=.. kc=.. grid=XxYx1 lds=.. launches=.. rounds=..
 * (rows x units: the workgroup's tile; acc: independent accumulators per wave; launches: one per step; rounds: workgroups per CU).
 * cus > 0: plan for a chip of that many CUs (no device is touched); cus == 0: the current device's count. */
int re2e_lmseq_plan(int T, int B, int H, int backward, int cus, char* out, size_t out_bytes);

/* ---- L2 fast-slow RNN over one truncated-BPTT window (csrc/fsrnn.hip): the recurrence of the FS-RNN LM (model/fsrnn.py; fsrnn.py:96-127).
 * One step is a chain of L + 1 LSTM cells of width H, each followed by zoneout: F0 (input hoisted into gates[0]) -> S (input d1 . F0) ->
 * F1 (input d2 . S) -> F2 .. F(L-1) (no input) -> F0 of the next step.  Cell index 0 .. L-1 = fast cells, L = the slow cell.  Time-major:
 *   gates (L+1,T,B,4H)   gates[0] holds x W_ih^T + b_ih + b_hh of F0 (gate order i,f,g,o) on entry; every cell's ACTIVATED gates on exit of
 *                        re2e_fsrnn_fwd; re2e_fsrnn_bwd overwrites them with d(pre-activation gates) (gates[0]: the gradient of its input)
 *   hbuf, cbuf (L+1,T+1,B,H)   block t+1 of cell c: its state after zoneout at step t.  Block 0 of cells L-1 and L is the initial fast /
 *                        slow state, written by the caller and left untouched; block 0 of the other cells is unused (never read or written)
 *   hd (2,T,B,H)         with dm: d1 . hbuf[0][t+1] and d2 . hbuf[L][t+1], the inputs of S and F1 (written by the forward)
 *   mh, mc (L+1,T,B,H)   zoneout masks per cell and step: new = mask . new + (1 - mask) . old; NULL: the scalars keep_h / keep_c
 *   dm (2,T,B,H)         the dropout masks d1 and d2 with their scale 1 / (1 - p) in them; NULL (then hd is NULL too): no dropout
 * w_ih, w_hh, b_ih, b_hh: HOST arrays of L+1 device pointers, (4H,H) / (4H) each; w_ih[1], w_ih[L] and every w_hh are read, the biases of
 * cells 1 .. L are read by the forward only, everything else may be NULL.  dy (T,B,H): the gradient of hbuf[L-1][1:]; d_fh / d_fc / d_sh /
 * d_sc (B,H), optional (NULL = zeros): the gradient flowing in through the final state; d_fh0 .. d_sc0 (B,H), optional outputs: the gradient
 * flowing out through the initial state.  Any H >= 1, B >= 1, 2 <= L <= 64; nothing beyond 4-byte alignment is assumed; one cell's gates
 * (T,B,4H) must stay below 2^31 elements.  L + 1 launches per time step on `stream`, the backward one more for each of d_fh0 / d_sh0.
 * workspace: re2e_fsrnn_workspace_bytes(B, H) (the backward's four carries; the forward needs none). */
size_t re2e_fsrnn_workspace_bytes(int B, int H);
int re2e_fsrnn_fwd(float* gates, float* hbuf, float* cbuf, float* hd, const float* const* w_ih, const float* const* w_hh,
                   const float* const* b_ih, const float* const* b_hh, const float* mh, const float* mc, const float* dm, float keep_h,
                   float keep_c, int T, int B, int H, int L, void* workspace, size_t workspace_bytes, re2e_stream_t stream);
int re2e_fsrnn_bwd(float* gates, const float* cbuf, const float* const* w_ih, const float* const* w_hh, const float* mh, const float* mc,
                   const float* dm, float keep_h, float keep_c, const float* dy, const float* d_fh, const float* d_fc, const float* d_sh,
                   const float* d_sc, float* d_fh0, float* d_fc0, float* d_sh0, float* d_sc0, int T, int B, int H, int L, void* workspace,
                   size_t workspace_bytes, re2e_stream_t stream);
/* The form re2e_fsrnn_fwd (backward == 0) / re2e_fsrnn_bwd runs this window with, as one line of space-separated key=value pairs in `out`;
 * nothing is launched.   family=fsrnn_fwd_step|fsrnn_bwd_step mfma=16x16x4 rows=.. units=.. acc=.. kc=.. grid=XxYx1 lds=.. cells=.. launches=..
 * rounds=..   (launches: cells x T; rounds: workgroups per CU and launch).  cus > 0: a chip of that many CUs (no device is touched). */
int re2e_fsrnn_plan(int T, int B, int H, int L, int backward, int cus, char* out, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RE2E_H */
