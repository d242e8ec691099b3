// Shared device/host helpers for the re2e HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include "../../include/re2e.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define RE2E_WAVE 64

void re2e_set_error(const char* fmt, ...);
bool re2e_stream_is_filler(hipStream_t stream);     // core.hip: re2e_stream_role
int re2e_cu_count();                                // core.hip: CUs of the current device; 256 without one

#define RE2E_CHECK_ARG(cond, msg)                     \
  do {                                                \
    if (!(cond)) {                                    \
      re2e_set_error("%s: %s", __func__, msg);        \
      return RE2E_EINVAL;                             \
    }                                                 \
  } while (0)

#define RE2E_LAUNCH_CHECK()                                                        \
  do {                                                                             \
    hipError_t e__ = hipGetLastError();                                            \
    if (e__ != hipSuccess) {                                                       \
      re2e_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e__));   \
      return RE2E_EHIP;                                                            \
    }                                                                              \
  } while (0)

// Experiment switches.  The shipped library reads eight environment variables, each covered by a parity test or result-neutral:
//   RE2E_LSTM_PERSIST / RE2E_LSTM_PERSIST_BWD = 0  launch-per-step recurrences (tests/test_kernels_gpu.py: persistent vs stepwise)
//   RE2E_LSTM_FWD2 / RE2E_LSTM_BWD3 = 0            the round-1..3 recurrence kernels instead of the round-4 forms (same test; they
//                                                  also serve the hidden sizes the round-4 forms are not built for)
//   RE2E_LSTM_BWD_UW = 1 | 2                       hidden units per backward workgroup / 8 of the round-1..3 kernel (same test, forced widths)
//   RE2E_DEC_PERSIST = 0 | 2                       launch-per-token decoder loop (2: only its backward) instead of csrc/decloop.hip (same file:
//                                                  decoder loop persistent vs stepwise, forward and backward)
//   RE2E_IGEMM_LOG                                 one stderr line per engine call (tools/igemm_table.py), no effect on results
//   RE2E_DEBUG_HOOKS = 1                           lets re2e_debug_force_abort / re2e_debug_occupy answer (tests/conftest.py sets it)
// Everything else -- occupancy probes, choices between shipped forms and rejected forms kept for A/B measurements -- is compiled in only with
// -DRE2E_EXPERIMENTS (make EXPERIMENTS=1 -> libre2e_hip_exp.so, used by tools/ through RE2E_LIB) and answers "unset" otherwise.  Of the
// recurrences (lstm.hip) that is RE2E_LSTM_STAMPS (phase stamps), RE2E_LSTM_BWD3_UN (tools/lstm_stamps.py) and RE2E_LSTM_WAVES_FWD
// (tools/bench_lstm.py); the switches of their rejected forms went with the forms.  Of the dense and implicit-GEMM
// products it is seven switches that choose between SHIPPED forms, read in one place per file (igemm.hip engine_switches: RE2E_NO_SKINNY_GEMM,
// RE2E_NO_ROW_TAIL, RE2E_TN_XCD_KSLICE, RE2E_IGEMM_NOMEM; gemm_nt.hip nt_switches: RE2E_NT2, RE2E_NT2_TAILWG, RE2E_NT2_LOG) and applied at the top
// of the plan (plan_gemm below); of the convolutions four (igemm.hip conv_switches: RE2E_NO_THIN, RE2E_NO_COUT1_ROWS, RE2E_NO_HALO, RE2E_CONV_NT2),
// read at the top of plan_conv, beside the Winograd kernels' probes (RE2E_WINO_LDS_KB / _LDSIN / _DBG / _STAMPS, RE2E_WW_DBG / _FLAT).  The
// rejected forms and their switches went with their measurements kept in DESIGN.md Appendix A.
#ifdef RE2E_EXPERIMENTS
static inline const char* exp_env(const char* name) { return getenv(name); }
#else
static inline const char* exp_env(const char*) { return nullptr; }
#endif

// Dynamic-LDS limit of one kernel, raised on demand.  The library is re-entrant (include/re2e.h): the only process-wide state
// are these idempotent attribute caches; the mutex keeps two host threads that ask for different sizes from leaving the smaller one set.
struct LdsLimit {
  std::mutex m;
  size_t set = 0;
  void ensure(const void* fn, size_t bytes) {
    std::lock_guard<std::mutex> g(m);
    if (bytes > set) {
      (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      set = bytes;
    }
  }
};

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
// tanh via exp; accurate to ~1e-7 relative for |x|<10, saturates cleanly
__device__ __forceinline__ float tanhf_(float x) {
  float ax = fabsf(x);
  float e = __expf(-2.0f * ax);
  float t = (1.0f - e) / (1.0f + e);
  return copysignf(t, x);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Block-wide sum for blockDim.x <= 1024 (fixed tree => deterministic).  `red` >= 16 floats of LDS.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  int nw = (blockDim.x + 63) >> 6;
  float r = 0.f;
  for (int i = 0; i < nw; ++i) r += red[i];
  return r;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  int nw = (blockDim.x + 63) >> 6;
  float r = -3.0e38f;
  for (int i = 0; i < nw; ++i) r = fmaxf(r, red[i]);
  return r;
}

// Top-k of a row held in LDS by a 256-thread workgroup: k rounds of a workgroup arg-max, descending, ties -> lower index (torch.topk
// order).  The row holds no NaN on entry (the callers store NaN scores as -inf); an entry that has been selected is marked with NaN and
// skipped afterwards, so the k results are always k DISTINCT valid indices -- also for rows with fewer than k entries above -inf.
// k <= n (an unselected entry always exists); red_v / red_i: 4 entries of LDS each; the row is published before the call and the
// results are after it.
__device__ __forceinline__ void block_topk256(float* row, int n, int k, int* out_i, float* out_v, float* red_v, int* red_i) {
  constexpr int NONE = 0x7fffffff;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY; int bi = NONE;
    for (int i = tid; i < n; i += 256) { const float v = row[i]; if (v == v && (bi == NONE || v > bv)) { bv = v; bi = i; } }   // ascending i: first maximum wins
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
      if (oi != NONE && (bi == NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[wid] = bv; red_i[wid] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w) if (red_i[w] != NONE && (bi == NONE || red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi))) { bv = red_v[w]; bi = red_i[w]; }
      out_i[r] = bi; out_v[r] = bv; row[bi] = __uint_as_float(0x7fc00000u);
    }
    __syncthreads();
  }
}

// torch.tanh / torch.relu / F.leaky_relu(0.2) / torch.sigmoid, NaN and +-inf included: a NaN stays a NaN (fmaxf(v, 0) would drop it), ReLU(-inf) = 0
__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case RE2E_ACT_TANH: return tanhf_(v);
    case RE2E_ACT_RELU: return v < 0.f ? 0.f : v;
    case RE2E_ACT_LRELU: return v > 0.f ? v : 0.2f * v;
    case RE2E_ACT_SIGMOID: return sigmoidf_(v);
    default: return v;
  }
}

// im2col geometry over an NHWC tensor: logical pixel grid (NI, PH, PW) -> input coordinate
// iy = py*SY + kh*DY + OY0, ix = px*SX + kw*DX + OX0 ; taps KH x KW ; C channels innermost.
struct ConvGeom {
  const float* in; int NI, H, W, C; int PH, PW; int KH, KW; int SY, SX, DY, DX, OY0, OX0;
};

// Output placement of a convolution row m = (n, py, px): plain (m*ldc) or, for the stride-2
// data-gradient parity classes, ((n*OHF + py*osy+ooy)*OWF + px*osx+oox)*ldc.
struct OutMap {
  float* out; long ldc; int remap; int PH, PW, OHF, OWF, osy, osx, ooy, oox;
  __device__ long off(int row) const {
    if (!remap) return (long)row * ldc;
    int j = row % PW; int t = row / PW; int i = t % PH; int n = t / PH;
    return (((long)n * OHF + i * osy + ooy) * OWF + j * osx + oox) * ldc;
  }
};

// K-sliced batches of products for wino44.hip (igemm.hip): out[z][M][N] over K / ns slices of the contraction, through plan_gemm below
int gemm_kslices_tn(int M, int N, int K, int ns, const float* A, long lda, const float* B, long ldb, float* out, hipStream_t st, int nolog = 0);
int gemm_kslices(int M, int N, int K, int ns, const float* A, long lda, const float* B, long ldb, float* out, hipStream_t st, int nolog = 0);

// ---- which kernel serves a dense product: the plan (igemm.hip plan_gemm; printed by re2e_gemm_plan) -----------------------------------------------
// gemm_nt.hip's part: the x W^T product as an LDS-DMA pipelined kernel, whole tiles (n_dp workgroups) + a stream-K tail (g_sk workgroups sharing
// the k-tiles of the tiles of the last partial round; bytes = the slabs of its cut tiles).  variant = 0: the pipeline does not serve the product.
struct NtPlan { int variant; int wg_per_cu; int bm, bn, bk; int ntm, ntn, nkt, n_dp, g_sk; size_t bytes; double est; };
NtPlan nt2_plan(int M, int N, int K, bool four_wave, int cus, bool stream_k);
bool nt2_operands_ok(int rows, int N, int K, const float* A, long lda, const float* B, long ldb, const float* C, long ldc, const float* bias, const float* bias2);
int* nt2_ticket_slice();      // zeroed arrival tickets for the cut tiles of one launch; nullptr: none to be had
void gemm_nt2(const NtPlan& pl, int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc, const float* bias, const float* bias2,
              int act, float beta, float* slabs, int* tickets, hipStream_t st, const int* rowmap, int phys_rows, int ident_rows, int kslices, int nolog);
// Everything the choice depends on, and nothing else.  a16 / b16: base 16-byte aligned and leading dimension % 4 == 0 (the plan adds the shape's part:
// no float4 may straddle a bound); pipe16: A, B, C and the biases are what nt2_operands_ok asks for.  kslices > 0: a K-sliced batch (K = all slices).
struct GemmIn { int transa, transb, M, N, K, act; bool a16, b16, pipe16, rowmap, filler; int cus, kslices; };
enum GemmRoute { kSkinnyWg, kPipeline, kEngine };
struct GemmPlan {
  // stream-independent: the same for a call on the main stream and on a filler stream (re2e_gemm_workspace_bytes sees no stream)
  size_t ws_bytes;       // what re2e_gemm_workspace_bytes answers; filled only where asked for
  int splits;            // engine: K slices (1: no slabs, no reduce)
  size_t need_bytes;     // workspace the route uses: the engine's slabs or the pipeline's
  // stream-dependent
  GemmRoute route;
  bool vec;              // skinny_wg, engine: the <.., VEC> instantiation (16-byte loads)
  int tile;              // engine: row of igemm.hip's tile table
  int m1;                // engine: rows [0, m1) run on `tile`, rows [m1, M) on the 64x64 row tail; M = no tail
  NtPlan nt;             // pipeline
};
GemmPlan plan_gemm(const GemmIn& in, bool with_workspace = false);
// ---- which kernel serves a convolution: the plan (igemm.hip plan_conv; printed by re2e_conv_plan) --------------------------------------------------
// Everything the choice depends on, and nothing else: the call kind, the ConvGeom-level geometry without its pointer, the output map, the epilogue,
// what is asked for beside the product (ReLU mask, fused pool), which operands are 16-byte aligned (absent ones count as aligned), the stream's
// role and the chip's CU count.  kConvIgemm: re2e_conv_igemm / _masked / re2e_conv3x3_relu_pool -- a forward (D = 1), a stride-1 data gradient
// (D = -1) or ONE parity class of a stride-2 data gradient (remap); kConvDgradS2: re2e_conv_dgrad_s2, the four parity classes in one launch (the
// geometry of one class, cls_o0[p] = input offset of parity p); kConvWgrad: re2e_conv_wgrad (wg16: the output gradient).
enum ConvKind { kConvIgemm, kConvDgradS2, kConvWgrad };
struct ConvIn {
  ConvKind kind;
  int NI, H, W, C, PH, PW, KH, KW, SY, SX, DY, DX, OY0, OX0, cls_o0[2];
  int Cout, act; float beta;
  bool remap, mask, pool;
  bool in16, wg16, out16, bias16, mask16, pool16, idx4;
  bool filler; int cus;
};
enum ConvRoute { kCin1Fwd, kCout1Rows, kCout1, kHalo, kConvPipeline, kConvEngine, kWgradCin1, kWgradCout1, kWgradEngine, kConvNone };
struct ConvPlan {
  ConvRoute route;       // kConvNone: a fused pool was asked for on a geometry the halo-patch kernel does not take (RE2E_EUNSUPPORTED)
  bool mask_pass;        // the separate relu_mask_kernel pass follows (a ReLU mask on the engine)
  bool note_2gib;        // a halo-patch geometry left to the pipeline / engine for a tensor of 2 GiB or more: the entry point says so, once per process
  int grid; size_t lds;  // thin and halo kernels
  int L, kh, kw, ch;     // thin: cin1_fwd<kh, kw>; cout1<L, kh, kw, ch> (0: the run-time loops)
  int th, tw, dir, nitems; bool relu;      // halo: patch, direction, ReLU instantiation, work items (one per workgroup)
  NtPlan nt; long shift; // pipeline: whole tiles only, n_dp = classes x tiles; bytes the descriptor starts in front of the tensor
  int tile; bool vec;    // engine (forward, data gradient and weight gradient): row of igemm.hip's tile table, 16-byte loads
  int splits; bool wide_reduce; size_t need_bytes, ws_bytes;      // weight gradient: slabs (thin: their count), the reduce, the workspace the call uses
  //                                                                  and what re2e_conv_wgrad_workspace_bytes answers (it sees no pointers and no stream)
};
ConvPlan plan_conv(const ConvIn& in);
// The parts of the plan the kernels' own files state (pure: eligibility and launch geometry, nothing enqueued), and the functions that enqueue a
// plan -- they cannot decline.  thinconv.hip: direct kernels for Cout == 1 (forward) and Cin == 1 / Cout == 1 (weight gradient), where an MFMA tile
// would be >= 97 % padding; thin_wgrad_slabs returns 0 when the shape is not covered.
bool thin_fwd_plan(const ConvIn& in, bool no_rows, ConvPlan& p);
void thin_conv_forward(const ConvPlan& p, const ConvGeom& g, const float* wg, int Cout, const OutMap& o, const float* bias, int act, float beta, hipStream_t st);
int thin_wgrad_slabs(int C, int Cout, int KH, int KW, long P, long rows, int PW, int SX);
void thin_wgrad(const ConvGeom& g, const float* dout, int Cout, float* slabs, int nslab, hipStream_t st);
// conv3x3.hip: 3x3 / stride-1 / pad-1 convolutions with C % 16 == 0 and Cout % 64 == 0 (halo patch staged once per channel chunk, taps walked in LDS)
bool halo_plan(const ConvIn& in, ConvPlan& p);
void halo_note_2gib(const ConvIn& in);
void halo_conv3x3(const ConvPlan& p, const ConvGeom& g, const float* wg, int Cout, float* out, const float* bias, int act, float beta, const float* mask,
                  hipStream_t st, float* pool_out = nullptr, unsigned char* pool_idx = nullptr);
// gemm_nt.hip: the pipeline's implicit-GEMM form (forward / data gradient; ncls = 4: the output parity classes of a stride-2 data gradient), whole tiles only
bool conv_nt2_plan(const ConvIn& in, ConvPlan& p);
void conv_nt2(const ConvPlan& p, const ConvGeom& g, int M, const float* wg, int Cout, float* out, long ldc, const float* bias, int act, float beta, int ncls,
              const int* cls_oy0, const int* cls_ox0, long cls_wstride, int remap, int OHF, int OWF, int osy, int osx, const int* ooy, const int* oox,
              hipStream_t st);
// What the fused Winograd entry points take, stated once: the entry points answer RE2E_EUNSUPPORTED from these, the layer-level plan
// (igemm.hip plan_conv_layer) chooses with them.  winograd.hip / wino_wgrad.hip / wino44.hip.
enum WinoFit { kWinoFits, kWinoChannels, kWinoGroups, kWinoBytes, kWinoItems };
WinoFit wino3x3_fit(int NI, int H, int W, int C, int Cout);
int wino3x3_images(int N, int H, int W, int C, int Cout);      // images per launch: all of them, or as many as keep both tensors under 2 GiB
WinoFit wino3x3_wgrad_fit(int NI, int H, int W, int C, int Cout);
WinoFit wino4x4_fit(int NI, int H, int W, int C, int Cout, int pad);
WinoFit wino4x4_wgrad_fit(int NI, int H, int W, int C, int Cout, int pad);
