// Unidirectional LSTM over one truncated-BPTT window, for training the RNNLM (model/lm.py forward_seq): carried initial state, any
// hidden size, no alignment assumed.  Two step kernels, each launched ONCE PER TIME STEP on the caller's stream -- every launch ends on
// its own, there are no flags between workgroups; where the work splits across workgroups it splits by launch.
//
//   forward step t   gates[t] (B,4H) += h[t-1] (B,H) W_hh^T, then the cell in the epilogue of the same launch.  A workgroup owns 64 rows
//                    x 16 units and ALL FOUR gates of those units (rows j, H+j, 2H+j, 3H+j of W_hh): wave w holds rows 16w .. 16w+15 as
//                    four 16x16 accumulators of v_mfma_f32_16x16x4_f32, one per gate, which put the same (row, unit) element of every gate
//                    on the same lane and register -- so the cell needs no second pass over memory and no exchange.
//   backward step t  dh = dy[t] + dgates[t+1] (B,4H) W_hh (K = 4H, N = H), then the cell backward on the same (row, unit) elements.  A
//                    workgroup owns 64 rows x 32 units: two independent accumulators per wave.  With gates == NULL the epilogue is the
//                    identity (the trailing dh0 = dgates[0] W_hh).
//
// Both stage their operands through LDS in chunks of 32 k with 4-byte loads predicated on row and k (a remainder is zero-filled, nothing is
// read past a row; W_hh rows at H = 650 are only 8-byte aligned), the next chunk's loads in flight over the current chunk's MFMAs.  The
// accumulator starts from the tensor the product is added to, so every result is ONE k-ordered fmaf chain: fma(a_K-1, b_K-1, ... fma(a_0, b_0, c)).
#include "common.h"

namespace {

constexpr int KC = 32;         // k per staged chunk
constexpr int LDA = KC + 4;    // row pitch of a [row][k] LDS tile: 36 r + q (r < 16, q < 4) hits 64 different banks
constexpr int BM = 64;         // rows per workgroup: 4 waves x 16
constexpr int FWD_UN = 16;     // units per forward workgroup (x 4 gates = 64 rows of W_hh)
constexpr int BWD_UN = 32;     // units per backward workgroup
constexpr int LDW = BWD_UN + 16;   // row pitch of the backward's [k][unit] W tile: 48 q + n (q < 4, n < 16) hits 64 different banks

// rows [r0, r0 + 64) x k [k0, k0 + 32) of a (nrows, K) matrix with leading dimension ld: 8 values per thread (row = tid / 32 + 8 i, k = tid % 32)
__device__ __forceinline__ void load_rows(float (&v)[8], const float* __restrict__ src, long ld, int r0, int nrows, int k0, int K) {
  const int k = k0 + (threadIdx.x & 31), r = r0 + (threadIdx.x >> 5);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = r + 8 * i;
    v[i] = (row < nrows && k < K) ? src[(long)row * ld + k] : 0.f;
  }
}
__device__ __forceinline__ void store_rows(float* tile, const float (&v)[8]) {
  const int k = threadIdx.x & 31, r = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 8; ++i) tile[(r + 8 * i) * LDA + k] = v[i];
}

// ---- forward step -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lmseq_fwd_step(float* __restrict__ gates, const float* __restrict__ w_hh, const float* __restrict__ h_prev,
                                                      const float* __restrict__ c_prev, float* __restrict__ h_out, float* __restrict__ c_out,
                                                      int B, int H) {
  __shared__ float As[BM * LDA];
  __shared__ float Ws[4 * FWD_UN * LDA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u0 = blockIdx.x * FWD_UN, b0 = blockIdx.y * BM;
  const int unit = u0 + (lane & 15);
  const long H4 = 4L * H;

  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wave * 16 + (lane >> 4) * 4 + r;
      acc[g][r] = (b < B && unit < H) ? gates[(long)b * H4 + (long)g * H + unit] : 0.f;
    }

  // W tile row (gate g, unit u) = g * 16 + u: thread (row = tid / 32 + 8 i, k = tid % 32)
  float av[8], wv[8];
  auto load_w = [&](int k0) {
    const int k = k0 + (tid & 31), r = tid >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = r + 8 * i, u = u0 + (row & 15);
      wv[i] = (u < H && k < H) ? w_hh[((long)(row >> 4) * H + u) * H + k] : 0.f;
    }
  };
  load_rows(av, h_prev, H, b0, B, 0, H);
  load_w(0);
  const float* a_rd = As + (wave * 16 + (lane & 15)) * LDA + (lane >> 4);
  const float* w_rd = Ws + (lane & 15) * LDA + (lane >> 4);
  for (int k0 = 0; k0 < H; k0 += KC) {
    __syncthreads();                      // the previous chunk has been read
    store_rows(As, av);
    store_rows(Ws, wv);
    __syncthreads();
    if (k0 + KC < H) { load_rows(av, h_prev, H, b0, B, k0 + KC, H); load_w(k0 + KC); }
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const float a = a_rd[ks * 4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w_rd[g * FWD_UN * LDA + ks * 4], acc[g], 0, 0, 0);
    }
  }

  if (unit >= H) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + wave * 16 + (lane >> 4) * 4 + r;
    if (b >= B) continue;
    const float ig = sigmoidf_(acc[0][r]), fg = sigmoidf_(acc[1][r]), gg = tanhf_(acc[2][r]), og = sigmoidf_(acc[3][r]);
    const long e = (long)b * H + unit;
    const float c = fg * c_prev[e] + ig * gg;
    float* grow = gates + (long)b * H4 + unit;
    grow[0] = ig; grow[H] = fg; grow[2L * H] = gg; grow[3L * H] = og;
    c_out[e] = c;
    h_out[e] = og * tanhf_(c);
  }
}

// ---- backward step ----------------------------------------------------------------------------------------------------------------------------
// dh = dy + dh_add + dg_next W_hh (each optional).  gates != NULL: the cell backward (gates: activated in, d pre-activation out; dc_in optional,
// dc_out written; dc_in may be dc_out: an element is read and written by the same lane).  gates == NULL: dh -> dh_out.
__global__ __launch_bounds__(256) void lmseq_bwd_step(const float* __restrict__ dg_next, const float* __restrict__ w_hh, const float* __restrict__ dy,
                                                      const float* __restrict__ dh_add, float* __restrict__ gates, const float* __restrict__ c_prev,
                                                      const float* __restrict__ c_cur, const float* dc_in, float* dc_out, float* __restrict__ dh_out,
                                                      int B, int H) {
  __shared__ float As[BM * LDA];
  __shared__ float Ws[KC * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u0 = blockIdx.x * BWD_UN, b0 = blockIdx.y * BM;
  const int K = 4 * H;
  const long H4 = 4L * H;

  f32x4 acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wave * 16 + (lane >> 4) * 4 + r, unit = u0 + s * 16 + (lane & 15);
      float v = 0.f;
      if (b < B && unit < H) {
        const long e = (long)b * H + unit;
        if (dy) v = dy[e];
        if (dh_add) v += dh_add[e];
      }
      acc[s][r] = v;
    }

  if (dg_next) {
    float av[8], wv[4];
    auto load_w = [&](int k0) {          // W_hh rows k0 .. k0 + 31, columns u0 .. u0 + 31: thread (k = tid / 32 + 8 i, n = tid % 32)
      const int n = u0 + (tid & 31), k = k0 + (tid >> 5);
#pragma unroll
      for (int i = 0; i < 4; ++i) wv[i] = (k + 8 * i < K && n < H) ? w_hh[(long)(k + 8 * i) * H + n] : 0.f;
    };
    load_rows(av, dg_next, H4, b0, B, 0, K);
    load_w(0);
    const float* a_rd = As + (wave * 16 + (lane & 15)) * LDA + (lane >> 4);
    const float* w_rd = Ws + (lane >> 4) * LDW + (lane & 15);
    for (int k0 = 0; k0 < K; k0 += KC) {
      __syncthreads();
      store_rows(As, av);
#pragma unroll
      for (int i = 0; i < 4; ++i) Ws[((tid >> 5) + 8 * i) * LDW + (tid & 31)] = wv[i];
      __syncthreads();
      if (k0 + KC < K) { load_rows(av, dg_next, H4, b0, B, k0 + KC, K); load_w(k0 + KC); }
#pragma unroll
      for (int ks = 0; ks < KC / 4; ++ks) {
        const float a = a_rd[ks * 4];
#pragma unroll
        for (int s = 0; s < 2; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w_rd[ks * 4 * LDW + s * 16], acc[s], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int unit = u0 + s * 16 + (lane & 15);
    if (unit >= H) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wave * 16 + (lane >> 4) * 4 + r;
      if (b >= B) continue;
      const long e = (long)b * H + unit;
      const float dh = acc[s][r];
      if (!gates) { dh_out[e] = dh; continue; }
      float* grow = gates + (long)b * H4 + unit;
      const float ig = grow[0], fg = grow[H], gg = grow[2L * H], og = grow[3L * H];
      const float tc = tanhf_(c_cur[e]);
      const float dc = (dc_in ? dc_in[e] : 0.f) + dh * og * (1.f - tc * tc);
      grow[0] = dc * gg * ig * (1.f - ig);
      grow[H] = dc * c_prev[e] * fg * (1.f - fg);
      grow[2L * H] = dc * ig * (1.f - gg * gg);
      grow[3L * H] = dh * tc * og * (1.f - og);
      dc_out[e] = dc * fg;
    }
  }
}

__global__ void sgd_kernel(float* p, const float* __restrict__ g, long n, float lr, const float* __restrict__ stats) {
  float coef = 1.f;
  if (stats) { if (stats[2] == 0.f) return; coef = stats[1]; }
  const float s = lr * coef;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] -= s * g[i];
}

bool shape_ok(int T, int B, int H) { return T >= 1 && B >= 1 && H >= 1 && (long)T * B * 4L * H < (1L << 31) && cdiv(B, BM) <= 65535; }
size_t carry_bytes(int B, int H) { return ((size_t)B * H * sizeof(float) + 255) / 256 * 256; }

}  // namespace

extern "C" size_t re2e_lmseq_workspace_bytes(int B, int H) { return B >= 1 && H >= 1 ? carry_bytes(B, H) : 0; }

extern "C" int re2e_lmseq_plan(int T, int B, int H, int backward, int cus, char* out, size_t out_bytes) {
  RE2E_CHECK_ARG(out && out_bytes > 0, "no output buffer");
  RE2E_CHECK_ARG(shape_ok(T, B, H), "T, B, H must be >= 1 and gates (T,B,4H) below 2^31 elements");
  if (cus <= 0) cus = re2e_cu_count();
  const int un = backward ? BWD_UN : FWD_UN, gx = cdiv(H, un), gy = cdiv(B, BM);
  const int lds = (int)sizeof(float) * (BM * LDA + (backward ? KC * LDW : 4 * FWD_UN * LDA));
  // launches: one per step (the backward adds the trailing dh0 product when the caller asks for dh0); rounds: workgroups per CU and launch
  const int n = snprintf(out, out_bytes, "family=%s mfma=16x16x4 rows=%d units=%d acc=%d kc=%d grid=%dx%dx1 lds=%d launches=%d rounds=%d",
                         backward ? "bwd_step" : "fwd_step", BM, un, backward ? 2 : 4, KC, gx, gy, lds, T, cdiv((long)gx * gy, cus));
  RE2E_CHECK_ARG(n > 0 && (size_t)n < out_bytes, "output buffer too small");
  return RE2E_OK;
}

extern "C" int re2e_lmseq_fwd(float* gates, const float* w_hh, float* hbuf, float* cbuf, int T, int B, int H, void* workspace, size_t workspace_bytes,
                              hipStream_t stream) {
  (void)workspace; (void)workspace_bytes;          // the forward carries nothing between its launches but hbuf / cbuf
  RE2E_CHECK_ARG(gates && w_hh && hbuf && cbuf, "null pointer");
  RE2E_CHECK_ARG(shape_ok(T, B, H), "T, B, H must be >= 1 and gates (T,B,4H) below 2^31 elements");
  const size_t BH = (size_t)B * H;
  const dim3 grid(cdiv(H, FWD_UN), cdiv(B, BM));
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(lmseq_fwd_step, grid, dim3(256), 0, stream, gates + 4 * BH * t, w_hh, hbuf + BH * t, cbuf + BH * t, hbuf + BH * (t + 1),
                       cbuf + BH * (t + 1), B, H);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}

extern "C" int re2e_lmseq_bwd(float* gates, const float* w_hh, const float* dy, const float* dh_last, const float* dc_last, const float* cbuf, float* dh0,
                              float* dc0, int T, int B, int H, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(gates && w_hh && dy && cbuf, "null pointer");
  RE2E_CHECK_ARG(shape_ok(T, B, H), "T, B, H must be >= 1 and gates (T,B,4H) below 2^31 elements");
  RE2E_CHECK_ARG(workspace && workspace_bytes >= carry_bytes(B, H), "workspace smaller than re2e_lmseq_workspace_bytes");
  const size_t BH = (size_t)B * H;
  float* carry = (float*)workspace;
  const dim3 grid(cdiv(H, BWD_UN), cdiv(B, BM));
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    hipLaunchKernelGGL(lmseq_bwd_step, grid, dim3(256), 0, stream, last ? (const float*)nullptr : gates + 4 * BH * (t + 1), w_hh, dy + BH * t,
                       last ? dh_last : (const float*)nullptr, gates + 4 * BH * t, cbuf + BH * t, cbuf + BH * (t + 1),
                       last ? dc_last : (const float*)carry, (t == 0 && dc0) ? dc0 : carry, (float*)nullptr, B, H);
    RE2E_LAUNCH_CHECK();
  }
  if (dh0) {
    hipLaunchKernelGGL(lmseq_bwd_step, grid, dim3(256), 0, stream, (const float*)gates, w_hh, (const float*)nullptr, (const float*)nullptr, (float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, dh0, B, H);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}

extern "C" int re2e_sgd_step(float* p, const float* g, long n, float lr, const float* stats, hipStream_t stream) {
  RE2E_CHECK_ARG(p && g && n > 0, "bad args");
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, p, g, n, lr, stats);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
