// Fast-slow RNN language model (model/fsrnn.py; fsrnn.py:96-127 upstream) over one truncated-BPTT window.  One time step is a CHAIN of
// L + 1 LSTM cells of the same width H, each followed by zoneout, each depending on the one before:
//     F0 (input: the embedding, hoisted out of time as `pre`)  ->  S (input: d1 . F0's output)  ->  F1 (input: d2 . S's output)
//     ->  F2 .. F(L-1) (no input: b_ih + b_hh + W_hh h only)  ->  F0 of the next step;     the slow state runs step to step.
// Two step kernels in the style of lmseq.hip, each launched ONCE PER CELL AND TIME STEP on the caller's stream: every launch ends on its
// own, there are no flags between workgroups.
//
//   forward cell step   acc = pre | b_ih + b_hh;  acc += x W_ih^T (optional);  acc += h_prev W_hh^T;  then, on the lane that holds the
//                       element: the cell, zoneout against h_prev / c_prev (a mask tensor or the scalar keep), the stores of the activated
//                       gates, h and c, and hd = h . dmask when a dropout mask is given.  64 rows x 16 units x 4 gates per workgroup.
//   backward cell step  dH = dmask . (a1 W1) + add_a + add_b + a2 W2 (each optional; the masked product runs first and is scaled in the
//                       accumulators, the second continues on top), zoneout backward (dh_new = m_h . dH, dc_new = m_c . dC, the
//                       pass-through (1 - m_h) . dH goes to dhp_out), then the cell backward on the same (row, unit) elements: the activated
//                       gates become d(pre-activations), dcp_out = dc . f + (1 - m_c) . dC.  The pre-zoneout cell state is recomputed as
//                       f c_prev + i g.  gates == NULL: dh_out = dH (the gradients of the initial h states).  64 rows x 32 units.
//
// Buffers (time-major; cell index 0 .. L-1 = fast cells, L = the slow cell; BH = B * H):
//   gates (L+1, T, B, 4H)   gates[0] holds x W_ih^T + b_ih + b_hh of F0 on entry; every cell's ACTIVATED gates on exit of the forward,
//                           d(pre-activations) on exit of the backward
//   hbuf, cbuf (L+1, T+1, B, H)   block t + 1 of cell c: its state (after zoneout) at step t, so the fast state after every cell of every
//                           step and the slow state per step.  Block 0 of cells L-1 and L is the initial fast / slow state, written by the
//                           caller and left untouched; block 0 of the other cells is unused.
//   hd (2, T, B, H)         with dm: d1 . hbuf[0][t+1] and d2 . hbuf[L][t+1], the inputs of S and F1
//   mh, mc (L+1, T, B, H)   zoneout masks of h and c per cell and step, or NULL: the scalars keep_h / keep_c (a blend)
//   dm (2, T, B, H)         the dropout masks d1, d2 (already scaled by 1 / (1 - p)), or NULL: none
// Operands are staged through LDS in chunks of 32 k with 4-byte loads predicated on row, unit and k; nothing beyond 4-byte alignment is assumed.
#include "common.h"

namespace {

constexpr int KC = 32;         // k per staged chunk
constexpr int LDA = KC + 4;    // row pitch of a [row][k] LDS tile: 36 r + q (r < 16, q < 4) hits 64 different banks
constexpr int BM = 64;         // rows per workgroup: 4 waves x 16
constexpr int FWD_UN = 16;     // units per forward workgroup (x 4 gates = 64 rows of W)
constexpr int BWD_UN = 32;     // units per backward workgroup
constexpr int LDW = BWD_UN + 16;   // row pitch of the backward's [k][unit] W tile
constexpr int MAX_L = 64;

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

// acc[g] += a (rows b0 .., (B,H)) . w (rows g H + u0 .., (4H,H))^T over k < H
__device__ __forceinline__ void fwd_product(f32x4 (&acc)[4], const float* __restrict__ a, const float* __restrict__ w, int b0, int B, int u0, int H,
                                            float* As, float* Ws) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float av[8], wv[8];
  auto load_w = [&](int k0) {            // W tile row (gate g, unit u) = g * 16 + u: thread (row = tid / 32 + 8 i, k = tid % 32)
    const int k = k0 + (tid & 31), r = tid >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = r + 8 * i, u = u0 + (row & 15);
      wv[i] = (u < H && k < H) ? w[((long)(row >> 4) * H + u) * H + k] : 0.f;
    }
  };
  load_rows(av, a, H, b0, B, 0, H);
  load_w(0);
  const float* a_rd = As + (wave * 16 + (lane & 15)) * LDA + (lane >> 4);
  const float* w_rd = Ws + (lane & 15) * LDA + (lane >> 4);
  for (int k0 = 0; k0 < H; k0 += KC) {
    __syncthreads();                      // the previous chunk (or the previous product's last one) has been read
    store_rows(As, av);
    store_rows(Ws, wv);
    __syncthreads();
    if (k0 + KC < H) { load_rows(av, a, H, b0, B, k0 + KC, H); load_w(k0 + KC); }
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const float av4 = a_rd[ks * 4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av4, w_rd[g * FWD_UN * LDA + ks * 4], acc[g], 0, 0, 0);
    }
  }
}

// gates: `pre` on entry when has_pre (read and written by the same lane), the activated gates on exit
__global__ __launch_bounds__(256) void fsrnn_fwd_step(float* gates, int has_pre, const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                      const float* __restrict__ x, const float* __restrict__ w_ih, const float* __restrict__ h_prev,
                                                      const float* __restrict__ w_hh, const float* __restrict__ c_prev, const float* __restrict__ mh,
                                                      const float* __restrict__ mc, float keep_h, float keep_c, float* __restrict__ h_out,
                                                      float* __restrict__ c_out, const float* __restrict__ dmask, float* __restrict__ hd_out, int B, int H) {
  __shared__ float As[BM * LDA];
  __shared__ float Ws[4 * FWD_UN * LDA];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.x * FWD_UN, b0 = blockIdx.y * BM;
  const int unit = u0 + (lane & 15);
  const long H4 = 4L * H;

  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float bias = (!has_pre && unit < H) ? b_ih[g * H + unit] + b_hh[g * H + unit] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wave * 16 + (lane >> 4) * 4 + r;
      acc[g][r] = (has_pre && b < B && unit < H) ? gates[(long)b * H4 + (long)g * H + unit] : bias;
    }
  }
  if (x) fwd_product(acc, x, w_ih, b0, B, u0, H, As, Ws);
  fwd_product(acc, h_prev, w_hh, b0, B, u0, H, As, Ws);

  if (unit >= H) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + wave * 16 + (lane >> 4) * 4 + r;
    if (b >= B) continue;
    const float ig = sigmoidf_(acc[0][r]), fg = sigmoidf_(acc[1][r]), gg = tanhf_(acc[2][r]), og = sigmoidf_(acc[3][r]);
    const long e = (long)b * H + unit;
    const float cp = c_prev[e], hp = h_prev[e];
    const float cn = fg * cp + ig * gg;
    const float hn = og * tanhf_(cn);
    const float m_h = mh ? mh[e] : keep_h, m_c = mc ? mc[e] : keep_c;
    const float h = hn * m_h + (1.f - m_h) * hp;
    const float c = cn * m_c + (1.f - m_c) * cp;
    float* grow = gates + (long)b * H4 + unit;
    grow[0] = ig; grow[H] = fg; grow[2L * H] = gg; grow[3L * H] = og;
    c_out[e] = c;
    h_out[e] = h;
    if (dmask) hd_out[e] = h * dmask[e];
  }
}

// acc[s] += a (rows b0 .., (B,4H)) . w ((4H,H), columns u0 + 16 s ..) over k < 4H
__device__ __forceinline__ void bwd_product(f32x4 (&acc)[2], const float* __restrict__ a, const float* __restrict__ w, int b0, int B, int u0, int H,
                                            float* As, float* Ws) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = 4 * H;
  const long H4 = 4L * H;
  float av[8], wv[4];
  auto load_w = [&](int k0) {          // W rows k0 .. k0 + 31, columns u0 .. u0 + 31: thread (k = tid / 32 + 8 i, n = tid % 32)
    const int n = u0 + (tid & 31), k = k0 + (tid >> 5);
#pragma unroll
    for (int i = 0; i < 4; ++i) wv[i] = (k + 8 * i < K && n < H) ? w[(long)(k + 8 * i) * H + n] : 0.f;
  };
  load_rows(av, a, H4, b0, B, 0, K);
  load_w(0);
  const float* a_rd = As + (wave * 16 + (lane & 15)) * LDA + (lane >> 4);
  const float* w_rd = Ws + (lane >> 4) * LDW + (lane & 15);
  for (int k0 = 0; k0 < K; k0 += KC) {
    __syncthreads();
    store_rows(As, av);
#pragma unroll
    for (int i = 0; i < 4; ++i) Ws[((tid >> 5) + 8 * i) * LDW + (tid & 31)] = wv[i];
    __syncthreads();
    if (k0 + KC < K) { load_rows(av, a, H4, b0, B, k0 + KC, K); load_w(k0 + KC); }
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      const float av4 = a_rd[ks * 4];
#pragma unroll
      for (int s = 0; s < 2; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av4, w_rd[ks * 4 * LDW + s * 16], acc[s], 0, 0, 0);
    }
  }
}

// add_a / add_b / dc_in may be the buffers dhp_out / dcp_out point to: an element is read and written by the same lane.
__global__ __launch_bounds__(256) void fsrnn_bwd_step(const float* __restrict__ a1, const float* __restrict__ w1, const float* __restrict__ dmask,
                                                      const float* __restrict__ a2, const float* __restrict__ w2, const float* add_a, const float* add_b,
                                                      float* gates, const float* __restrict__ c_prev, const float* __restrict__ mh,
                                                      const float* __restrict__ mc, float keep_h, float keep_c, const float* dc_in, float* dhp_out,
                                                      float* dcp_out, float* dh_out, int B, int H) {
  __shared__ float As[BM * LDA];
  __shared__ float Ws[KC * LDW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.x * BWD_UN, b0 = blockIdx.y * BM;
  const long H4 = 4L * H;

  f32x4 acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s][r] = 0.f;
  if (a1) bwd_product(acc, a1, w1, b0, B, u0, H, As, Ws);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wave * 16 + (lane >> 4) * 4 + r, unit = u0 + s * 16 + (lane & 15);
      if (b < B && unit < H) {
        const long e = (long)b * H + unit;
        float v = acc[s][r];
        if (dmask) v *= dmask[e];
        if (add_a) v += add_a[e];
        if (add_b) v += add_b[e];
        acc[s][r] = v;
      }
    }
  if (a2) bwd_product(acc, a2, w2, b0, B, u0, H, As, Ws);

#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int unit = u0 + s * 16 + (lane & 15);
    if (unit >= H) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + wave * 16 + (lane >> 4) * 4 + r;
      if (b >= B) continue;
      const long e = (long)b * H + unit;
      const float dH = acc[s][r];
      if (!gates) { dh_out[e] = dH; continue; }
      const float m_h = mh ? mh[e] : keep_h, m_c = mc ? mc[e] : keep_c;
      const float dC = dc_in ? dc_in[e] : 0.f;
      const float dh = m_h * dH;
      float* grow = gates + (long)b * H4 + unit;
      const float ig = grow[0], fg = grow[H], gg = grow[2L * H], og = grow[3L * H];
      const float cp = c_prev[e];
      const float tc = tanhf_(fg * cp + ig * gg);
      const float dc = m_c * dC + dh * og * (1.f - tc * tc);
      grow[0] = dc * gg * ig * (1.f - ig);
      grow[H] = dc * cp * fg * (1.f - fg);
      grow[2L * H] = dc * ig * (1.f - gg * gg);
      grow[3L * H] = dh * tc * og * (1.f - og);
      dhp_out[e] = (1.f - m_h) * dH;
      dcp_out[e] = dc * fg + (1.f - m_c) * dC;
    }
  }
}

bool shape_ok(int T, int B, int H, int L) {
  return T >= 1 && B >= 1 && H >= 1 && L >= 2 && L <= MAX_L && (long)T * B * 4L * H < (1L << 31) && cdiv(B, BM) <= 65535;
}
size_t carry_bytes(int B, int H) { return ((size_t)B * H * sizeof(float) + 255) / 256 * 256; }
#define FSRNN_SHAPE_MSG "T, B, H must be >= 1, 2 <= L <= 64 and one cell's gates (T,B,4H) below 2^31 elements"

}  // namespace

extern "C" size_t re2e_fsrnn_workspace_bytes(int B, int H) { return B >= 1 && H >= 1 ? 4 * carry_bytes(B, H) : 0; }

extern "C" int re2e_fsrnn_plan(int T, int B, int H, int L, int backward, int cus, char* out, size_t out_bytes) {
  RE2E_CHECK_ARG(out && out_bytes > 0, "no output buffer");
  RE2E_CHECK_ARG(shape_ok(T, B, H, L), FSRNN_SHAPE_MSG);
  if (cus <= 0) cus = re2e_cu_count();
  const int un = backward ? BWD_UN : FWD_UN, gx = cdiv(H, un), gy = cdiv(B, BM);
  const int lds = (int)sizeof(float) * (BM * LDA + (backward ? KC * LDW : 4 * FWD_UN * LDA));
  // launches: one per cell and step (the backward adds one per initial h state the caller asks for: at most 2); rounds: workgroups per CU and launch
  const int n = snprintf(out, out_bytes, "family=%s mfma=16x16x4 rows=%d units=%d acc=%d kc=%d grid=%dx%dx1 lds=%d cells=%d launches=%d rounds=%d",
                         backward ? "fsrnn_bwd_step" : "fsrnn_fwd_step", BM, un, backward ? 2 : 4, KC, gx, gy, lds, L + 1, T * (L + 1),
                         cdiv((long)gx * gy, cus));
  RE2E_CHECK_ARG(n > 0 && (size_t)n < out_bytes, "output buffer too small");
  return RE2E_OK;
}

extern "C" int re2e_fsrnn_fwd(float* gates, float* hbuf, float* cbuf, float* hd, const float* const* w_ih, const float* const* w_hh,
                              const float* const* b_ih, const float* const* b_hh, const float* mh, const float* mc, const float* dm, float keep_h,
                              float keep_c, int T, int B, int H, int L, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)workspace; (void)workspace_bytes;          // the forward carries nothing between its launches but hbuf / cbuf
  RE2E_CHECK_ARG(gates && hbuf && cbuf && w_ih && w_hh && b_ih && b_hh, "null pointer");
  RE2E_CHECK_ARG(shape_ok(T, B, H, L), FSRNN_SHAPE_MSG);
  RE2E_CHECK_ARG((dm != nullptr) == (hd != nullptr), "dm and hd go together");
  RE2E_CHECK_ARG(w_ih[1] && w_ih[L], "the slow cell and fast cell 1 need w_ih");
  for (int c = 0; c <= L; ++c) RE2E_CHECK_ARG(w_hh[c] && (c == 0 || (b_ih[c] && b_hh[c])), "null weight or bias");
  const size_t BH = (size_t)B * H, TBH = BH * T, SB = BH * (T + 1);
  const dim3 grid(cdiv(H, FWD_UN), cdiv(B, BM));
  auto step = [&](int c, int t, bool pre, const float* x, const float* hp, const float* cp, const float* dmask, float* hd_out) {
    hipLaunchKernelGGL(fsrnn_fwd_step, grid, dim3(256), 0, stream, gates + 4 * (TBH * c + BH * t), pre ? 1 : 0, pre ? nullptr : b_ih[c],
                       pre ? nullptr : b_hh[c], x, x ? w_ih[c] : nullptr, hp, w_hh[c], cp, mh ? mh + TBH * c + BH * t : nullptr,
                       mc ? mc + TBH * c + BH * t : nullptr, keep_h, keep_c, hbuf + SB * c + BH * (t + 1), cbuf + SB * c + BH * (t + 1), dmask, hd_out, B, H);
  };
  for (int t = 0; t < T; ++t) {
    const size_t cur = BH * (t + 1), prev = BH * t;
    step(0, t, true, nullptr, hbuf + SB * (L - 1) + prev, cbuf + SB * (L - 1) + prev, dm ? dm + prev : nullptr, hd ? hd + prev : nullptr);
    RE2E_LAUNCH_CHECK();
    step(L, t, false, hd ? hd + prev : hbuf + cur, hbuf + SB * L + prev, cbuf + SB * L + prev, dm ? dm + TBH + prev : nullptr,
         hd ? hd + TBH + prev : nullptr);
    RE2E_LAUNCH_CHECK();
    for (int k = 1; k < L; ++k) {
      const float* x = k == 1 ? (hd ? hd + TBH + prev : hbuf + SB * L + cur) : nullptr;
      step(k, t, false, x, hbuf + SB * (k - 1) + cur, cbuf + SB * (k - 1) + cur, nullptr, nullptr);
      RE2E_LAUNCH_CHECK();
    }
  }
  return RE2E_OK;
}

extern "C" int re2e_fsrnn_bwd(float* gates, const float* cbuf, const float* const* w_ih, const float* const* w_hh, const float* mh, const float* mc,
                              const float* dm, float keep_h, float keep_c, const float* dy, const float* d_fh, const float* d_fc, const float* d_sh,
                              const float* d_sc, float* d_fh0, float* d_fc0, float* d_sh0, float* d_sc0, int T, int B, int H, int L, void* workspace,
                              size_t workspace_bytes, hipStream_t stream) {
  RE2E_CHECK_ARG(gates && cbuf && w_ih && w_hh && dy, "null pointer");
  RE2E_CHECK_ARG(shape_ok(T, B, H, L), FSRNN_SHAPE_MSG);
  RE2E_CHECK_ARG(workspace && workspace_bytes >= 4 * carry_bytes(B, H), "workspace smaller than re2e_fsrnn_workspace_bytes");
  RE2E_CHECK_ARG(w_ih[1] && w_ih[L], "the slow cell and fast cell 1 need w_ih");
  for (int c = 0; c <= L; ++c) RE2E_CHECK_ARG(w_hh[c], "null weight");
  const size_t BH = (size_t)B * H, TBH = BH * T, SB = BH * (T + 1), cf = carry_bytes(B, H) / sizeof(float);
  float* f_dhp = (float*)workspace;          // the pass-through (1 - m_h) . dH and the whole dC of the fast chain's / the slow cell's last launch
  float* f_dcp = f_dhp + cf;
  float* s_dhp = f_dhp + 2 * cf;
  float* s_dcp = f_dhp + 3 * cf;
  const dim3 grid(cdiv(H, BWD_UN), cdiv(B, BM));
  auto G = [&](int c, int t) { return gates + 4 * (TBH * c + BH * t); };
  auto step = [&](int c, int t, const float* a1, const float* w1, const float* dmask, const float* a2, const float* w2, const float* add_a,
                  const float* add_b, const float* cp, const float* dc_in, float* dhp_out, float* dcp_out) {
    hipLaunchKernelGGL(fsrnn_bwd_step, grid, dim3(256), 0, stream, a1, w1, dmask, a2, w2, add_a, add_b, G(c, t), cp,
                       mh ? mh + TBH * c + BH * t : nullptr, mc ? mc + TBH * c + BH * t : nullptr, keep_h, keep_c, dc_in, dhp_out, dcp_out,
                       (float*)nullptr, B, H);
  };
  const float* none = nullptr;
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    const size_t cur = BH * (t + 1), prev = BH * t;
    for (int k = L - 1; k >= 1; --k) {
      if (k == L - 1)          // consumers: the output of step t, F0 of step t + 1 (or the final state's gradient)
        step(k, t, none, none, none, last ? none : G(0, t + 1), w_hh[0], dy + prev, last ? d_fh : f_dhp, cbuf + SB * (k - 1) + cur, last ? d_fc : f_dcp,
             f_dhp, f_dcp);
      else                     // consumer: fast cell k + 1 (no input: the recurrent path only)
        step(k, t, none, none, none, G(k + 1, t), w_hh[k + 1], none, f_dhp, cbuf + SB * (k - 1) + cur, f_dcp, f_dhp, f_dcp);
      RE2E_LAUNCH_CHECK();
    }
    // the slow cell: F1's input through d2, its own next step
    step(L, t, G(1, t), w_ih[1], dm ? dm + TBH + prev : none, last ? none : G(L, t + 1), w_hh[L], none, last ? d_sh : s_dhp, cbuf + SB * L + prev,
         last ? d_sc : s_dcp, s_dhp, (t == 0 && d_sc0) ? d_sc0 : s_dcp);
    RE2E_LAUNCH_CHECK();
    // F0: the slow cell's input through d1, F1's recurrent path
    step(0, t, G(L, t), w_ih[L], dm ? dm + prev : none, G(1, t), w_hh[1], none, f_dhp, cbuf + SB * (L - 1) + prev, f_dcp, f_dhp,
         (t == 0 && d_fc0) ? d_fc0 : f_dcp);
    RE2E_LAUNCH_CHECK();
  }
  if (d_fh0) {
    hipLaunchKernelGGL(fsrnn_bwd_step, grid, dim3(256), 0, stream, none, none, none, (const float*)G(0, 0), w_hh[0], none, (const float*)f_dhp,
                       (float*)nullptr, none, none, none, 0.f, 0.f, none, (float*)nullptr, (float*)nullptr, d_fh0, B, H);
    RE2E_LAUNCH_CHECK();
  }
  if (d_sh0) {
    hipLaunchKernelGGL(fsrnn_bwd_step, grid, dim3(256), 0, stream, none, none, none, (const float*)G(L, 0), w_hh[L], none, (const float*)s_dhp,
                       (float*)nullptr, none, none, none, 0.f, 0.f, none, (float*)nullptr, (float*)nullptr, d_sh0, B, H);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}
