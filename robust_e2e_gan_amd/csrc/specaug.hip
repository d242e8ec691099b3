// SpecAugment on the normalised filterbank features: re2e_spec_augment_fwd / _bwd (include/re2e.h states the contract).  A time warp per
// utterance over its own valid frames (two segments, each resized along time as torch's bicubic interpolate with align_corners=False
// resizes it), then frequency and time masks; the padding passes through.  8 MB at (32, 800, 80): a vector kernel of a single wave of workgroups,
// measured launch-bound on a tensor small enough to stay in the caches (6 / 11 us beside 4 us for a copy, profiles/spec_augment.md).
//
// One description per FRAME.  What an output frame t reads -- four clamped source frames and their cubic-convolution weights, or one frame
// to copy, or nothing (a time mask) -- does not depend on the feature lane: sa_desc works it out once per frame, in integers up to the one
// fp32 division that gives the fractional position, and the workgroup keeps the descriptions of its frames in LDS.  The forward kernel
// (SA_FT output frames of one row per workgroup) gathers y[t] = sum_k wt[k] x[idx[k]]; the backward kernel (SA_BT SOURCE frames per
// workgroup) is a gather as well: source frame s sums wt[k] dy[t] over the contiguous run of output frames t whose clamped taps hit it
// (sa_range inverts i0(t) in integers), in ascending t and tap order -- no atomics, two runs agree bit for bit.  The backward workgroup
// stages the descriptions of the SA_CH output frames from the first one its tile reads; a segment stretches by less than 2 within the
// contract, so that covers the tile, and an output frame beyond the staged window (only a plan outside the contract has one) is described
// on the spot by the same function.
//
// Every plan value is clamped where it is read (sa_row, sa_desc, the staged frequency masks): no plan can index outside row r of x / y.
// Rows are float4 where F % 4 == 0 and both pointers are 16-byte aligned, scalar otherwise; the host chooses from the call's own operands.
#include "common.h"

namespace {

constexpr int SA_FT = 32;                                  // forward: output frames per workgroup
constexpr int SA_BT = 32;                                  // backward: source frames per workgroup
constexpr int SA_CH = 2 * SA_BT + 16;                      // backward: staged output-frame descriptions
constexpr int SA_MAXM = RE2E_SPECAUG_MAX_MASKS;
constexpr float SA_A = -0.75f;                             // the cubic convolution's A

enum { SA_PAD = 0, SA_ZERO = 1, SA_COPY = 2, SA_WARP = 3 };  // padding frame (copied, unmasked); time-masked; one valid frame; four taps

struct SaRow { int T, c, w; };                             // clamped: 0 <= T <= Tp; c == 0 (no warp) or 1 <= c, w <= T - 1
struct SaDesc { int idx[4]; float wt[4]; int kind; };      // absolute source frames of the row and their weights

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ SaRow sa_row(const int* __restrict__ p, int Tp) {
  SaRow r;
  r.T = clampi(p[0], 0, Tp);
  int c = p[1], w = p[2];
  if (c <= 0 || r.T < 2) { c = 0; w = 0; }
  else { c = c < r.T - 1 ? c : r.T - 1; w = clampi(w, 1, r.T - 1); }
  r.c = c; r.w = w;
  return r;
}

__device__ __forceinline__ long floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }      // b > 0

__device__ __forceinline__ SaDesc sa_desc(const int* __restrict__ p, const SaRow r, int nF, int nT, int t) {
  SaDesc d;
  d.idx[0] = d.idx[1] = d.idx[2] = d.idx[3] = t;
  d.wt[0] = 1.f; d.wt[1] = d.wt[2] = d.wt[3] = 0.f;
  d.kind = SA_PAD;
  if (t >= r.T) return d;
  for (int k = 0; k < nT; ++k) {
    const int t0 = clampi(p[3 + 2 * nF + 2 * k], 0, r.T), tl = clampi(p[4 + 2 * nF + 2 * k], 0, r.T - t0);
    if (t >= t0 && t < t0 + tl) { d.kind = SA_ZERO; return d; }
  }
  d.kind = SA_COPY;
  if (r.c == 0) return d;
  int n_in, n_out, base, tt;
  if (t < r.w) { n_in = r.c; n_out = r.w; base = 0; tt = t; }
  else { n_in = r.T - r.c; n_out = r.T - r.w; base = r.c; tt = t - r.w; }
  if (n_in == n_out) { d.idx[0] = d.idx[1] = d.idx[2] = d.idx[3] = base + tt; return d; }
  const long N = (2L * tt + 1) * n_in - n_out, D = 2L * n_out;
  const long i0 = floor_div(N, D);
  const float tau = (float)(N - i0 * D) / (float)D;        // both below 2^24: exact operands, one division
  const float x0 = tau + 1.f, x3 = (1.f - tau) + 1.f, x2 = 1.f - tau;
  d.wt[0] = ((SA_A * x0 - 5.f * SA_A) * x0 + 8.f * SA_A) * x0 - 4.f * SA_A;
  d.wt[1] = ((SA_A + 2.f) * tau - (SA_A + 3.f)) * tau * tau + 1.f;
  d.wt[2] = ((SA_A + 2.f) * x2 - (SA_A + 3.f)) * x2 * x2 + 1.f;
  d.wt[3] = ((SA_A * x3 - 5.f * SA_A) * x3 + 8.f * SA_A) * x3 - 4.f * SA_A;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long i = i0 - 1 + k;
    d.idx[k] = base + (int)(i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i));
  }
  d.kind = SA_WARP;
  return d;
}

// First output frame tt of a segment (n_in -> n_out) with i0(tt) >= a:  (2 tt + 1) n_in >= (2 a + 1) n_out, clamped to 0 .. n_out.
__device__ __forceinline__ int sa_first(long a, int n_in, int n_out) {
  const long Q = (2 * a + 1) * (long)n_out;
  const long q = -floor_div(-Q, n_in);                     // ceil(Q / n_in): 2 tt + 1 >= q
  const long tt = floor_div(q, 2);
  return (int)(tt < 0 ? 0 : (tt > n_out ? n_out : tt));
}

// The output frames [lo, hi) whose clamped taps can hit source frame s of the row.
__device__ __forceinline__ void sa_range(const SaRow r, int s, int& lo, int& hi) {
  lo = s; hi = s + 1;
  if (s >= r.T || r.c == 0) return;
  int n_in, n_out, base, obase;
  if (s < r.c) { n_in = r.c; n_out = r.w; base = 0; obase = 0; }
  else { n_in = r.T - r.c; n_out = r.T - r.w; base = r.c; obase = r.w; }
  const int j = s - base;
  if (n_in == n_out) { lo = obase + j; hi = lo + 1; return; }
  lo = obase + (j == 0 ? 0 : sa_first((long)j - 2, n_in, n_out));                 // taps i0 - 1 .. i0 + 2: j - 2 <= i0 <= j + 1,
  hi = obase + (j == n_in - 1 ? n_out : sa_first((long)j + 2, n_in, n_out));      // the ends of a segment collect the clamped taps
}

template <int VEC> struct SaV { float e[VEC]; };
template <int VEC> __device__ __forceinline__ SaV<VEC> sa_ld(const float* __restrict__ p) {
  SaV<VEC> r;
  if constexpr (VEC == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    r.e[0] = q.x; r.e[1] = q.y; r.e[2] = q.z; r.e[3] = q.w;
  } else {
    r.e[0] = *p;
  }
  return r;
}
template <int VEC> __device__ __forceinline__ void sa_st(float* __restrict__ p, const SaV<VEC>& v) {
  if constexpr (VEC == 4) {
    f32x4 q; q.x = v.e[0]; q.y = v.e[1]; q.z = v.e[2]; q.w = v.e[3];
    *reinterpret_cast<f32x4*>(p) = q;
  } else {
    *p = v.e[0];
  }
}

// The clamped frequency masks of the row as [first, end) pairs, by the lanes 64 .. 64 + nF of the workgroup.
__device__ __forceinline__ void sa_stage_fmasks(const int* __restrict__ p, int nF, int F, int* fm) {
  const int k = (int)threadIdx.x - 64;
  if (k >= 0 && k < nF) {
    const int f0 = clampi(p[3 + 2 * k], 0, F), fl = clampi(p[4 + 2 * k], 0, F - f0);
    fm[2 * k] = f0; fm[2 * k + 1] = f0 + fl;
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void sa_fwd_kernel(const float* __restrict__ x, const int* __restrict__ plan, int P, int Tp, int F, int nF, int nT,
                                                     int tiles, float* __restrict__ y) {
  __shared__ SaDesc ds[SA_FT];
  __shared__ int fm[2 * SA_MAXM];
  const int tid = threadIdx.x;
  const int row = blockIdx.x / tiles, t0 = (blockIdx.x - row * tiles) * SA_FT;
  const int nfr = Tp - t0 < SA_FT ? Tp - t0 : SA_FT;
  const int* p = plan + (long)row * P;
  const SaRow r = sa_row(p, Tp);
  if (tid < nfr) ds[tid] = sa_desc(p, r, nF, nT, t0 + tid);
  sa_stage_fmasks(p, nF, F, fm);
  __syncthreads();
  const int FV = F / VEC;
  const float* xr = x + (long)row * Tp * F;
  float* yr = y + ((long)row * Tp + t0) * F;
  for (int i = tid; i < nfr * FV; i += 256) {
    const int fr = i / FV, f = (i - fr * FV) * VEC;
    const int kind = ds[fr].kind;
    SaV<VEC> v;
    if (kind == SA_ZERO) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) v.e[e] = 0.f;
    } else if (kind != SA_WARP) {
      v = sa_ld<VEC>(xr + (long)ds[fr].idx[0] * F + f);
    } else {
      const SaV<VEC> a0 = sa_ld<VEC>(xr + (long)ds[fr].idx[0] * F + f), a1 = sa_ld<VEC>(xr + (long)ds[fr].idx[1] * F + f),
                     a2 = sa_ld<VEC>(xr + (long)ds[fr].idx[2] * F + f), a3 = sa_ld<VEC>(xr + (long)ds[fr].idx[3] * F + f);
      const float w0 = ds[fr].wt[0], w1 = ds[fr].wt[1], w2 = ds[fr].wt[2], w3 = ds[fr].wt[3];
#pragma unroll
      for (int e = 0; e < VEC; ++e)                          // explicit: the float4 and the scalar form round alike
        v.e[e] = fmaf(a3.e[e], w3, fmaf(a2.e[e], w2, fmaf(a1.e[e], w1, a0.e[e] * w0)));
    }
    if (kind >= SA_COPY) {
      for (int k = 0; k < nF; ++k) {
        const int fa = fm[2 * k], fb = fm[2 * k + 1];
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (f + e >= fa && f + e < fb) v.e[e] = 0.f;
      }
    }
    sa_st<VEC>(yr + (long)fr * F + f, v);
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void sa_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ plan, int P, int Tp, int F, int nF, int nT,
                                                     int tiles, float* __restrict__ dx) {
  __shared__ SaDesc ds[SA_CH];
  __shared__ int fm[2 * SA_MAXM];
  __shared__ int rng[2 * SA_BT];
  const int tid = threadIdx.x;
  const int row = blockIdx.x / tiles, s0 = (blockIdx.x - row * tiles) * SA_BT;
  const int ns = Tp - s0 < SA_BT ? Tp - s0 : SA_BT;
  const int* p = plan + (long)row * P;
  const SaRow r = sa_row(p, Tp);
  const int FV = F / VEC;
  const float* gr = dy + (long)row * Tp * F;
  float* dr = dx + ((long)row * Tp + s0) * F;
  if (s0 >= r.T) {                                         // a tile wholly in the padding (uniform over the workgroup): a copy, nothing staged
    for (int i = tid; i < ns * FV; i += 256) sa_st<VEC>(dr + (long)i * VEC, sa_ld<VEC>(gr + (long)s0 * F + (long)i * VEC));
    return;
  }
  int U0, hi0;
  sa_range(r, s0, U0, hi0);                                // the ranges ascend with s: the tile's first output frame
  if (tid < ns) {
    int lo, hi;
    sa_range(r, s0 + tid, lo, hi);
    rng[2 * tid] = lo; rng[2 * tid + 1] = hi;
  }
  for (int i = tid; i < SA_CH && U0 + i < Tp; i += 256) ds[i] = sa_desc(p, r, nF, nT, U0 + i);
  sa_stage_fmasks(p, nF, F, fm);
  __syncthreads();
  for (int i = tid; i < ns * FV; i += 256) {
    const int fr = i / FV, f = (i - fr * FV) * VEC, s = s0 + fr;
    SaV<VEC> acc;
    if (s >= r.T) {
      acc = sa_ld<VEC>(gr + (long)s * F + f);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc.e[e] = 0.f;
      const int lo = rng[2 * fr], hi = rng[2 * fr + 1];
      for (int t = lo; t < hi; ++t) {
        const unsigned u = (unsigned)(t - U0);
        int kind; float ws = 0.f;
        if (u < (unsigned)SA_CH) {
          kind = ds[u].kind;
#pragma unroll
          for (int k = 0; k < 4; ++k) ws += ds[u].idx[k] == s ? ds[u].wt[k] : 0.f;
        } else {                                           // beyond the staged window: only a plan outside the contract gets here
          const SaDesc d = sa_desc(p, r, nF, nT, t);
          kind = d.kind;
#pragma unroll
          for (int k = 0; k < 4; ++k) ws += d.idx[k] == s ? d.wt[k] : 0.f;
        }
        if (kind < SA_COPY) continue;                      // a time-masked output frame contributes nothing
        const SaV<VEC> g = sa_ld<VEC>(gr + (long)t * F + f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.e[e] = fmaf(ws, g.e[e], acc.e[e]);
      }
      for (int k = 0; k < nF; ++k) {                       // nor does a frequency-masked cell
        const int fa = fm[2 * k], fb = fm[2 * k + 1];
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (f + e >= fa && f + e < fb) acc.e[e] = 0.f;
      }
    }
    sa_st<VEC>(dr + (long)fr * F + f, acc);
  }
}

bool sa_vec4(const float* a, const float* b, int F) {
  return F % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}

}  // namespace

extern "C" int re2e_spec_augment_geometry(int which) {
  switch (which) {
    case 0: return SA_FT;
    case 1: return SA_BT;
    case 2: return SA_MAXM;
    case 3: return SA_CH;
    default: return -1;
  }
}

#define SA_CHECK_COMMON(in, out, same_msg)                                                                                     \
  RE2E_CHECK_ARG(in && plan && out, "null operand");                                                                           \
  RE2E_CHECK_ARG(in != out, same_msg);                                                                                         \
  RE2E_CHECK_ARG(R >= 1 && Tp >= 1 && F >= 1, "bad shape (a non-positive size)");                                              \
  RE2E_CHECK_ARG(nF >= 0 && nT >= 0 && nF <= SA_MAXM && nT <= SA_MAXM, "nF or nT outside 0 .. RE2E_SPECAUG_MAX_MASKS");        \
  RE2E_CHECK_ARG((reinterpret_cast<uintptr_t>(in) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&                  \
                 (reinterpret_cast<uintptr_t>(plan) & 3) == 0, "an operand is not aligned to its element size")

extern "C" int re2e_spec_augment_fwd(const float* x, const int* plan, int R, int Tp, int F, int nF, int nT, float* y, hipStream_t stream) {
  SA_CHECK_COMMON(x, y, "x == y: in place is not offered (a warped frame reads frames that would already be overwritten)");
  const int tiles = cdiv(Tp, SA_FT);
  RE2E_CHECK_ARG((long)R * tiles <= 2147483647L, "bad shape (more than 2^31 - 1 workgroups)");
  const int P = 3 + 2 * nF + 2 * nT;
  if (sa_vec4(x, y, F)) hipLaunchKernelGGL(sa_fwd_kernel<4>, dim3(R * tiles), dim3(256), 0, stream, x, plan, P, Tp, F, nF, nT, tiles, y);
  else hipLaunchKernelGGL(sa_fwd_kernel<1>, dim3(R * tiles), dim3(256), 0, stream, x, plan, P, Tp, F, nF, nT, tiles, y);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}

extern "C" int re2e_spec_augment_bwd(const float* dy, const int* plan, int R, int Tp, int F, int nF, int nT, float* dx, hipStream_t stream) {
  SA_CHECK_COMMON(dy, dx, "dy == dx: in place is not offered (a source frame sums output frames that would already be overwritten)");
  const int tiles = cdiv(Tp, SA_BT);
  RE2E_CHECK_ARG((long)R * tiles <= 2147483647L, "bad shape (more than 2^31 - 1 workgroups)");
  const int P = 3 + 2 * nF + 2 * nT;
  if (sa_vec4(dy, dx, F)) hipLaunchKernelGGL(sa_bwd_kernel<4>, dim3(R * tiles), dim3(256), 0, stream, dy, plan, P, Tp, F, nF, nT, tiles, dx);
  else hipLaunchKernelGGL(sa_bwd_kernel<1>, dim3(R * tiles), dim3(256), 0, stream, dy, plan, P, Tp, F, nF, nT, tiles, dx);
  RE2E_LAUNCH_CHECK();
  return RE2E_OK;
}
