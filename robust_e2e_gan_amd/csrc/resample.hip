// K0 speed perturbation: re2e_wav_resample, scipy.signal.resample_poly(x, up, down) with its defaults for a batch of independent jobs
// (include/re2e.h states the definition).  About 2 half / up + 1 = 21 taps per output at the Kaldi speeds (10/9, 10/11): a bandwidth-bound
// vector kernel, no matrix instruction.
//
// Polyphase form.  Output m reads the table at half + m down - j up.  With a = half + m down, jm = a / up and phi = a mod up these are
// the indices phi + t up, t = 0, 1, .., against x[jm - t]: ONE phase of the table, walked upwards, against the signal walked downwards.
// The device table of a ratio is laid out by phase, T[phi][t] = h[phi + t up] for t < NT (zero where phi + t up > 2 half), with
// NT = ceil((2 half + 1) / up) made ODD: every output then takes exactly NT steps in ascending tap order (the steps beyond its last tap add
// exact zeros), the summation order is fixed by construction, and two runs agree bit for bit.
//
// Shape.  A workgroup of 256 lanes owns RS_G = 1024 consecutive outputs of one job.  It stages the job's table once (float4 loads), then
// walks its outputs in sub-tiles of S outputs, S <= RS_G the most whose input span fits the staged run (S = RS_G unless down / up is above about 9; the
// host computes it): the int16 span x[jlo .. jhi] the sub-tile reads goes to LDS as it is, in 4-byte words from an EVEN sample address
// (the run starts one sample early when soff + jlo is odd, so an odd src_off costs nothing; a word with a sample outside 0 .. L - 1 falls back
// to two guarded 2-byte loads and zero fill: nothing outside the source range is ever read, and the tap loop has no conditions).
// A lane takes PAIRS of adjacent outputs, the pair aligned to an even destination address: one 4-byte store of two int16, one 8-byte
// store of two floats where the address allows, single stores at a sub-tile's ragged ends.
//
// LDS banks.  Lanes of a wavefront hold different phases; phase phi starts at word phi NT, and NT odd makes phi -> phi NT mod 64 a
// bijection for the up <= 64 phases there are: lanes of different phases read different banks at every step, lanes of one phase the same
// word (a broadcast).  The signal reads of adjacent lanes are 2 down / up samples apart, 4 bytes at the speeds near 1: consecutive banks.
// 18.5 KB + 5.5 KB of LDS: six workgroups per CU.
//
// The int16 output is saturate(rintf(.)) of the very register the fp32 output stores (re2e_wav_istft's rule).
#include "common.h"

#include <map>
#include <math.h>
#include <utility>
#include <vector>

namespace {

constexpr int RS_G = 1024;                                 // outputs per workgroup
constexpr int RS_CHUNK = 32;                               // jobs per launch: their index rows travel as a kernel argument
constexpr int RS_XS = 9472;                                // staged samples (int16)
constexpr int RS_HS = 1408;                                // staged table floats: up NT <= 20 R + 1 + 2 up - 1
constexpr int RS_SMIN = 64;                                // S is a multiple of it
constexpr long RS_LMAX = 2147483647L;

static_assert(RS_G % RS_SMIN == 0 && RS_SMIN % 2 == 0, "sub-tiles are whole pairs");
static_assert(RS_XS % 2 == 0 && RS_HS % 4 == 0, "word / float4 staging");
static_assert(20 * RE2E_WAV_RESAMPLE_MAX_RATE + 2 * RE2E_WAV_RESAMPLE_MAX_RATE <= RS_HS, "the widest table fits");
static_assert(RS_XS * 2 + RS_HS * 4 <= 65536, "static LDS");

struct RsJobs {                                            // read-only kernel argument (uniform index: scalar loads)
  long soff[RS_CHUNK], slen[RS_CHUNK], first[RS_CHUNK], count[RS_CHUNK], doff[RS_CHUNK];
  const float* tab[RS_CHUNK];
  int up[RS_CHUNK], down[RS_CHUNK], nt[RS_CHUNK], sub[RS_CHUNK];
};

// Samples a sub-tile of S outputs stages at most: NT below the first output's newest sample, one for the even start, and the newest
// sample of the last output, (phi0 + (S - 1) down) / up with phi0 <= up - 1, rounded up to a whole word.
inline long rs_span(int S, int up, int down, int nt) { return ((long)nt + 1 + ((long)(up - 1) + (long)(S - 1) * down) / up + 1 + 1) & ~1L; }

__global__ __launch_bounds__(256) void wav_resample_kernel(const short* __restrict__ pcm, const RsJobs u, float* wav, short* out,
                                                           int* __restrict__ clip_count) {
  __shared__ __attribute__((aligned(16))) short xs[RS_XS];
  __shared__ __attribute__((aligned(16))) float hs[RS_HS];
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const long count = u.count[q];
  const long i0 = (long)blockIdx.x * RS_G;
  if (i0 >= count) return;
  const int up = u.up[q], down = u.down[q], nt = u.nt[q], S = u.sub[q];
  const int half = 10 * (up > down ? up : down);
  const long slen = u.slen[q];
  const short* sp = pcm + u.soff[q];
  const long base = u.doff[q];
  const int n_out = count - i0 < RS_G ? (int)(count - i0) : RS_G;
  {                                                        // the job's table, already laid out by phase and padded to whole float4
    const f32x4* tp = reinterpret_cast<const f32x4*>(u.tab[q]);
    f32x4* hp = reinterpret_cast<f32x4*>(hs);
    const int n4 = (up * nt + 3) >> 2;
    for (int i = tid; i < n4; i += 256) hp[i] = tp[i];
  }
  int clipped = 0;
#pragma unroll 1
  for (int o0 = 0; o0 < n_out; o0 += S) {
    const int ns = n_out - o0 < S ? n_out - o0 : S;
    const long a0 = (long)half + (u.first[q] + i0 + o0) * (long)down;     // output o of the sub-tile: a = a0 + o down
    const long jm0 = a0 / up;
    const int phi0 = (int)(a0 - jm0 * up);
    const long jlo0 = jm0 - (nt - 1);
    const int sh = (int)(((long)(reinterpret_cast<uintptr_t>(sp) >> 1) + jlo0) & 1);   // start the run at an even sample address
    const long jlo = jlo0 - sh;                                            // xs position p holds x[jlo + p]
    const int span = nt + sh + (phi0 + (ns - 1) * down) / up;              // positions read: 0 .. span - 1 (<= rs_span(S) <= RS_XS)
    if (o0 > 0) __syncthreads();                                           // the run is staged again: the last sub-tile's reads are done
    for (int w = tid; 2 * w < span; w += 256) {
      const long j = jlo + 2 * w;
      unsigned v;
      if (j >= 0 && j + 1 < slen) {
        v = *reinterpret_cast<const unsigned*>(sp + j);
      } else {
        const unsigned lo = j >= 0 && j < slen ? (unsigned short)sp[j] : 0u;
        const unsigned hi = j + 1 >= 0 && j + 1 < slen ? (unsigned short)sp[j + 1] : 0u;
        v = lo | (hi << 16);
      }
      reinterpret_cast<unsigned*>(xs)[w] = v;
    }
    __syncthreads();
    // pairs at even destination addresses: pair w holds the outputs 2 w - par and 2 w - par + 1 of the sub-tile
    const long d0 = base + i0 + o0;
    const int par = out ? (int)((reinterpret_cast<uintptr_t>(out + d0) >> 1) & 1) : (int)((reinterpret_cast<uintptr_t>(wav + d0) >> 2) & 1);
    for (int w = tid; 2 * w - par < ns; w += 256) {
      float y[2] = {0.f, 0.f};
      bool live[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int o = 2 * w - par + e;
        live[e] = o >= 0 && o < ns;
        if (live[e]) {
          const int local = phi0 + o * down;
          const int dq = local / up;
          const float* hr = hs + (local - dq * up) * nt;
          const short* xr = xs + (nt - 1 + sh + dq);
          float acc = 0.f;
          for (int t = 0; t < nt; ++t) acc = fmaf(hr[t], (float)xr[-t], acc);
          y[e] = acc;
        }
      }
      const long d = d0 + 2 * w - par;                                     // destination of the pair's first output
      if (wav) {
        if (live[0] && live[1] && (reinterpret_cast<uintptr_t>(wav + d) & 7) == 0) {
          *reinterpret_cast<float2*>(wav + d) = make_float2(y[0], y[1]);
        } else {
          if (live[0]) wav[d] = y[0];
          if (live[1]) wav[d + 1] = y[1];
        }
      }
      if (out) {
        short s[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float rv = rintf(y[e]);
          if (live[e] && (rv > 32767.f || rv < -32768.f)) ++clipped;
          s[e] = (short)fminf(32767.f, fmaxf(-32768.f, rv));
        }
        if (live[0] && live[1] && (reinterpret_cast<uintptr_t>(out + d) & 3) == 0) {
          *reinterpret_cast<unsigned*>(out + d) = (unsigned)(unsigned short)s[0] | ((unsigned)(unsigned short)s[1] << 16);
        } else {
          if (live[0]) out[d] = s[0];
          if (live[1]) out[d + 1] = s[1];
        }
      }
    }
  }
  if (out && clip_count) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) clipped += __shfl_xor(clipped, o, 64);
    if (lane == 0 && clipped > 0) atomicAdd(clip_count, clipped);
  }
}

// ---- the table: built on the host in double, rounded once to fp32, kept per (up, down) -------------------------------------------------------------
double bessel_i0(double x) {                               // power series sum_k ((x / 2)^k / k!)^2
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

struct RsTable {
  int half = 0, nt = 0;
  std::vector<float> h;                                    // h[0 .. 2 half], include/re2e.h's definition
  std::map<int, float*> dev;                               // per device: T[phi][t], up rows of nt floats, padded to whole float4
};

std::mutex rs_mutex;
std::map<std::pair<int, int>, RsTable> rs_tables;

const char* rs_ratio_error(int up, int down) {
  if (up < 1 || down < 1) return "up < 1 or down < 1";
  if (up == down) return "up == down: a speed of exactly 1 is not a job (the samples pass through untouched)";
  if ((up > down ? up : down) > RE2E_WAV_RESAMPLE_MAX_RATE) return "max(up, down) > RE2E_WAV_RESAMPLE_MAX_RATE";
  int a = up, b = down;
  while (b) { const int t = a % b; a = b; b = t; }
  if (a != 1) return "gcd(up, down) != 1: give the ratio in lowest terms";
  return nullptr;
}

// The table of a checked ratio; dev_out: its phase layout on the current device as well (allocated and copied once per process and
// device, with a blocking copy: later calls on any stream find it complete).  nullptr: the device refused.
const RsTable* rs_table(int up, int down, const float** dev_out) {
  std::lock_guard<std::mutex> g(rs_mutex);
  RsTable& t = rs_tables[std::make_pair(up, down)];
  if (t.h.empty()) {
    const int R = up > down ? up : down, half = 10 * R, n = 2 * half + 1;
    const double pi = 3.14159265358979323846, fc = 1.0 / R, i0b = bessel_i0(5.0);
    std::vector<double> gd(n);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
      // sinc's argument is rounded as numpy.sinc rounds it, pi * (fc * d): at the zero crossings (d a multiple of R) the value of the sine IS
      // the rounding residue of that argument, 1e-17 of the peak, and an output that reads such a tap alone (a unit impulse) is compared to
      // float64 RELATIVE to it
      const double d = (double)(i - half), r = d / half, x = pi * (fc * d);
      const double sinc = i == half ? 1.0 : sin(x) / x;
      const double rr = 1.0 - r * r;
      gd[i] = fc * sinc * bessel_i0(5.0 * sqrt(rr > 0.0 ? rr : 0.0)) / i0b;
      sum += gd[i];
    }
    t.half = half;
    t.nt = ((n + up - 1) / up) | 1;
    t.h.resize(n);
    for (int i = 0; i < n; ++i) t.h[i] = (float)((double)up * gd[i] / sum);
  }
  int device = 0;
  if (dev_out && hipGetDevice(&device) != hipSuccess) return nullptr;
  if (dev_out && !t.dev.count(device)) {
    const int n = 2 * t.half + 1, floats = (up * t.nt + 3) / 4 * 4;
    if (floats > RS_HS) return nullptr;                    // (cannot happen: static_assert above)
    std::vector<float> lay(floats, 0.f);
    for (int phi = 0; phi < up; ++phi)
      for (int k = 0; k < t.nt; ++k)
        if (phi + k * up < n) lay[phi * t.nt + k] = t.h[phi + k * up];
    float* d = nullptr;
    if (hipMalloc(&d, floats * sizeof(float)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, lay.data(), floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return nullptr;
    }
    t.dev[device] = d;
  }
  if (dev_out) *dev_out = t.dev[device];
  return &t;
}

}  // namespace

extern "C" int re2e_wav_resample_geometry(int which) {
  switch (which) {
    case 0: return RS_G;
    case 1: return RS_CHUNK;
    case 2: return RE2E_WAV_RESAMPLE_MAX_RATE;
    default: return -1;
  }
}

extern "C" int re2e_wav_resample_taps(int up, int down, float* h_host, int* half) {
  const char* bad = rs_ratio_error(up, down);
  RE2E_CHECK_ARG(!bad, bad);
  RE2E_CHECK_ARG(h_host || half, "no output: h_host and half are both NULL");
  const RsTable* t = rs_table(up, down, nullptr);
  if (half) *half = t->half;
  if (h_host) memcpy(h_host, t->h.data(), t->h.size() * sizeof(float));
  return RE2E_OK;
}

extern "C" int re2e_wav_resample(const short* pcm, long pcm_samples, const long* src_off, const long* src_len, const int* up, const int* down,
                                 const long* first, const long* count, const long* dst_off, int n_jobs, long out_samples, float* wav_f32,
                                 short* pcm_out, int* clip_count, hipStream_t stream) {
  RE2E_CHECK_ARG(pcm && src_off && src_len && up && down && first && count && dst_off, "null operand");
  RE2E_CHECK_ARG(wav_f32 || pcm_out, "no output: wav_f32 and pcm_out are both NULL");
  RE2E_CHECK_ARG(n_jobs >= 1, "bad shape (n_jobs < 1)");
  RE2E_CHECK_ARG(pcm_samples > 0 && out_samples > 0, "bad shape");
  RE2E_CHECK_ARG((reinterpret_cast<uintptr_t>(pcm) & 1) == 0 && (reinterpret_cast<uintptr_t>(pcm_out) & 1) == 0 &&
                 (reinterpret_cast<uintptr_t>(wav_f32) & 3) == 0, "an operand is not aligned to its element size");
  for (int q = 0; q < n_jobs; ++q) {
    const char* bad = rs_ratio_error(up[q], down[q]);
    RE2E_CHECK_ARG(!bad, bad);
    RE2E_CHECK_ARG(src_len[q] >= 1 && src_len[q] <= RS_LMAX, "a source length outside 1 .. 2^31 - 1");
    RE2E_CHECK_ARG(src_off[q] >= 0 && src_off[q] <= pcm_samples - src_len[q], "a source range outside 0 .. pcm_samples");
    const long lout = (src_len[q] * up[q] + down[q] - 1) / down[q];       // L' = ceil(L up / down)
    RE2E_CHECK_ARG(first[q] >= 0 && count[q] >= 1, "first < 0 or count < 1");
    RE2E_CHECK_ARG(first[q] <= lout && count[q] <= lout - first[q], "first + count beyond the resampled length ceil(src_len up / down)");
    RE2E_CHECK_ARG(dst_off[q] >= 0 && dst_off[q] <= out_samples - count[q], "a destination range outside 0 .. out_samples");
  }
  if (pcm_out == pcm) {                          // in place: the resampled signals land behind the uploaded samples of the same blob
    RE2E_CHECK_ARG(out_samples <= pcm_samples, "in place (pcm_out is pcm): out_samples beyond pcm_samples");
    for (int q = 0; q < n_jobs; ++q)
      for (int s = 0; s < n_jobs; ++s)
        RE2E_CHECK_ARG(dst_off[q] + count[q] <= src_off[s] || src_off[s] + src_len[s] <= dst_off[q],
                       "in place (pcm_out is pcm): a destination range overlaps a source range of the same call");
  }
  std::vector<const RsTable*> tabs(n_jobs);
  std::vector<const float*> dtab(n_jobs);
  std::vector<int> subs(n_jobs);
  for (int q = 0; q < n_jobs; ++q) {             // every table is on the device, every sub-tile chosen, before the first launch
    tabs[q] = rs_table(up[q], down[q], &dtab[q]);
    if (!tabs[q]) {
      re2e_set_error("%s: the table of %d/%d could not be placed on the device: %s", __func__, up[q], down[q], hipGetErrorString(hipGetLastError()));
      return RE2E_EHIP;
    }
    int S = RS_G;
    while (S > RS_SMIN && rs_span(S, up[q], down[q], tabs[q]->nt) > RS_XS) S -= RS_SMIN;
    RE2E_CHECK_ARG(rs_span(S, up[q], down[q], tabs[q]->nt) <= RS_XS, "the input span of a ratio does not fit the staged run");   // (not below MAX_RATE)
    subs[q] = S;
  }
  for (int q0 = 0; q0 < n_jobs; q0 += RS_CHUNK) {
    const int nq = n_jobs - q0 < RS_CHUNK ? n_jobs - q0 : RS_CHUNK;
    RsJobs u;
    long longest = 0;                            // the longest job of the chunk sizes the grid
    for (int i = 0; i < RS_CHUNK; ++i) {
      const int q = q0 + (i < nq ? i : 0);
      u.soff[i] = src_off[q]; u.slen[i] = src_len[q]; u.first[i] = first[q]; u.count[i] = count[q]; u.doff[i] = dst_off[q];
      u.tab[i] = dtab[q]; u.up[i] = up[q]; u.down[i] = down[q]; u.nt[i] = tabs[q]->nt; u.sub[i] = subs[q];
      if (count[q] > longest) longest = count[q];
    }
    hipLaunchKernelGGL(wav_resample_kernel, dim3(cdiv(longest, RS_G), nq), dim3(256), 0, stream, pcm, u, wav_f32, pcm_out, clip_count);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}
