// K0 waveform front end: noise mixing at a drawn SNR and the 512-point STFT of the reference's offline data/prepare_feats.py
// (wav.read, MakeMixture, librosa.stft(n_fft=512, hop 256, scipy.signal.hamming)) on the device, from 16-bit PCM to the padded
// (B,Tmax,257) tensors the joint step reads.  No FFT library: one wavefront transforms one frame.
//
// re2e_wav_mix_scale: one workgroup per utterance sums s^2 and the noise segment's n^2 in double, a fixed stride per thread and a fixed
// tree over the threads, so the scale g is the same bits on every run.
//
// re2e_wav_stft: a workgroup of four wavefronts takes FRAMES = 8 consecutive frames of one utterance.  It stages the run of
// 256 * (FRAMES + 1) padded samples those frames share once per stream (reflect padding and the modular noise index are resolved here, int16
// -> fp32), then each wavefront transforms z = w s + i w g n with ONE 512-point complex FFT per frame: 512 = 8 x 8 x 8, every lane holds 8
// points and runs a radix-8 butterfly in registers, with two exchanges through LDS between the three passes.  Clean and noise spectra come
// apart by conjugate symmetry, C[k] = (Z[k] + conj Z[512-k]) / 2, gN[k] = (Z[k] - conj Z[512-k]) / 2i, and the mixture follows by linearity,
// M = C + gN.  The noise is scaled BEFORE the transform: the two halves of z leak into each other at fp32 rounding level, and a noise file is
// recorded at any level, while g n is at most the speech's power (SNR >= 0 dB) -- so the leak stays at rounding level of C, and silent speech
// under a loud file (g = 0) still gives C = 0 exactly.  The output rows are written 64 consecutive bins per wavefront store.
//
// re2e_wav_istft / re2e_wav_sdr_sums: the way back (enhanced magnitudes and a phase to samples) and the sums of SNR / SI-SDR, further down.
//
// LDS banking of the exchanges (8-byte elements; ds_read_b64 conflicts per 32-lane half over 64 dword banks):
//   pass 1 -> 2: element (k0, n1, n0) at 72 k0 + 8 n1 + n0.  Written lane-consecutive (lane = 8 n1 + n0); read by lane (k0, n0) for each n1:
//                a half wave covers k0 = 0..3, n0 = 0..7 -> 72 k0 + n0 is 0..7, 8..15, 16..23, 24..31 mod 32: conflict free.
//   pass 2 -> 3: element (k0, k1, n0) at 68 n0 + 8 k1 + k0.  Read lane-consecutive (lane = 8 k1 + k0) for each n0; written by lane (k0, n0)
//                for each k1: 68 n0 + k0 is 4 n0 + k0 mod 32, distinct over the half wave.
#include "common.h"

#include <math.h>

namespace {

constexpr int NFFT = 512, HOP = 256, NBIN = 257;
constexpr int FRAMES = 8;                        // frames per workgroup (two per wavefront)
constexpr int RUN = HOP * (FRAMES + 1);          // staged samples per stream
constexpr int CHUNK = 32;                        // utterances per launch: their index rows travel as a kernel argument
constexpr float FLOOR = 1e-7f;

struct WavUtt {                                  // read-only kernel argument (uniform index: scalar loads, nothing is copied)
  long soff[CHUNK], slen[CHUNK], noff[CHUNK], nlen[CHUNK], s0[CHUNK];
};
struct WavUttRev : WavUtt {                      // re2e_wav_stft_rev: the mixture's own speech stream
  long moff[CHUNK];
};
template <bool REV> struct UttOf { typedef WavUtt type; };
template <> struct UttOf<true> { typedef WavUttRev type; };
struct WavRatio {
  double r[CHUNK];                               // 10^(dB/10), taken in double on the host
};
struct WavOut {
  float *clean, *clean_log, *mix, *mix_log, *cos, *clean_ang, *mix_ang;
};

__device__ float g_wav_window[NFFT];             // 0.54 - 0.46 cos(2 pi n / 511): built on the host in double, rounded to fp32
__device__ float2 g_wav_twiddle[NFFT];           // exp(-2 pi i k / 512), likewise

// Y[k] = sum_j x[j] exp(-2 pi i j k / 8), natural order in and out, in registers (decimation in frequency: 8 -> 2 x 4)
__device__ __forceinline__ void fft8(float (&re)[8], float (&im)[8]) {
  constexpr float C8 = 0.70710678118654752440f;
  float ar[8], ai[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ar[j] = re[j] + re[j + 4]; ai[j] = im[j] + im[j + 4];
    ar[j + 4] = re[j] - re[j + 4]; ai[j + 4] = im[j] - im[j + 4];
  }
  float tr, ti;
  tr = C8 * (ar[5] + ai[5]); ti = C8 * (ai[5] - ar[5]); ar[5] = tr; ai[5] = ti;          // * exp(-i pi/4)
  tr = ai[6]; ti = -ar[6]; ar[6] = tr; ai[6] = ti;                                       // * -i
  tr = C8 * (ai[7] - ar[7]); ti = -C8 * (ar[7] + ai[7]); ar[7] = tr; ai[7] = ti;         // * exp(-3i pi/4)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = 4 * h;
    const float b0r = ar[a] + ar[a + 2], b0i = ai[a] + ai[a + 2], b2r = ar[a] - ar[a + 2], b2i = ai[a] - ai[a + 2];
    const float b1r = ar[a + 1] + ar[a + 3], b1i = ai[a + 1] + ai[a + 3];
    const float b3r = ai[a + 1] - ai[a + 3], b3i = -(ar[a + 1] - ar[a + 3]);             // -i (a1 - a3)
    re[h] = b0r + b1r; im[h] = b0i + b1i;
    re[h + 4] = b0r - b1r; im[h + 4] = b0i - b1i;
    re[h + 2] = b2r + b3r; im[h + 2] = b2i + b3i;
    re[h + 6] = b2r - b3r; im[h + 6] = b2i - b3i;
  }
}

__device__ __forceinline__ void zero_rows(float* p, long first, int n, int tid) {
  if (!p) return;
  for (int i = tid; i < n; i += 256) p[first + i] = 0.f;
}

// REV (re2e_wav_stft_rev; needs NOISE): the imaginary half of z is w (rs + g n), rs = pcm[moff ..) the mixture's own (reverberant) speech,
// and M is that half's spectrum itself; C stays the spectrum of the dry s.
template <bool NOISE, bool REV = false>
__global__ __launch_bounds__(256) void wav_stft_kernel(const short* __restrict__ pcm, const typename UttOf<REV>::type u, const float* __restrict__ scale,
                                                       int b0, int Tmax, const WavOut o, const float* __restrict__ cmvn) {
  __shared__ float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float xs[RUN];
  __shared__ float xn[NOISE ? RUN : 1];
  __shared__ float2 xbuf[4][576];
  const int bi = blockIdx.y, b = b0 + bi, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long L = u.slen[bi];
  const int T = 1 + (int)(L >> 8);
  const int t0 = blockIdx.x * FRAMES;
  const long row0 = (long)b * Tmax;
  if (t0 >= T) {                                 // padding only: rows t0 .. of this utterance are zero in every output
    const int n = (min(t0 + FRAMES, Tmax) - t0) * NBIN;
    const long first = (row0 + t0) * NBIN;
    zero_rows(o.clean, first, n, tid); zero_rows(o.clean_log, first, n, tid); zero_rows(o.mix, first, n, tid);
    zero_rows(o.mix_log, first, n, tid); zero_rows(o.cos, first, n, tid); zero_rows(o.clean_ang, first, n, tid);
    zero_rows(o.mix_ang, first, n, tid);
    return;
  }
  for (int i = tid; i < NFFT; i += 256) { win[i] = g_wav_window[i]; tw[i] = g_wav_twiddle[i]; }
  const float g = NOISE ? scale[b] : 0.f;
  {
    const short* sp = pcm + u.soff[bi];
    const short* np = NOISE ? pcm + u.noff[bi] : nullptr;
    const short* mp = nullptr;
    if constexpr (REV) mp = pcm + u.moff[bi];
    const unsigned N = NOISE ? (unsigned)u.nlen[bi] : 1u, s0 = NOISE ? (unsigned)u.s0[bi] : 0u;
    const long first = (long)HOP * (t0 - 1);
    for (int j = tid; j < RUN; j += 256) {
      const long i = first + j;
      const long r = i < 0 ? -i : (i >= L ? 2 * (L - 1) - i : i);          // reflect (librosa center=True)
      const bool in = r >= 0 && r < L;                                     // false only under frames >= T, which are not transformed
      xs[j] = in ? (float)sp[r] : 0.f;
      if (NOISE && !REV) xn[j] = in ? g * (float)np[(s0 + (unsigned)r) % N] : 0.f; // s0 + r < 2^32
      if (REV) xn[j] = in ? (float)mp[r] + g * (float)np[(s0 + (unsigned)r) % N] : 0.f;
    }
  }
  __syncthreads();
  float2* zb = xbuf[wave];
  const int n0 = lane & 7, k0 = lane >> 3;
#pragma unroll 1
  for (int f = wave; f < FRAMES; f += 4) {         // every wavefront makes the same two trips: the barriers below are uniform
    const int t = t0 + f;
    float re[8], im[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float w = win[lane + 64 * j];
      re[j] = w * xs[HOP * f + lane + 64 * j];
      im[j] = NOISE ? w * xn[HOP * f + lane + 64 * j] : 0.f;
    }
    fft8(re, im);                                  // over n2 -> k0
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 c = tw[k * lane];
      const float r = re[k] * c.x - im[k] * c.y, i = re[k] * c.y + im[k] * c.x;
      re[k] = r; im[k] = i;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) zb[72 * k + lane] = make_float2(re[k], im[k]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 v = zb[72 * k0 + 8 * j + n0]; re[j] = v.x; im[j] = v.y; }
    __syncthreads();
    fft8(re, im);                                  // over n1 -> k1
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 c = tw[8 * n0 * k];
      const float r = re[k] * c.x - im[k] * c.y, i = re[k] * c.y + im[k] * c.x;
      re[k] = r; im[k] = i;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) zb[68 * n0 + 8 * k + k0] = make_float2(re[k], im[k]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 v = zb[68 * j + lane]; re[j] = v.x; im[j] = v.y; }
    __syncthreads();
    fft8(re, im);                                  // over n0 -> k2: Z[lane + 64 k2]
#pragma unroll
    for (int k = 0; k < 8; ++k) zb[lane + 64 * k] = make_float2(re[k], im[k]);
    __syncthreads();
    if (t < Tmax) {
      const bool live = t < T;
      const long row = (row0 + t) * NBIN;
#pragma unroll 1
      for (int k = lane; k < NBIN; k += 64) {
        float v_clean = 0.f, v_clog = 0.f, v_mix = 0.f, v_mlog = 0.f, v_cos = 0.f, v_cang = 0.f, v_mang = 0.f;
        if (live) {
          const float m0 = cmvn ? cmvn[k] : 0.f, m1 = cmvn ? cmvn[NBIN + k] : 1.f;
          const float2 zk = zb[k], zm = zb[(NFFT - k) & (NFFT - 1)];
          const bool real_bin = (k & (HOP - 1)) == 0;                      // k = 0 and 256: the spectrum of a real signal is real there
          float cr, ci, nr = 0.f, ni = 0.f;
          if (NOISE) {
            cr = 0.5f * (zk.x + zm.x); ci = 0.5f * (zk.y - zm.y);
            nr = 0.5f * (zk.y + zm.y); ni = -0.5f * (zk.x - zm.x);
          } else {
            cr = zk.x; ci = zk.y;
          }
          if (real_bin) { ci = 0.f; ni = 0.f; }
          if (!REV && g == 0.f) { nr = 0.f; ni = 0.f; }                       // no noise (zero-power segment): M is C bit for bit
          const float cm = sqrtf(cr * cr + ci * ci);
          v_clean = cm < FLOOR ? FLOOR : cm;
          v_clog = (10.f * log10f(v_clean) + m0) * m1;
          v_cang = atan2f(ci, cr);
          if (NOISE) {
            const float mr = REV ? nr : cr + nr, mi = REV ? ni : ci + ni;
            const float mm = sqrtf(mr * mr + mi * mi);
            v_mix = mm < FLOOR ? FLOOR : mm;
            v_mlog = (10.f * log10f(v_mix) + m0) * m1;
            v_mang = atan2f(mi, mr);
            // cos(angle C - angle M) = Re(C conj M) / (|C| |M|); a zero magnitude counts as angle 0 (np.angle)
            const float ucr = cm > 0.f ? cr / cm : 1.f, uci = cm > 0.f ? ci / cm : 0.f;
            const float umr = mm > 0.f ? mr / mm : 1.f, umi = mm > 0.f ? mi / mm : 0.f;
            v_cos = fminf(1.f, fmaxf(-1.f, ucr * umr + uci * umi));
          }
        }
        if (o.clean) o.clean[row + k] = v_clean;
        if (o.clean_log) o.clean_log[row + k] = v_clog;
        if (o.clean_ang) o.clean_ang[row + k] = v_cang;
        if (NOISE) {
          if (o.mix) o.mix[row + k] = v_mix;
          if (o.mix_log) o.mix_log[row + k] = v_mlog;
          if (o.cos) o.cos[row + k] = v_cos;
          if (o.mix_ang) o.mix_ang[row + k] = v_mang;
        }
      }
    }
    __syncthreads();                               // zb is written again on the next trip
  }
}

__global__ __launch_bounds__(256) void wav_mix_scale_kernel(const short* __restrict__ pcm, const WavUtt u, const WavRatio ratio, int b0,
                                                            float* __restrict__ scale_out, int* __restrict__ zero_count) {
  __shared__ double red_s[256], red_n[256];
  const int bi = blockIdx.x, tid = threadIdx.x;
  const long L = u.slen[bi];
  const short* sp = pcm + u.soff[bi];
  const short* np = pcm + u.noff[bi];
  const unsigned N = (unsigned)u.nlen[bi], step = 256u % N;
  unsigned idx = ((unsigned)u.s0[bi] + (unsigned)tid) % N;             // (s0 + i) mod N, carried from i to i + 256
  double es = 0.0, pn = 0.0;
  for (long i = tid; i < L; i += 256) {
    const double s = (double)sp[i], n = (double)np[idx];
    es += s * s;
    pn += n * n;
    idx += step;
    if (idx >= N) idx -= N;
  }
  red_s[tid] = es; red_n[tid] = pn;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) { red_s[tid] += red_s[tid + h]; red_n[tid] += red_n[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double p = red_n[0];
    float g = 0.f;
    if (p > 0.0) g = (float)sqrt(red_s[0] / (p * ratio.r[bi]));
    else if (zero_count) atomicAdd(zero_count, 1);
    scale_out[b0 + bi] = g;
  }
}

// The two tables, once per device and process (synchronous, on first use).
int ensure_tables() {
  static std::mutex m;
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  std::lock_guard<std::mutex> lock(m);
  if (done[dev]) return 0;
  static float win[NFFT];
  static float2 tw[NFFT];
  const double pi = 3.14159265358979323846;
  for (int n = 0; n < NFFT; ++n) {
    win[n] = (float)(0.54 - 0.46 * cos(2.0 * pi * n / (NFFT - 1)));
    tw[n] = make_float2((float)cos(2.0 * pi * n / NFFT), (float)-sin(2.0 * pi * n / NFFT));
  }
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wav_window), win, sizeof(win)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wav_twiddle), tw, sizeof(tw)) != hipSuccess) return -1;
  done[dev] = true;
  return 0;
}

constexpr long LMAX = 2147483647L;               // lengths stay below 2^31

// nullptr, or what is wrong with utterance b
const char* check_utt(const long* soff, const long* slen, const long* noff, const long* nlen, const long* s0, int b) {
  if (soff[b] < 0) return "negative speech offset";
  if (slen[b] < NBIN) return "an utterance is shorter than 257 samples (reflect padding needs 257)";
  if (slen[b] > LMAX) return "an utterance has 2^31 samples or more";
  if (noff) {
    if (noff[b] < 0) return "negative noise offset";
    if (nlen[b] < 1 || nlen[b] > LMAX) return "noise length outside 1 .. 2^31 - 1";
    if (s0[b] < 0 || s0[b] >= nlen[b]) return "noise_start outside its noise file";
  }
  return nullptr;
}

void fill_chunk(WavUtt& u, const long* soff, const long* slen, const long* noff, const long* nlen, const long* s0, int b0, int nb) {
  for (int i = 0; i < CHUNK; ++i) {
    const int b = b0 + (i < nb ? i : 0);
    u.soff[i] = soff[b]; u.slen[i] = slen[b];
    u.noff[i] = noff ? noff[b] : 0; u.nlen[i] = noff ? nlen[b] : 1; u.s0[i] = noff ? s0[b] : 0;
  }
}

// ---- the way back: re2e_wav_istft ---------------------------------------------------------------------------------------------------------
// With hop = NFFT / 2 every kept sample lies under exactly two frames: hop block h (samples 256 h .. 256 h + 255) is the second half of
// frame h plus the first half of frame h + 1, over w^2 of the two halves -- a gather, no atomics.  A workgroup owns IBLOCKS = 15 consecutive
// hop blocks and transforms the IFRAMES = 16 frames under them (the first frame of the next group is transformed again there: 1/15 more
// work, no wait on another workgroup).  Two real frames share one complex transform, the mirror image of the forward's packing:
// Z = Xa + i Xb over the Hermitian-extended spectra gives xa + i xb.  The inverse runs on the forward's butterflies and twiddles as
// conj(FFT(conj Z)) / 512.  The imaginary parts of bins 0 and 256 are dropped BEFORE packing (kept, Im Xa[0] would land in xb).
// The spectrum of a pair is staged in the wavefront's exchange buffer in natural order (bin k and its mirror 512 - k written by the lane
// that read bin k: lane-consecutive, conflict free), the windowed frames go to fr[frame][n] (lane-consecutive), and sample m of every block
// belongs to thread m, which keeps 1 / (512 (w[m]^2 + w[m + 256]^2)) in a register.  Rows t >= T_b are never read.
constexpr int IFRAMES = 16, IBLOCKS = IFRAMES - 1;

struct IstftUtt {                                // read-only kernel argument, as WavUtt
  long off[CHUNK], len[CHUNK];
};

__global__ __launch_bounds__(256) void wav_istft_kernel(const float* __restrict__ mag, const float* __restrict__ ang, const IstftUtt u, int b0,
                                                        int Tmax, float* __restrict__ wav, short* __restrict__ pcm, int* __restrict__ clip_count) {
  __shared__ float win[NFFT];
  __shared__ float2 tw[NFFT];
  __shared__ float2 xbuf[4][576];
  __shared__ float fr[IFRAMES][NFFT];
  const int bi = blockIdx.y, b = b0 + bi, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long L = u.len[bi];
  const int T = 1 + (int)(L >> 8);
  const int h0 = blockIdx.x * IBLOCKS;           // first hop block = first frame of this workgroup
  if (h0 >= T) return;                           // blocks 0 .. T - 2 carry samples, block T - 1 is the zero tail
  for (int i = tid; i < NFFT; i += 256) { win[i] = g_wav_window[i]; tw[i] = g_wav_twiddle[i]; }
  __syncthreads();
  const long row0 = (long)b * Tmax;
  float2* zb = xbuf[wave];
  const int n0 = lane & 7, k0 = lane >> 3;
#pragma unroll 1
  for (int q = wave; q < IFRAMES / 2; q += 4) {    // every wavefront makes the same two trips: the barriers below are uniform
    const int ta = h0 + 2 * q, tb = ta + 1;
    const bool live_a = ta < T, live_b = tb < T;   // an odd T leaves a lone frame; frames >= T are zero and their rows are not read
    const long rowa = (row0 + ta) * NBIN, rowb = (row0 + tb) * NBIN;
#pragma unroll 1
    for (int k = lane; k < NBIN; k += 64) {
      float ar = 0.f, ai = 0.f, br = 0.f, bim = 0.f;
      if (live_a) { float s, c; const float m = mag[rowa + k]; sincosf(ang[rowa + k], &s, &c); ar = m * c; ai = m * s; }
      if (live_b) { float s, c; const float m = mag[rowb + k]; sincosf(ang[rowb + k], &s, &c); br = m * c; bim = m * s; }
      if ((k & (HOP - 1)) == 0) { ai = 0.f; bim = 0.f; }                    // k = 0 and 256: the spectrum of a real frame is real there
      zb[k] = make_float2(ar - bim, -(ai + br));                           // conj Z[k], Z[k] = Xa[k] + i Xb[k]
      if (k > 0 && k < HOP) zb[NFFT - k] = make_float2(ar + bim, ai - br); // conj Z[512 - k], Z[512 - k] = conj Xa[k] + i conj Xb[k]
    }
    __syncthreads();
    float re[8], im[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 v = zb[lane + 64 * j]; re[j] = v.x; im[j] = v.y; }
    __syncthreads();
    fft8(re, im);
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 c = tw[k * lane];
      const float r = re[k] * c.x - im[k] * c.y, i = re[k] * c.y + im[k] * c.x;
      re[k] = r; im[k] = i;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) zb[72 * k + lane] = make_float2(re[k], im[k]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 v = zb[72 * k0 + 8 * j + n0]; re[j] = v.x; im[j] = v.y; }
    __syncthreads();
    fft8(re, im);
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 c = tw[8 * n0 * k];
      const float r = re[k] * c.x - im[k] * c.y, i = re[k] * c.y + im[k] * c.x;
      re[k] = r; im[k] = i;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) zb[68 * n0 + 8 * k + k0] = make_float2(re[k], im[k]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float2 v = zb[68 * j + lane]; re[j] = v.x; im[j] = v.y; }
    fft8(re, im);                                  // 512 (xa - i xb)[lane + 64 k]
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float w = win[lane + 64 * k];
      fr[2 * q][lane + 64 * k] = w * re[k];
      fr[2 * q + 1][lane + 64 * k] = -(w * im[k]);
    }
    __syncthreads();                               // zb is written again on the next trip; after the last one fr is complete
  }
  const float w0 = win[tid], w1 = win[tid + HOP];
  const float inv = 1.f / ((float)NFFT * (w0 * w0 + w1 * w1));
  const long base = u.off[bi];
  int clipped = 0;
#pragma unroll 1
  for (int g = 0; g < IBLOCKS; ++g) {
    const int h = h0 + g;
    if (h >= T) break;
    const long i = (long)HOP * h + tid;
    float v = 0.f;
    if (h < T - 1) v = (fr[g][HOP + tid] + fr[g + 1][tid]) * inv;
    else if (i >= L) break;                        // the tail 256 (T - 1) .. L is zero (librosa's length padding); nothing beyond L
    if (wav) wav[base + i] = v;
    if (pcm) {
      const float r = rintf(v);
      if (r > 32767.f || r < -32768.f) ++clipped;
      pcm[base + i] = (short)fminf(32767.f, fmaxf(-32768.f, r));
    }
  }
  if (pcm && clip_count) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) clipped += __shfl_xor(clipped, o, 64);
    if (lane == 0 && clipped > 0) atomicAdd(clip_count, clipped);
  }
}

// re2e_wav_sdr_sums: one workgroup per utterance, each thread a fixed run of indices into three double sums, then a fixed tree (as
// wav_mix_scale_kernel): the same bits on every run.  1024 threads and SDR_UNROLL loads of each stream in flight per thread: the sums are
// bound by the latency of the loads, not by the arithmetic.
constexpr int SDR_THREADS = 1024, SDR_UNROLL = 4;          // a workgroup's stride is SDR_THREADS * SDR_UNROLL samples

struct SdrUtt {
  long roff[CHUNK], eoff[CHUNK], len[CHUNK];
};

__global__ __launch_bounds__(SDR_THREADS) void wav_sdr_sums_kernel(const short* __restrict__ ref, const float* __restrict__ est, const SdrUtt u,
                                                                   int b0, double* __restrict__ sums) {
  __shared__ double red[3][SDR_THREADS];
  const int bi = blockIdx.x, tid = threadIdx.x;
  const long n = u.len[bi];
  const short* sp = ref + u.roff[bi];
  const float* yp = est + u.eoff[bi];
  double ss = 0.0, yy = 0.0, sy = 0.0;
  for (long i0 = tid; i0 < n; i0 += SDR_THREADS * SDR_UNROLL) {
    short sv[SDR_UNROLL];
    float yv[SDR_UNROLL];
#pragma unroll
    for (int j = 0; j < SDR_UNROLL; ++j) {         // the loads of a trip first, then its sums in index order
      const long i = i0 + SDR_THREADS * j;
      const bool in = i < n;
      sv[j] = in ? sp[i] : (short)0;
      yv[j] = in ? yp[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < SDR_UNROLL; ++j) {         // an index beyond n adds exact zeros
      const double s = (double)sv[j], y = (double)yv[j];
      ss += s * s; yy += y * y; sy += s * y;
    }
  }
  red[0][tid] = ss; red[1][tid] = yy; red[2][tid] = sy;
  __syncthreads();
  for (int h = SDR_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) { red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; red[2][tid] += red[2][tid + h]; }
    __syncthreads();
  }
  if (tid < 3) sums[3 * (long)(b0 + bi) + tid] = red[tid][0];
}

}  // namespace

extern "C" int re2e_wav_mix_scale(const short* pcm, const long* speech_off, const long* speech_len, const long* noise_off,
                                  const long* noise_len, const long* noise_start, const float* snr_db, int B, float* scale_out,
                                  int* zero_count, hipStream_t stream) {
  RE2E_CHECK_ARG(pcm && speech_off && speech_len && noise_off && noise_len && noise_start && snr_db && scale_out, "null operand");
  RE2E_CHECK_ARG(B > 0, "bad shape");
  for (int b = 0; b < B; ++b) {
    const char* why = check_utt(speech_off, speech_len, noise_off, noise_len, noise_start, b);
    RE2E_CHECK_ARG(!why, why);
    RE2E_CHECK_ARG(snr_db[b] == snr_db[b] && fabsf(snr_db[b]) <= 200.f, "snr_db outside -200 .. 200 dB");
  }
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
    WavUtt u;
    WavRatio r;
    fill_chunk(u, speech_off, speech_len, noise_off, noise_len, noise_start, b0, nb);
    for (int i = 0; i < CHUNK; ++i) r.r[i] = pow(10.0, (double)snr_db[b0 + (i < nb ? i : 0)] / 10.0);
    hipLaunchKernelGGL(wav_mix_scale_kernel, dim3(nb), dim3(256), 0, stream, pcm, u, r, b0, scale_out, zero_count);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}

extern "C" int re2e_wav_stft(const short* pcm, const long* speech_off, const long* speech_len, const long* noise_off, const long* noise_len,
                             const long* noise_start, const float* scale, int B, int Tmax, float* clean, float* clean_log, float* mix,
                             float* mix_log, float* cos_out, float* clean_ang, float* mix_ang, const float* cmvn, hipStream_t stream) {
  RE2E_CHECK_ARG(pcm && speech_off && speech_len, "null operand");
  RE2E_CHECK_ARG(B > 0 && Tmax > 0, "bad shape");
  if (noise_off) {
    RE2E_CHECK_ARG(noise_len && noise_start, "noise_off without noise_len / noise_start");
    RE2E_CHECK_ARG(scale, "noise without a scale (re2e_wav_mix_scale writes it)");
  } else {
    RE2E_CHECK_ARG(!mix && !mix_log && !cos_out && !mix_ang, "a mixture output without noise (noise_off is NULL: only the clean stream exists)");
  }
  for (int b = 0; b < B; ++b) {
    const char* why = check_utt(speech_off, speech_len, noise_off, noise_len, noise_start, b);
    RE2E_CHECK_ARG(!why, why);
    RE2E_CHECK_ARG(1 + speech_len[b] / HOP <= Tmax, "Tmax is below an utterance's frame count 1 + L / 256");
  }
  if (ensure_tables() != 0) {
    re2e_set_error("%s: could not upload the window and twiddle tables", __func__);
    return RE2E_EHIP;
  }
  const WavOut o = {clean, clean_log, mix, mix_log, cos_out, clean_ang, mix_ang};
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
    WavUtt u;
    fill_chunk(u, speech_off, speech_len, noise_off, noise_len, noise_start, b0, nb);
    const dim3 grid(cdiv(Tmax, FRAMES), nb);
    if (noise_off) hipLaunchKernelGGL(wav_stft_kernel<true>, grid, dim3(256), 0, stream, pcm, u, scale, b0, Tmax, o, cmvn);
    else hipLaunchKernelGGL(wav_stft_kernel<false>, grid, dim3(256), 0, stream, pcm, u, scale, b0, Tmax, o, cmvn);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}

extern "C" int re2e_wav_stft_rev(const short* pcm, const long* speech_off, const long* mix_off, const long* speech_len, const long* noise_off,
                                 const long* noise_len, const long* noise_start, const float* scale, int B, int Tmax, float* clean,
                                 float* clean_log, float* mix, float* mix_log, float* cos_out, float* clean_ang, float* mix_ang, const float* cmvn,
                                 hipStream_t stream) {
  if (!mix_off)
    return re2e_wav_stft(pcm, speech_off, speech_len, noise_off, noise_len, noise_start, scale, B, Tmax, clean, clean_log, mix, mix_log, cos_out,
                         clean_ang, mix_ang, cmvn, stream);
  RE2E_CHECK_ARG(pcm && speech_off && speech_len, "null operand");
  RE2E_CHECK_ARG(B > 0 && Tmax > 0, "bad shape");
  RE2E_CHECK_ARG(noise_off && noise_len && noise_start, "mix_off without noise (noise_off / noise_len / noise_start)");
  RE2E_CHECK_ARG(scale, "noise without a scale (re2e_wav_mix_scale writes it)");
  for (int b = 0; b < B; ++b) {
    const char* why = check_utt(speech_off, speech_len, noise_off, noise_len, noise_start, b);
    RE2E_CHECK_ARG(!why, why);
    RE2E_CHECK_ARG(mix_off[b] >= 0, "negative mixture offset");
    RE2E_CHECK_ARG(1 + speech_len[b] / HOP <= Tmax, "Tmax is below an utterance's frame count 1 + L / 256");
  }
  if (ensure_tables() != 0) {
    re2e_set_error("%s: could not upload the window and twiddle tables", __func__);
    return RE2E_EHIP;
  }
  const WavOut o = {clean, clean_log, mix, mix_log, cos_out, clean_ang, mix_ang};
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
    WavUttRev u;
    fill_chunk(u, speech_off, speech_len, noise_off, noise_len, noise_start, b0, nb);
    for (int i = 0; i < CHUNK; ++i) u.moff[i] = mix_off[b0 + (i < nb ? i : 0)];
    hipLaunchKernelGGL((wav_stft_kernel<true, true>), dim3(cdiv(Tmax, FRAMES), nb), dim3(256), 0, stream, pcm, u, scale, b0, Tmax, o, cmvn);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}

extern "C" int re2e_wav_istft(const float* mag, const float* ang, const long* out_off, const long* out_len, int B, int Tmax, long out_samples,
                              float* wav_f32, short* pcm_out, int* clip_count, hipStream_t stream) {
  RE2E_CHECK_ARG(mag && ang, "null operand (mag and ang are both needed)");
  RE2E_CHECK_ARG(out_off && out_len, "null operand");
  RE2E_CHECK_ARG(wav_f32 || pcm_out, "no output: wav_f32 and pcm_out are both NULL");
  RE2E_CHECK_ARG(B > 0 && Tmax > 0 && out_samples > 0, "bad shape");
  for (int b = 0; b < B; ++b) {
    RE2E_CHECK_ARG(out_len[b] >= NBIN, "an utterance is shorter than 257 samples (the forward's reflect padding needs 257)");
    RE2E_CHECK_ARG(out_len[b] <= LMAX, "an utterance has 2^31 samples or more");
    RE2E_CHECK_ARG(1 + out_len[b] / HOP <= Tmax, "Tmax is below an utterance's frame count 1 + L / 256");
    RE2E_CHECK_ARG(out_off[b] >= 0 && out_off[b] <= out_samples - out_len[b], "an output offset outside its range 0 .. out_samples - L");
  }
  if (ensure_tables() != 0) {
    re2e_set_error("%s: could not upload the window and twiddle tables", __func__);
    return RE2E_EHIP;
  }
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
    IstftUtt u;
    int Tlong = 0;                               // the longest utterance of the chunk sizes the grid
    for (int i = 0; i < CHUNK; ++i) {
      const int b = b0 + (i < nb ? i : 0);
      u.off[i] = out_off[b]; u.len[i] = out_len[b];
      const int T = 1 + (int)(out_len[b] / HOP);
      if (T > Tlong) Tlong = T;
    }
    hipLaunchKernelGGL(wav_istft_kernel, dim3(cdiv(Tlong, IBLOCKS), nb), dim3(256), 0, stream, mag, ang, u, b0, Tmax, wav_f32, pcm_out, clip_count);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}

extern "C" int re2e_wav_sdr_sums(const short* ref_pcm, const long* ref_off, const float* est, const long* est_off, const long* len, int B,
                                 double* sums, hipStream_t stream) {
  RE2E_CHECK_ARG(ref_pcm && ref_off && est && est_off && len && sums, "null operand");
  RE2E_CHECK_ARG(B > 0, "bad shape");
  for (int b = 0; b < B; ++b) {
    RE2E_CHECK_ARG(ref_off[b] >= 0 && est_off[b] >= 0, "negative offset");
    RE2E_CHECK_ARG(len[b] >= 1 && len[b] <= LMAX, "length outside 1 .. 2^31 - 1");
  }
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
    SdrUtt u;
    for (int i = 0; i < CHUNK; ++i) {
      const int b = b0 + (i < nb ? i : 0);
      u.roff[i] = ref_off[b]; u.eoff[i] = est_off[b]; u.len[i] = len[b];
    }
    hipLaunchKernelGGL(wav_sdr_sums_kernel, dim3(nb), dim3(SDR_THREADS), 0, stream, ref_pcm, est, u, b0, sums);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}
