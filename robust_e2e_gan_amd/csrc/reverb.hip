// K0 reverberation: re2e_wav_reverb, the truncated convolution np.convolve(h, x)[:len(x)] of the reference's Make_Reverberation
// (data/audioparse.py:254-303) for a batch of independent jobs, on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32.
//
// Toeplitz product.  A tile is 32 x 32 consecutive outputs starting at i0, Y[r][c] = y[i0 + 32 r + c].  With j = k - c,
//   Y[r][c] = sum_j A[r][j] B[j][c],   A[r][j] = x[i0 + 32 r - j],   B[j][c] = h[j + c],   -32 <= j < K
// (h is zero outside 0 .. K - 1, x before sample 0; j = -32 adds exact zeros and keeps the count of steps even): K + 32 contraction steps
// for 1024 outputs.  Both operands are plain 1-D runs in LDS, and a lane reads ONE float of each per instruction (A: row r = lane & 31,
// B: column c = lane & 31, both at j + (lane >> 5)).
//
// Shape.  A workgroup of RV_WAVES = 4 wavefronts owns RV_OT = 4096 consecutive outputs of one job, a wavefront RV_TILES = 1 tile (the
// instruction's issue interval equals its dependent latency, so one accumulator keeps the matrix stream full; two tiles per wavefront
// save tap reads, which are free, and were 16 % slower at B = 32 x 12.8 s: 800 workgroups of twice the work on 768 resident slots leave
// a tail -- DESIGN.md Appendix A).  The taps are walked in K-tiles of RV_KT = 2048: K-tile 0 takes j = -32 .. RV_KT - 1, K-tile t > 0
// takes j = t RV_KT .. (t + 1) RV_KT - 1, each cut at K and rounded up to RV_STEP = 16 steps (eight instructions per trip).  Per K-tile
// the workgroup stages, once, the tap run h[jlo .. jend + 31] (shared by its four wavefronts) and the signal run
// x[i0 - jend + 1 .. i0 + RV_OT - jlo] that its tiles read under those taps, int16 -> fp32; every odd case is resolved there by a bounds
// test per sample (2-byte loads: a src_off at an odd sample needs nothing; indices before 0 or from src_len on read as zero; taps outside
// 0 .. K - 1 are zero), so the MFMA loop has no conditions.  The accumulators stay in registers over the K-tiles and j ascends: the
// summation order of every output is fixed by construction, two runs agree bit for bit.  About 34 KB of LDS: four workgroups per CU.
//
// LDS layout of the signal run: position p lives at p + (p >> 5), ONE PAD FLOAT PER 32.  The A read of a half wavefront is 32 rows at
// a stride of 32 floats; with the pad the stride is 33, and 33 r mod 64 is distinct over r = 0 .. 31 (r for even r, r + 32 for odd r), so
// the 32 lanes fall into 32 different banks.  Chosen over the XOR swizzle because the run is addressed by a sliding position (p falls by
// one per step): with the pad the address is p plus a shift, and consecutive steps keep the banks distinct for free, while an XOR of
// the row bits would have to be recomputed against the column bits at every step -- in vector instructions, each of which takes 4-8
// cycles from the fp32 matrix stream (profiles/r05_mfma_coissue.txt); with the pad a trip's 16 positions share one block of 32 and their
// addresses are a uniform base, a per-lane constant and an immediate.  The two halves of a wavefront read at j and j + 1:
// their bank sets {33 r} and {33 r - 1} share one bank of 64.  The B read is 32 consecutive floats.
//
// The int16 output is saturate(rintf(.)) of the very register the fp32 output stores (re2e_wav_istft's rule).
#include "common.h"

#include <math.h>

namespace {

constexpr int RV_TILE = 1024;                              // outputs of one 32 x 32 tile
constexpr int RV_TILES = 1;                                // tiles per wavefront
constexpr int RV_WAVES = 4;
constexpr int RV_OT = RV_TILE * RV_TILES * RV_WAVES;       // outputs per workgroup
constexpr int RV_KT = 2048;                                // taps per K-tile
constexpr int RV_STEP = 16;                                // contraction steps per trip of the MFMA loop
constexpr int RV_CHUNK = 32;                               // jobs per launch: their index rows travel as a kernel argument
constexpr int RV_NJ = RV_KT + 32;                          // most steps of one K-tile (K-tile 0)
constexpr int RV_XS = RV_OT + RV_NJ;                       // staged signal positions
constexpr int RV_XS_FLOATS = RV_XS + RV_XS / 32 + 1;
constexpr int RV_HS_FLOATS = RV_NJ + 32;
constexpr long RV_LMAX = 2147483647L;

static_assert(RV_KT % RV_STEP == 0 && RV_STEP % 2 == 0, "a K-tile is a whole number of trips of step pairs");
static_assert(32 % RV_STEP == 0 && RV_TILE % RV_STEP == 0, "the positions of a trip lie in one padded block of 32");
static_assert((RV_XS_FLOATS + RV_HS_FLOATS) * 4 <= 65536, "static LDS");

struct RevJobs {                                           // read-only kernel argument (uniform index: scalar loads)
  long soff[RV_CHUNK], slen[RV_CHUNK], first[RV_CHUNK], count[RV_CHUNK], hoff[RV_CHUNK], hlen[RV_CHUNK], doff[RV_CHUNK];
};

__device__ __forceinline__ int xpad(int p) { return p + (p >> 5); }

__global__ __launch_bounds__(256) void wav_reverb_kernel(const short* __restrict__ pcm, const float* __restrict__ rir, const RevJobs u,
                                                         float* wav, short* out, int* __restrict__ clip_count) {
  __shared__ float xs[RV_XS_FLOATS];
  __shared__ float hs[RV_HS_FLOATS];
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long count = u.count[q];
  const long i0 = (long)blockIdx.x * RV_OT;
  if (i0 >= count) return;
  const long slen = u.slen[q], first = u.first[q];
  const int K = (int)u.hlen[q];
  const short* sp = pcm + u.soff[q];
  const float* hp = rir + u.hoff[q];
  const long left = count - i0;
  const int live = left >= RV_OT ? RV_OT : (int)((left + RV_TILE - 1) / RV_TILE) * RV_TILE;      // outputs of the tiles that hold any
  const int r = lane & 31, lh = lane >> 5;
  const int toff0 = wave * RV_TILES * RV_TILE;
  f32x16 acc[RV_TILES];
#pragma unroll
  for (int t = 0; t < RV_TILES; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  const int nkt = (K + RV_KT - 1) / RV_KT;
#pragma unroll 1
  for (int kt = 0; kt < nkt; ++kt) {
    const int jlo = kt == 0 ? -32 : kt * RV_KT;
    const int jhi = min(K, (kt + 1) * RV_KT);
    const int nj = (jhi - jlo + RV_STEP - 1) / RV_STEP * RV_STEP;         // <= RV_NJ
    for (int t = tid; t < nj + 32; t += 256) {                            // hs[t] = h[jlo + t]
      const int k = jlo + t;
      hs[t] = k >= 0 && k < K ? hp[k] : 0.f;
    }
    const long s0 = first + i0 - (jlo + nj) + 1;                          // xs position p holds x[s0 + p]
    for (int p = tid; p < live + nj; p += 256) {
      const long s = s0 + p;
      xs[xpad(p)] = s >= 0 && s < slen ? (float)sp[s] : 0.f;
    }
    __syncthreads();
    // Step j = jlo + jr reads B at hs[jr + c] (jr + c < nj + 32) and A at position toff + 32 r + nj - jr - 1 (0 .. live - 33 + nj).  A trip
    // takes jr = jj .. jj + RV_STEP - 1: with Q = toff + nj - jj - RV_STEP, a multiple of RV_STEP, its positions are Q + 32 r + e, e < RV_STEP,
    // all in ONE block of 32, so their padded address is xpad(Q) + 33 r + e: a uniform part per trip, a constant per lane and an immediate.
    // The loop then spends one vector instruction per operand and trip on addresses; every other one would cost the matrix stream 4-8
    // cycles (profiles/r05_mfma_coissue.txt).
    if (toff0 < live) {                                                   // (a wavefront whose tile holds no output only keeps the barriers)
      const float* al = xs + 33 * r - lh;
      const float* hb = hs + r + lh;
#pragma unroll 1
      for (int jj = 0; jj < nj; jj += RV_STEP) {
        const int Q = toff0 + nj - jj - RV_STEP;
        const float* ap = al + xpad(Q);
        float b[RV_STEP / 2], a[RV_TILES][RV_STEP / 2];
#pragma unroll
        for (int m = 0; m < RV_STEP / 2; ++m) {
          b[m] = hb[jj + 2 * m];
#pragma unroll
          for (int t = 0; t < RV_TILES; ++t) a[t][m] = ap[t * (RV_TILE + RV_TILE / 32) + RV_STEP - 1 - 2 * m];
        }
#pragma unroll
        for (int m = 0; m < RV_STEP / 2; ++m)
#pragma unroll
          for (int t = 0; t < RV_TILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][m], b[m], acc[t], 0, 0, 0);
      }
    }
    __syncthreads();                                                      // the runs are staged again for the next K-tile
  }
  const long base = u.doff[q];
  int clipped = 0;
#pragma unroll
  for (int t = 0; t < RV_TILES; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * lh;
      const long i = i0 + toff0 + t * RV_TILE + 32 * row + r;
      if (i < count) {
        const float v = acc[t][e];
        if (wav) wav[base + i] = v;
        if (out) {
          const float rv = rintf(v);
          if (rv > 32767.f || rv < -32768.f) ++clipped;
          out[base + i] = (short)fminf(32767.f, fmaxf(-32768.f, rv));
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

}  // namespace

extern "C" int re2e_wav_reverb_geometry(int which) {
  switch (which) {
    case 0: return RV_KT;
    case 1: return RV_OT;
    case 2: return RV_CHUNK;
    case 3: return RE2E_WAV_RIR_MAX;
    case 4: return RV_STEP;
    default: return -1;
  }
}

extern "C" int re2e_wav_reverb(const short* pcm, long pcm_samples, const float* rir, long rir_floats, const long* src_off, const long* src_len,
                               const long* first, const long* count, const long* rir_off, const long* rir_len, const long* dst_off, int n_jobs,
                               long out_samples, float* wav_f32, short* pcm_out, int* clip_count, hipStream_t stream) {
  RE2E_CHECK_ARG(pcm && rir && src_off && src_len && first && count && rir_off && rir_len && dst_off, "null operand");
  RE2E_CHECK_ARG(wav_f32 || pcm_out, "no output: wav_f32 and pcm_out are both NULL");
  RE2E_CHECK_ARG(n_jobs >= 1, "bad shape (n_jobs < 1)");
  RE2E_CHECK_ARG(pcm_samples > 0 && rir_floats > 0 && out_samples > 0, "bad shape");
  for (int q = 0; q < n_jobs; ++q) {
    RE2E_CHECK_ARG(rir_len[q] >= 1 && rir_len[q] <= RE2E_WAV_RIR_MAX, "a filter length outside 1 .. RE2E_WAV_RIR_MAX taps");
    RE2E_CHECK_ARG(src_len[q] >= 1 && src_len[q] <= RV_LMAX, "a source length outside 1 .. 2^31 - 1");
    RE2E_CHECK_ARG(src_off[q] >= 0 && src_off[q] <= pcm_samples - src_len[q], "a source range outside 0 .. pcm_samples");
    RE2E_CHECK_ARG(rir_off[q] >= 0 && rir_off[q] <= rir_floats - rir_len[q], "a filter range outside 0 .. rir_floats");
    RE2E_CHECK_ARG(first[q] >= 0 && count[q] >= 1, "first < 0 or count < 1");
    RE2E_CHECK_ARG(first[q] <= src_len[q] && count[q] <= src_len[q] - first[q], "first + count beyond src_len");
    RE2E_CHECK_ARG(dst_off[q] >= 0 && dst_off[q] <= out_samples - count[q], "a destination range outside 0 .. out_samples");
  }
  if (pcm_out == pcm) {                          // in place: the reverberant signals land behind the uploaded samples of the same blob
    RE2E_CHECK_ARG(out_samples <= pcm_samples, "in place (pcm_out is pcm): out_samples beyond pcm_samples");
    for (int q = 0; q < n_jobs; ++q)
      for (int s = 0; s < n_jobs; ++s)
        RE2E_CHECK_ARG(dst_off[q] + count[q] <= src_off[s] || src_off[s] + src_len[s] <= dst_off[q],
                       "in place (pcm_out is pcm): a destination range overlaps a source range of the same call");
  }
  for (int q0 = 0; q0 < n_jobs; q0 += RV_CHUNK) {
    const int nq = n_jobs - q0 < RV_CHUNK ? n_jobs - q0 : RV_CHUNK;
    RevJobs u;
    long longest = 0;                            // the longest job of the chunk sizes the grid
    for (int i = 0; i < RV_CHUNK; ++i) {
      const int q = q0 + (i < nq ? i : 0);
      u.soff[i] = src_off[q]; u.slen[i] = src_len[q]; u.first[i] = first[q]; u.count[i] = count[q];
      u.hoff[i] = rir_off[q]; u.hlen[i] = rir_len[q]; u.doff[i] = dst_off[q];
      if (count[q] > longest) longest = count[q];
    }
    hipLaunchKernelGGL(wav_reverb_kernel, dim3(cdiv(longest, RV_OT), nq), dim3(256), 0, stream, pcm, rir, u, wav_f32, pcm_out, clip_count);
    RE2E_LAUNCH_CHECK();
  }
  return RE2E_OK;
}
