// Loudness and true-peak output stage (host/loudness.py): the ITU-R BS.1770-4 meter at 48 kHz, the static gain and the look-ahead
// peak limiter.  Waveforms are x [B, C, N] fp32 with C in {1, 2}; row (b, c) starts at x + (b*C + c)*ld, ld >= N.
//
//   kweight_chunks_kernel   the K-weighting cascade (two biquads, transposed direct form II, fp64 state) over chunks of 480
//                           samples, one lane per chunk.  <false>: every chunk from zero state, its four end-state values kept;
//                           <true>: every chunk from its true initial state, sum y^2 per chunk, the ten chunk sums of a hop added
//                           in chunk order.  Between the two, kweight_carry_kernel advances s_{k+1} = T s_k + end_k per row (T:
//                           the chunk's 4x4 homogeneous transition, built on the host) and leaves each chunk's initial state.
//   loudness_gate_kernel    hop energies -> 400 ms blocks -> absolute (-70 LUFS) and relative (-10 LU) gate -> integrated loudness.
//   true_peak_kernel        p[n] = max_c max(|x[n]|, |u[4n+1]|, |u[4n+2]|, |u[4n+3]|), u the 4x oversampled signal (three 12-tap
//                           phases, taps from the host), and its maximum per clip.
//   limiter_kernel          r = min(1, c / (G p)), sliding minimum over [m, m+W] by doubling steps, box mean over [n-W, n], y = G g x.
//   gain_kernel             y = G x: one fp32 multiply per sample.
// No floating-point atomics anywhere: every sum has one fixed order, the maxima go through integer atomicMax on the bit pattern of
// non-negative floats.
#include "kernels.h"

namespace {

// ---- K-weighting (BS.1770-4, 48 kHz), a0 = 1
constexpr double KW_B0 = 1.53512485958697, KW_B1 = -2.69169618940638, KW_B2 = 1.19839281085285;
constexpr double KW_A1 = -1.69065929318241, KW_A2 = 0.73248077421585;
constexpr double KH_B0 = 1.0, KH_B1 = -2.0, KH_B2 = 1.0;
constexpr double KH_A1 = -1.99004745483398, KH_A2 = 0.99007225036621;

constexpr int LK_CHUNK = 480, LK_HOP = 4800, LK_CPH = LK_HOP / LK_CHUNK;   // ten chunks per hop
constexpr int LK_CPB = 60;                       // chunks per workgroup (one wave, 60 of its lanes): six whole hops
constexpr int LK_SUB = 96, LK_PITCH = LK_SUB + 1;  // staged sub-tile of a chunk; odd pitch: the lanes' reads hit 60 distinct banks

struct Mat4 { double m[16]; };

template <bool ENERGY>
__global__ __launch_bounds__(64) void kweight_chunks_kernel(const float* __restrict__ x, long ld, int nck, double* __restrict__ work,
                                                            double* __restrict__ e, int nh) {
  __shared__ float tile[LK_CPB * LK_PITCH];
  __shared__ double csum[LK_CPB];
  const int lane = threadIdx.x, row = blockIdx.y;
  const int ck0 = blockIdx.x * LK_CPB;
  const int chunk = ck0 + lane;
  const bool active = lane < LK_CPB && chunk < nck;
  const float* xr = x + (long)row * ld;
  double* w = work + ((long)row * nck + chunk) * 4;
  double s1 = 0., s2 = 0., t1 = 0., t2 = 0., acc = 0.;
  if (ENERGY && active) { s1 = w[0]; s2 = w[1]; t1 = w[2]; t2 = w[3]; }
  for (int sub = 0; sub < LK_CHUNK; sub += LK_SUB) {
    __syncthreads();
    for (int el = lane; el < LK_CPB * LK_SUB; el += 64) {       // coalesced: 96 consecutive floats per chunk
      const int ck = el / LK_SUB, i = el - ck * LK_SUB;
      const int g = ck0 + ck;
      tile[ck * LK_PITCH + i] = g < nck ? xr[(long)g * LK_CHUNK + sub + i] : 0.f;     // g < nck: below nh * 4800 <= N
    }
    __syncthreads();
    if (active) {
      const float* t = tile + lane * LK_PITCH;
      for (int i = 0; i < LK_SUB; ++i) {
        const double xv = (double)t[i];
        const double y1 = __builtin_fma(KW_B0, xv, s1);
        s1 = __builtin_fma(KW_B1, xv, __builtin_fma(-KW_A1, y1, s2));
        s2 = __builtin_fma(KW_B2, xv, -KW_A2 * y1);
        const double y2 = __builtin_fma(KH_B0, y1, t1);
        t1 = __builtin_fma(KH_B1, y1, __builtin_fma(-KH_A1, y2, t2));
        t2 = __builtin_fma(KH_B2, y1, -KH_A2 * y2);
        if (ENERGY) acc = __builtin_fma(y2, y2, acc);
      }
    }
  }
  if (!ENERGY) {
    if (active) { w[0] = s1; w[1] = s2; w[2] = t1; w[3] = t2; }
    return;
  }
  if (lane < LK_CPB) csum[lane] = active ? acc : 0.;
  __syncthreads();
  const int hop = blockIdx.x * (LK_CPB / LK_CPH) + lane;
  if (lane < LK_CPB / LK_CPH && hop < nh) {
    double s = 0.;
    for (int k = 0; k < LK_CPH; ++k) s += csum[lane * LK_CPH + k];      // chunk order
    e[(long)row * nh + hop] = s;
  }
}

// One wave per row; lane 0 walks the chunks (the recurrence is 4 x 4 per step), the wave moves 64 chunks' values through LDS so
// that no global load sits on the dependent chain.  In place: ends in, initial states out.
__global__ __launch_bounds__(64) void kweight_carry_kernel(double* __restrict__ work, int nck, Mat4 T) {
  __shared__ double buf[64 * 4];
  const int lane = threadIdx.x;
  double* w = work + (long)blockIdx.x * nck * 4;
  double s[4] = {0., 0., 0., 0.};
  for (int base = 0; base < nck; base += 64) {
    const int n4 = min(64, nck - base) * 4;
    for (int i = lane; i < n4; i += 64) buf[i] = w[(long)base * 4 + i];
    __syncthreads();
    if (lane == 0) {
      for (int i = 0; i < n4; i += 4) {
        double nx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          nx[r] = __builtin_fma(T.m[r * 4 + 0], s[0], __builtin_fma(T.m[r * 4 + 1], s[1],
                  __builtin_fma(T.m[r * 4 + 2], s[2], __builtin_fma(T.m[r * 4 + 3], s[3], buf[i + r]))));
#pragma unroll
        for (int r = 0; r < 4; ++r) { buf[i + r] = s[r]; s[r] = nx[r]; }
      }
    }
    __syncthreads();
    for (int i = lane; i < n4; i += 64) w[(long)base * 4 + i] = buf[i];
    __syncthreads();
  }
}

// ---- gate: one wave per clip
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // butterfly: every lane ends with the same bits
  return v;
}

__device__ __forceinline__ double block_z(const double* __restrict__ e, int C, int nh, int j) {
  double z = 0.;
  for (int c = 0; c < C; ++c)
    for (int h = 0; h < 4; ++h) z += e[(long)c * nh + j + h];
  return z / 19200.;
}

__global__ __launch_bounds__(64) void loudness_gate_kernel(const double* __restrict__ e, int C, int nh, double* __restrict__ lufs,
                                                           double* __restrict__ gamma, double* __restrict__ block_lufs) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nb = nh - 3;
  const double* eb = e + (long)b * C * nh;
  const double ninf = -__builtin_inf();
  double sum = 0., cnt = 0.;
  for (int j = lane; j < nb; j += 64) {
    const double z = block_z(eb, C, nh, j);
    const double l = -0.691 + 10. * log10(z);
    block_lufs[(long)b * nb + j] = l;
    if (l > -70.) { sum += z; cnt += 1.; }
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  double L = ninf, G = ninf;
  if (cnt > 0.) {
    G = -0.691 + 10. * log10(sum / cnt) - 10.;
    double sum2 = 0., cnt2 = 0.;
    for (int j = lane; j < nb; j += 64) {
      const double z = block_z(eb, C, nh, j);
      const double l = -0.691 + 10. * log10(z);
      if (l > -70. && l > G) { sum2 += z; cnt2 += 1.; }
    }
    sum2 = wave_sum(sum2);
    cnt2 = wave_sum(cnt2);
    if (cnt2 > 0.) L = -0.691 + 10. * log10(sum2 / cnt2);
  }
  if (lane == 0) { lufs[b] = L; gamma[b] = G; }
}

// ---- true peak and limiter
constexpr int TP_TILE = 1024, TP_LO = 5, TP_HI = 6;        // u[4n + r] reads x[n - 5 .. n + 6]
constexpr int LIM_WMAX = 480;
struct Taps { float h[36]; };                              // [3 phases][12]: h[r - 1][j + 5] multiplies x[n + j]

// stage x[row, n_lo .. n_lo + len) into LDS, zero outside [0, N)
__device__ __forceinline__ void stage_row(const float* __restrict__ xr, int N, long n_lo, int len, float* __restrict__ xs) {
  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    const long n = n_lo + i;
    xs[i] = (n >= 0 && n < N) ? xr[n] : 0.f;
  }
}

// xs[i] is x[n]; the caller guarantees xs[i - 5 .. i + 6]
__device__ __forceinline__ float peak4(const float* __restrict__ xs, int i, const Taps& t) {
  float p = fabsf(xs[i]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float u = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) u = __builtin_fmaf(xs[i - TP_LO + j], t.h[r * 12 + j], u);
    p = fmaxf(p, fabsf(u));
  }
  return p;
}

__device__ __forceinline__ float block_max_256(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void true_peak_kernel(const float* __restrict__ x, int C, int N, long ld, Taps taps,
                                                        unsigned* __restrict__ tp, unsigned* __restrict__ sp, float* __restrict__ env) {
  __shared__ float xs[TP_TILE + TP_LO + TP_HI];
  __shared__ float red[8];
  const int b = blockIdx.y;
  const long n0 = (long)blockIdx.x * TP_TILE;
  float p[TP_TILE / 256], a[TP_TILE / 256];
#pragma unroll
  for (int k = 0; k < TP_TILE / 256; ++k) p[k] = a[k] = 0.f;
  for (int c = 0; c < C; ++c) {
    __syncthreads();
    stage_row(x + ((long)b * C + c) * ld, N, n0 - TP_LO, TP_TILE + TP_LO + TP_HI, xs);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TP_TILE / 256; ++k) {
      const int i = threadIdx.x + k * 256;
      if (n0 + i < N) {
        p[k] = fmaxf(p[k], peak4(xs, i + TP_LO, taps));
        a[k] = fmaxf(a[k], fabsf(xs[i + TP_LO]));
      }
    }
  }
  float pm = 0.f, am = 0.f;
#pragma unroll
  for (int k = 0; k < TP_TILE / 256; ++k) {
    const int i = threadIdx.x + k * 256;
    if (env && n0 + i < N) env[(long)b * N + n0 + i] = p[k];
    pm = fmaxf(pm, p[k]);
    am = fmaxf(am, a[k]);
  }
  pm = block_max_256(pm, red);
  if (threadIdx.x == 0) atomicMax(tp + b, __float_as_uint(pm));      // non-negative floats order as their bit patterns
  if (sp) {
    am = block_max_256(am, red + 4);
    if (threadIdx.x == 0) atomicMax(sp + b, __float_as_uint(am));
  }
}

__global__ __launch_bounds__(256) void gain_kernel(const float* __restrict__ x, int C, int N, long ld, const float* __restrict__ gain,
                                                   float* __restrict__ y, long ldy) {
  const int row = blockIdx.y;
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float G = gain[row / C];
  const float v = x[(long)row * ld + n];
  y[(long)row * ldy + n] = G == 0.f ? v : G * v;           // gain 0 marks a clip that is passed through unchanged
}

// One workgroup = TP_TILE output samples of one clip.  LDS (floats): xs [TILE + 2W + 11] the staged channel, later a ping-pong buffer;
// ra [TILE + 2W] the envelope, then r on [n0 - W, n0 + TILE + W); rb [TILE + 2W] the other ping-pong buffer.
__global__ __launch_bounds__(256) void limiter_kernel(const float* __restrict__ x, int C, int N, long ld, const float* __restrict__ gain,
                                                      double ceil_lin, int W, Taps taps, float* __restrict__ y, long ldy,
                                                      float* __restrict__ g_out) {
  constexpr int RMAX = TP_TILE + 2 * LIM_WMAX;
  __shared__ float xs[RMAX + TP_LO + TP_HI];
  __shared__ float ra[RMAX];
  __shared__ float rb[RMAX];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long n0 = (long)blockIdx.x * TP_TILE;
  const float G = gain[b];
  if (G == 0.f) {                                            // passed through unchanged
    for (int c = 0; c < C; ++c)
      for (int i = tid; i < TP_TILE; i += 256)
        if (n0 + i < N) y[((long)b * C + c) * ldy + n0 + i] = x[((long)b * C + c) * ld + n0 + i];
    if (g_out)
      for (int i = tid; i < TP_TILE; i += 256)
        if (n0 + i < N) g_out[(long)b * N + n0 + i] = 1.f;
    return;
  }
  const int R = TP_TILE + 2 * W;                             // r positions: sample n0 - W + i
  for (int c = 0; c < C; ++c) {
    __syncthreads();
    stage_row(x + ((long)b * C + c) * ld, N, n0 - W - TP_LO, R + TP_LO + TP_HI, xs);
    __syncthreads();
    for (int i = tid; i < R; i += 256) {
      const float p = peak4(xs, i + TP_LO, taps);
      ra[i] = c == 0 ? p : fmaxf(ra[i], p);
    }
  }
  __syncthreads();
  for (int i = tid; i < R; i += 256) {
    const long n = n0 - W + i;
    float r = 1.f;
    if (n >= 0 && n < N) {
      // c / (G p) in fp64 (the product of two fp32 values is exact there), rounded DOWN to fp32: G r p <= c up to fp64 rounding
      const double q = ceil_lin / ((double)G * (double)ra[i]);
      r = q >= 1. ? 1.f : __double2float_rd(q);
    }
    ra[i] = r;
  }
  __syncthreads();
  // sliding minimum over [i, i + W]: K doubling steps give windows of P = 2^K <= W + 1, two of them cover W + 1
  const int L = W + 1;
  const float* cur = ra;
  float* nxt = rb;
  int P = 1, valid = R;
  while (2 * P <= L) {
    valid -= P;
    for (int i = tid; i < valid; i += 256) nxt[i] = fminf(cur[i], cur[i + P]);
    __syncthreads();
    P *= 2;
    cur = nxt;
    nxt = cur == rb ? xs : rb;
  }
  const int M = TP_TILE + W;                                 // gmin positions: sample n0 - W + i
  for (int i = tid; i < M; i += 256) nxt[i] = fminf(cur[i], cur[i + L - P]);
  __syncthreads();
  const float* gm = nxt;
  const float fl = (float)L;
  for (int i = tid; i < TP_TILE; i += 256) {
    if (n0 + i >= N) continue;
    float s = 0.f;
    for (int t = 0; t < L; ++t) s += gm[i + t];              // m = n - W .. n, in that order
    const float g = fminf(s / fl, ra[i + W]);                // every window holds n: g <= r[n] but for rounding, which the min removes
    if (g_out) g_out[(long)b * N + n0 + i] = g;
    const float Gg = G * g;
    for (int c = 0; c < C; ++c) y[((long)b * C + c) * ldy + n0 + i] = Gg * x[((long)b * C + c) * ld + n0 + i];
  }
}

int check_wave(const void* x, int B, int C, int N, long ld, const char* what) {
  if (!x || B < 1 || N < 1 || ld < N) return foley_set_err(what, __FILE__, __LINE__);
  if (C != 1 && C != 2) return foley_set_err("loudness: 1 or 2 channels", __FILE__, __LINE__);
  return 0;
}

}  // namespace

int launch_loudness_energy(const float* x, int B, int C, int N, long ld, const double* T16, double* work, int64_t work_doubles,
                           double* e, hipStream_t st) {
  if (int rc = check_wave(x, B, C, N, ld, "loudness_energy: x [B, C, N] with ld >= N")) return rc;
  if (!T16) return foley_set_err("loudness_energy: the chunk transition matrix is required", __FILE__, __LINE__);
  const int nh = N / LK_HOP;
  if (nh < 1) return 0;                                      // no complete hop: e is empty
  const int nck = nh * LK_CPH, rows = B * C;
  if (!work || !e || work_doubles < (int64_t)rows * nck * 4)
    return foley_set_err("loudness_energy: work needs B * C * (N / 4800) * 40 doubles", __FILE__, __LINE__);
  Mat4 T;
  for (int i = 0; i < 16; ++i) T.m[i] = T16[i];
  const dim3 grid((nck + LK_CPB - 1) / LK_CPB, rows);
  FOLEY_LAUNCH(kweight_chunks_kernel<false>, grid, dim3(64), 0, st, x, ld, nck, work, e, nh);
  FOLEY_LAUNCH(kweight_carry_kernel, dim3(rows), dim3(64), 0, st, work, nck, T);
  FOLEY_LAUNCH(kweight_chunks_kernel<true>, grid, dim3(64), 0, st, x, ld, nck, work, e, nh);
  return 0;
}

int launch_loudness_gate(const double* e, int B, int C, int nh, double* lufs, double* gamma, double* block_lufs, hipStream_t st) {
  if (!e || !lufs || !gamma || B < 1 || nh < 0 || (C != 1 && C != 2) || (nh > 3 && !block_lufs))
    return foley_set_err("loudness_gate: e [B, C, nh], lufs / gamma [B], block_lufs [B, nh - 3]", __FILE__, __LINE__);
  FOLEY_LAUNCH(loudness_gate_kernel, dim3(B), dim3(64), 0, st, e, C, nh, lufs, gamma, block_lufs);
  return 0;
}

static Taps load_taps(const float* taps36) {
  Taps t;
  for (int i = 0; i < 36; ++i) t.h[i] = taps36[i];
  return t;
}

int launch_true_peak(const float* x, int B, int C, int N, long ld, const float* taps36, float* tp, float* sp, float* env,
                     hipStream_t st) {
  if (int rc = check_wave(x, B, C, N, ld, "true_peak: x [B, C, N] with ld >= N")) return rc;
  if (!taps36 || !tp) return foley_set_err("true_peak: taps and the peak output are required", __FILE__, __LINE__);
  FOLEY_CHECK_HIP(hipMemsetAsync(tp, 0, sizeof(float) * B, st));
  if (sp) FOLEY_CHECK_HIP(hipMemsetAsync(sp, 0, sizeof(float) * B, st));
  FOLEY_LAUNCH(true_peak_kernel, dim3((N + TP_TILE - 1) / TP_TILE, B), dim3(256), 0, st, x, C, N, ld, load_taps(taps36),
               (unsigned*)tp, (unsigned*)sp, env);
  return 0;
}

int launch_loudness_apply(const float* x, int B, int C, int N, long ld, const float* gain, int limiter, double ceil_lin, int W,
                          const float* taps36, float* y, long ldy, float* g_out, hipStream_t st) {
  if (int rc = check_wave(x, B, C, N, ld, "loudness_apply: x [B, C, N] with ld >= N")) return rc;
  if (!gain || !y || ldy < N) return foley_set_err("loudness_apply: gain [B], y [B, C, N] with ldy >= N", __FILE__, __LINE__);
  if (!limiter) {
    if (g_out) return foley_set_err("loudness_apply: the gain curve exists in limiter mode only", __FILE__, __LINE__);
    FOLEY_LAUNCH(gain_kernel, dim3((N + 255) / 256, B * C), dim3(256), 0, st, x, C, N, ld, gain, y, ldy);
    return 0;
  }
  if (!taps36 || W < 1 || W > LIM_WMAX || !(ceil_lin > 0.))
    return foley_set_err("loudness_apply: limiter needs taps, 1 <= W <= 480 and a positive ceiling", __FILE__, __LINE__);
  FOLEY_LAUNCH(limiter_kernel, dim3((N + TP_TILE - 1) / TP_TILE, B), dim3(256), 0, st, x, C, N, ld, gain, ceil_lin, W,
               load_taps(taps36), y, ldy, g_out);
  return 0;
}
