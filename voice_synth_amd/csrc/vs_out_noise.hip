/*
 * vs_out_noise.hip -- vowel -n (reference vowel_new.c:302-324): white noise added to the filtered signal, frame by frame
 * (Lframe = 800 samples at 16 kHz, 1100 at 22.05 kHz, vw:361-363):
 *     aux = 0; for every sample of the frame: aux += (float)y[i]*y[i];                (float, in sample order)
 *     sig_power = aux / (float)ni;  NoiseDistWidth = sqrt(12*sig_power/snr);          (float)
 *     noiseval = (1.0*random())/RAND_MAX;  aux = NoiseDistWidth*(noiseval - 0.5);     (float <- double)
 *     y[i] = round2int(1.0*y[i] + 1.0*aux);
 * The power of a WHOLE frame stands in front of its first noise sample, so this is two streaming passes over the
 * finished PCM, behind whatever kernel wrote it (the fused wave-specialised kernels, the one-wave kernel, the wide
 * filter kernel -- none of them knows about frames):
 *   vs_out_power_kernel  one thread per (utterance, frame): the sequential float sum, then NoiseDistWidth -> ondw[row][frame];
 *   vs_out_noise_kernel  one thread per 8 samples: the vowel process draws once per sample, in order, so draw n belongs
 *                        to sample n -- two Philox blocks per thread, every sample independent.
 * 2 B/sample read + 4 B/sample read and written, only when asked for.
 */
#include "vs_kernel_table.h"
#include "vs_dev_generator.h"
#include "vs_dev_filter.h"
#include "vs_dev_onoise.h"

/* aux += (float)y*y over the 8 samples of 16 bytes of a row, in sample order (vowel_new.c:304-306) */
__device__ __forceinline__ void vs_power8(const vs_u32x4 v, float &aux)
{
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = (float)(int)(int16_t)(v[e] & 0xFFFFu), hi = (float)((int)v[e] >> 16);
    aux += lo * lo;
    aux += hi * hi;
  }
}

/* NoiseDistWidth of frame fr of the utterance of record L (row `row`), or of nothing (NaN is never read) behind its end */
template <bool VEC>
__device__ __forceinline__ float vs_frame_width(const VsKernelArgs &args, const VsDevLane *__restrict__ L, long row, int fr, float snr)
{
  const int N = args.n_samples;
  const int Lframe = L->Lframe;
  const long f0 = (long)fr * Lframe;
  if (f0 >= N) return __uint_as_float(VS_ONDW_UNKNOWN);
  const int left = N - (int)f0;
  const int ni = (left < Lframe) ? left : Lframe;
  const int16_t *__restrict__ fp = args.out + row * args.out_pitch + f0;
  float aux = 0.0f;
  int i = 0;
  if (VEC) {
    /* frames start on even samples (Lframe is a multiple of 100) of rows that start on 4-byte boundaries: 16-byte
     * loads, eight of them -- one 128-byte line of this thread's frame -- in flight before the first is used, so a
     * line is asked for once although 64 threads of a wavefront read 64 different frames */
    const vs_u32x4 *__restrict__ vp = (const vs_u32x4 *)fp;
    const int nvec = ni >> 3;
    int c = 0;
    for (; c + 8 <= nvec; c += 8) {
      vs_u32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = vp[c + j];
#pragma unroll
      for (int j = 0; j < 8; ++j) vs_power8(v[j], aux);
    }
    for (; c < nvec; ++c) vs_power8(vp[c], aux);
    i = nvec << 3;
  }
  for (; i < ni; ++i) {
    const float f = (float)fp[i];
    aux += f * f;
  }
  return vs_noise_width(aux, ni, snr);
}

/* every frame: one thread per (utterance, frame) */
template <bool VEC>
__global__ void __launch_bounds__(256) vs_out_power_kernel(VsKernelArgs args)
{
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long l = gid / args.ondw_pitch;
  if (l >= (long)args.n_lanes) return;
  const int fr = (int)(gid - l * args.ondw_pitch);
  const VsDevLane *__restrict__ L = args.lanes + l;
  const float snr = L->out_snr;
  if (!(snr > 0.0f)) return;
  const long row = (long)L->row;
  args.ondw[row * args.ondw_pitch + fr] = vs_frame_width<VEC>(args, L, row, fr, snr);
}

/* Behind a fused kernel that took the frame powers along (vs_synth_ws_pow_kernel): one thread per utterance looks through
 * its row of the table and does what that kernel left -- the frames behind its last whole super-step (args.odone[row] says
 * where they start) and the ones it marked unknown because the quirk path of round2int() ran during them (VsFramePower). */
template <bool VEC>
__global__ void __launch_bounds__(64) vs_out_power_fill_kernel(VsKernelArgs args)
{
  const long l = (long)blockIdx.x * 64 + threadIdx.x;
  if (l >= (long)args.n_lanes) return;
  const VsDevLane *__restrict__ L = args.lanes + l;
  const float snr = L->out_snr;
  if (!(snr > 0.0f)) return;
  const long row = (long)L->row;
  float *__restrict__ wrow = args.ondw + row * args.ondw_pitch;
  const int done = args.odone[row];
  const int frames = (int)(((long)args.n_samples + L->Lframe - 1) / L->Lframe);
  for (int fr = 0; fr < frames; ++fr)
    if (fr >= done || __float_as_uint(wrow[fr]) == VS_ONDW_UNKNOWN) wrow[fr] = vs_frame_width<VEC>(args, L, row, fr, snr);
}

/* VS_ONOISE_OCTETS octets of 8 samples per thread, 256 threads apart (measurement builds: -DVS_ONOISE_OCTETS=1 ...) */
#ifndef VS_ONOISE_OCTETS
#define VS_ONOISE_OCTETS 1
#endif
#ifndef VS_ONOISE_ROWMAJOR
#define VS_ONOISE_ROWMAJOR 1
#endif
template <bool VEC>
__global__ void __launch_bounds__(256) vs_out_noise_kernel(VsKernelArgs args, unsigned segs, unsigned seg_magic, unsigned seg_shift)
{
  constexpr int OCT = VS_ONOISE_OCTETS;
  /* one workgroup = 256 * OCT octets of ONE utterance: its key, frame length and row are wave-uniform */
#if VS_ONOISE_ROWMAJOR
  /* consecutive workgroups walk along a row: utterance = block / segs by the launcher's multiplier (scalar) */
  const unsigned lane_idx = (segs == 1u) ? blockIdx.x : ((unsigned)(((unsigned long long)blockIdx.x * seg_magic) >> 32) >> seg_shift);
  const unsigned seg = blockIdx.x - lane_idx * segs;
#else
  const unsigned lane_idx = blockIdx.x, seg = blockIdx.y;
#endif
  const VsDevLane *__restrict__ L = args.lanes + lane_idx;
  const float snr = L->out_snr;
  if (!(snr > 0.0f)) return;
  const int N = args.n_samples;
  const int base = (int)((seg * (256u * OCT) + threadIdx.x) * 8u);
  if (base >= N) return;
  const long row = (long)L->row;
  int16_t *__restrict__ orow = args.out + row * args.out_pitch;
  const float *__restrict__ wrow = args.ondw + row * args.ondw_pitch;
  const uint32_t magic = L->lframe_magic;
  const int sh = 31 - __builtin_clz((unsigned)(L->Lframe - 1)); /* ceil(log2(Lframe)) - 1 */
  const uint32_t k0 = L->okey0, k1 = L->okey1;
  vs_u32x4 yp[OCT]; /* 8 samples each, packed as they lie in the row */
  float w0[OCT], w1[OCT];
#pragma unroll
  for (int c = 0; c < OCT; ++c) {
    const int i0 = base + c * 2048;
    if (i0 >= N) continue;
    const int16_t *op = orow + i0;
    if (VEC && (i0 + 8 <= N)) {
      yp[c] = *(const vs_u32x4 *)op;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        yp[c][e] = vs_pack16((i0 + 2 * e < N) ? (int)op[2 * e] : 0, (i0 + 2 * e + 1 < N) ? (int)op[2 * e + 1] : 0);
    }
    /* the frames of the two quads (Lframe is a multiple of 4, not of 8): i / Lframe by the record's multiplier */
    const int fr0 = (int)(__umulhi((uint32_t)i0, magic) >> sh);
    const int fr1 = (i0 + 4 < N) ? (int)(__umulhi((uint32_t)(i0 + 4), magic) >> sh) : fr0;
    w0[c] = wrow[fr0];
    w1[c] = wrow[fr1];
  }
#pragma unroll
  for (int c = 0; c < OCT; ++c) {
    const int i0 = base + c * 2048;
    if (i0 >= N) continue;
    int16_t *op = orow + i0;
    uint32_t o[8];
    vs_philox((uint32_t)(i0 >> 2), k0, k1, o[0], o[1], o[2], o[3]);
    vs_philox((uint32_t)(i0 >> 2) + 1u, k0, k1, o[4], o[5], o[6], o[7]);
    vs_u32x4 v = yp[c];
    if (vs_onoise_width_is_plain(w0[c]) && vs_onoise_width_is_plain(w1[c])) {
      const double d0 = (double)w0[c], d1 = (double)w1[c], h0 = -0.5 * d0, h1 = -0.5 * d1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r0 = vs_onoise_neg_round_of_draw(o[2 * e], (e < 2) ? d0 : d1, (e < 2) ? h0 : h1);
        const int r1 = vs_onoise_neg_round_of_draw(o[2 * e + 1], (e < 2) ? d0 : d1, (e < 2) ? h0 : h1);
        v[e] = vs_onoise_sub2(v[e], r0, r1);
      }
    } else {
      int y[8];
      vs_unpack8(v, y);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = vs_clamp_pack16(vs_onoise_literal(y[2 * e], o[2 * e] >> 1, (e < 2) ? w0[c] : w1[c]),
                               vs_onoise_literal(y[2 * e + 1], o[2 * e + 1] >> 1, (e < 2) ? w0[c] : w1[c]));
    }
    if (VEC && (i0 + 8 <= N)) {
      *(vs_u32x4 *)op = v;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (i0 + k < N) op[k] = (int16_t)((k & 1) ? (v[k >> 1] >> 16) : (v[k >> 1] & 0xFFFFu));
    }
  }
}

#define VS_E_OUT_POWER(V) {VS_KERNEL_ID(VS_KF_OUT_POWER, V, 0, 0, 0), vs_out_power_kernel<V>}
#define VS_E_OUT_POWER_FILL(V) {VS_KERNEL_ID(VS_KF_OUT_POWER_FILL, V, 0, 0, 0), vs_out_power_fill_kernel<V>}
#define VS_E_OUT_NOISE(V) {VS_KERNEL_ID(VS_KF_OUT_NOISE, V, 0, 0, 0), vs_out_noise_kernel<V>}
const VsKernelEntry vs_kernel_table_out_power[] = {VS_E_OUT_POWER(false), VS_E_OUT_POWER(true), VS_E_OUT_POWER_FILL(false),
                                                   VS_E_OUT_POWER_FILL(true), {0, nullptr}};
const VsNoiseTable vs_noise_table = {VS_ONOISE_OCTETS, VS_ONOISE_ROWMAJOR, {VS_E_OUT_NOISE(false), VS_E_OUT_NOISE(true)}};
