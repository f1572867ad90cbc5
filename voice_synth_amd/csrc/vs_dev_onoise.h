/*
 * vs_dev_onoise.h -- one output-noise sample of vowel -n, literally and as the noise kernel computes it.
 * Included behind vs_dev_primitives.h by vs_out_noise.hip, whose kernel it serves, and by vs_selftest.hip, which holds
 * the short form to the literal one.
 */
#ifndef VS_DEV_ONOISE_H
#define VS_DEV_ONOISE_H

/* One noise sample, literally (vowel_new.c:315-317); r = the draw, what random() returns. */
__device__ __forceinline__ int vs_onoise_literal(int y, uint32_t r, float ndw)
{
  const float noiseval = (float)vs_unit_of_draw(r);
  const float aux = (float)((double)ndw * ((double)noiseval - 0.5));
  return vs_round2int(1.0 * (double)y + 1.0 * (double)aux);
}
/* ... and as the noise kernel computes it, 19 vector instructions per sample instead of 34 (and the kernel is bound by them:
 * Philox alone is 9.4).
 *   noiseval: (float)((1.0*r)/RAND_MAX) is the float next to r/(2^31 - 1) = r*2^-31*(1 + 2^-31 + ...): an integer r of
 *     up to 31 bits rounded to 24, where the tail only ever decides an exact tie (upwards).  r*inv, inv = RN(1/RAND_MAX),
 *     is within an ulp of the quotient -- 2^-52 relative, where no integer r lies closer than 2^-31 relative to a point
 *     that rounds the other way -- so the two correction steps of vs_unit_of_draw() cannot matter behind the
 *     conversion (device self-test [7]: all 2^31 draws).
 *   aux: noiseval - 0.5 is exact in double, so RN(NoiseDistWidth * (noiseval - 0.5)) is ONE fused multiply-add,
 *     fma(NoiseDistWidth, noiseval, -NoiseDistWidth/2): the same exact quantity, rounded once, to double; then to float.
 *   rounding: y is an integer, so round2int(y + aux) = clamp(y + ceil(aux - 0.5)) for every float aux outside
 *     (-2^-38, 0): where the double sum y + aux rounds at all (|aux| < 2^-14) it stays strictly between y - 1 and y + 1 on
 *     aux's side of y, at least 2^-38 - 2^-40 away from the integers the reference's "x + 1" could round up to.  Inside
 *     that interval round2int has its quirks (x + 1 rounds to an integer: vs_dev_primitives.h).  A nonzero aux is at
 *     least NoiseDistWidth * 2^-25 in magnitude (the floats next to one half), so a frame whose width is 0 or >= 2^-13
 *     never meets the interval: the test is per FRAME, not per sample.  ceil(aux - 0.5) = -floor(-aux + 0.5) is ONE
 *     instruction on gfx950, V_CVT_RPI_I32_F32.
 *   clamp: widths below 65534 keep |aux| <= 32767, the rounded value fits 16 bits, and two samples are subtracted,
 *     saturated and lifted from -32768 to the reference's -32767 as a pair (V_CVT_PK_I16_I32, V_PK_SUB_I16 clamp,
 *     V_PK_MAX_I16) straight from the packed words of the row.
 * Frames outside [2^-13, 65534) (an SNR beyond ~90 dB, or below 0 dB on a clipped signal: the ABI takes any out_snr > 0)
 * take the literal form.  Self-test [7]: every float outside (-2^-38, 0) at nine values of y. */
__device__ __forceinline__ bool vs_onoise_width_is_plain(float ndw) { return (ndw == 0.0f) || (ndw >= 0x1p-13f && ndw < 65534.0f); }
__device__ __forceinline__ bool vs_onoise_aux_is_plain(float aux)
{
  return (__float_as_uint(aux) - 0x80000001u) > 0x2C7FFFFEu; /* not in (-2^-38, -0) */
}
/* floor(-aux + 0.5) = -ceil(aux - 0.5) */
__device__ __forceinline__ int vs_onoise_neg_round(float aux)
{
  int r;
  asm("v_cvt_rpi_i32_f32_e64 %0, -%1" : "=v"(r) : "v"(aux));
  return r;
}
__device__ __forceinline__ int vs_onoise_neg_round_of_draw(uint32_t o, double ndw, double neg_half_ndw)
{
  const float noiseval = (float)((double)(o >> 1) * 0x1.00000002p-31);
  return vs_onoise_neg_round((float)__builtin_fma(ndw, (double)noiseval, neg_half_ndw));
}
/* {y.lo - r0, y.hi - r1}, each saturated to int16 and lifted to >= -32767; |r0|, |r1| <= 32767 */
__device__ __forceinline__ uint32_t vs_onoise_sub2(uint32_t ypair, int r0, int r1)
{
  const vs_i16x2 r = __builtin_amdgcn_cvt_pk_i16(r0, r1);
  uint32_t d;
  asm("v_pk_sub_i16 %0, %1, %2 clamp" : "=v"(d) : "v"(ypair), "v"(__builtin_bit_cast(uint32_t, r)));
  const vs_i16x2 floor_ = {(short)-32767, (short)-32767};
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(vs_i16x2, d), floor_));
}

#endif
