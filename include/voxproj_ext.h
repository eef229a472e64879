/*
 * voxproj_ext.h -- entry points of libvoxproj.so added after the 64 functions of voxproj.h.  Same library, same vp_ prefix,
 * same error codes and vp_last_error(); VP_ABI_VERSION does not change, a caller detects these functions by symbol.
 * voxproj.h stays as it is: what it declares is frozen.
 */
#ifndef VOXPROJ_EXT_H
#define VOXPROJ_EXT_H

#include "voxproj.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * View-dependent colour: spherical harmonics (SH) of degree 0 .. 3, the appearance model of the reference's Gaussians
 * (utils/sh_utils.py:57-112, gaussian_renderer/__init__.py:67-72).  A per-Gaussian pre-pass: it produces the colour rows
 * f32 [N,3] that vp_splat_rasterize and its loss / backward entry points take as features, and the adjoint carries the
 * colour gradient those return on to the coefficients and, through the view direction, to the means.
 * tests/sh_reference.py states the contract in NumPy.
 *
 * Parameters (the reference's layout, coefficient index before channel): f_dc f32 [N,3], f_rest f32 [N,Kr,3] with
 * Kr = (max_degree + 1)^2 - 1, rows contiguous (3 Kr floats apart); means f32 [N,3]; campos: the camera centre, three HOST
 * floats (-R^T t of a world-to-camera matrix); degree: the active degree, 0 <= degree <= max_degree <= 3.  Coefficients
 * beyond the active degree are not read.  With sh[0] = f_dc, sh[k] = f_rest[k - 1], all arithmetic fp32 without contraction:
 *
 *   p = mean - campos;  r = sqrtf((p.x p.x + p.y p.y) + p.z p.z);  (x, y, z) = r > 0 ? p / r : (0, 0, 0)
 *   pre[c]    = (sum over k < (degree + 1)^2 of Y_k(x, y, z) sh[k][c], added in ascending k) + 0.5
 *   colors[c] = max(pre[c], 0);   bit c of clamped = (pre[c] < 0)
 *
 *   Y_0  =  0.28209479177387814
 *   Y_1  = -0.4886025119029199 y              Y_2  =  0.4886025119029199 z              Y_3  = -0.4886025119029199 x
 *   Y_4  =  1.0925484305920792 xy             Y_5  = -1.0925484305920792 yz             Y_6  =  0.31539156525252005 (2zz - xx - yy)
 *   Y_7  = -1.0925484305920792 xz             Y_8  =  0.5462742152960396 (xx - yy)
 *   Y_9  = -0.5900435899266435 y (3xx - yy)   Y_10 =  2.890611442640554 xyz             Y_11 = -0.4570457994644658 y (4zz - xx - yy)
 *   Y_12 =  0.3731763325901154 z (2zz - 3xx - 3yy)                                      Y_13 = -0.4570457994644658 x (4zz - xx - yy)
 *   Y_14 =  1.445305721320277 z (xx - yy)     Y_15 = -0.5900435899266435 x (xx - 3yy)
 *
 * vp_sh_colors writes colors f32 [N,3] and, when not NULL, clamped u8 [N].
 *
 * vp_sh_colors_backward takes grad_colors f32 [N,3] and the clamped bytes of the forward; the gradient passes where
 * pre[c] >= 0 (torch's clamp_min): g[c] = bit c of clamped ? 0 : grad_colors[c].  Each output may be NULL:
 *   grad_dc   f32 [N,3]     = Y_0 g
 *   grad_rest f32 [N,Kr,3]  = Y_k g[c] for k < (degree + 1)^2, exact zeros beyond: the array is written whole
 *   grad_means f32 [N,3]    = r > 0 ? (q - dir (dir . q)) / r : 0,  q = sum_k (sum_c sh[k][c] g[c]) grad Y_k(x, y, z)
 * f_dc is never read by the backward (Y_0 is a constant) and may be NULL; f_rest is read only when grad_means is wanted
 * and degree > 0, and may be NULL otherwise.
 *
 * Both calls: no workspace, no atomics, bit-identical from run to run, asynchronous on `stream`; n = 0 is valid and
 * launches nothing.  VP_EINVAL, decided on the host before any launch: n outside [0, 2^31 - 1], degrees outside
 * 0 <= degree <= max_degree <= 3, a NULL or non-finite campos, a NULL array that the call reads or must write (n > 0), an
 * array pointer that is not 4-byte aligned.  16-byte accesses are used wherever the addresses allow; a base that is only
 * 4-byte aligned (a row-offset view) is correct and costs one narrower access at each end of a workgroup's stretch.
 */
int vp_sh_colors(const float *f_dc, const float *f_rest, const float *means, const float *campos, int64_t n, int degree,
                 int max_degree, float *colors, uint8_t *clamped, void *stream);
int vp_sh_colors_backward(const float *f_dc, const float *f_rest, const float *means, const float *campos, int64_t n,
                          int degree, int max_degree, const float *grad_colors, const uint8_t *clamped, float *grad_dc,
                          float *grad_rest, float *grad_means, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXPROJ_EXT_H */
