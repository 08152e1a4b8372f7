// vpt_mat4_sums.h — the constant part of mvp_inv * (x, y, -+1, 1), summed once per matrix on the host (PassArgs.mvp_near / mvp_far;
// vpt_device.h mat4_mul_point).  Host only, nothing of the project's: tests/test_matrix_sums.py builds it with a host compiler.
// The kernels used to start each component with fma(m[8+i], -+1, m[12+i]) per lane: the product with -+1 is exact, so the fma rounds
// once, exactly as the subtraction and the addition below.  volatile: one IEEE operation each, nothing to contract or reassociate.
#pragma once
static inline void mat4_point_sums(const float *m, float *near4, float *far4) {
    for (int i = 0; i < 4; i++) {
        volatile float lo = m[12 + i] - m[8 + i], hi = m[12 + i] + m[8 + i];
        near4[i] = lo; far4[i] = hi;
    }
}
