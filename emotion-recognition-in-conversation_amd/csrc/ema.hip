// Exponential moving average of the parameters (lumo/contrib/module/ema.py:51-61, MMIN's ema_model): one elementwise launch over
// the flat parameter buffer, ema = alpha * ema + (1 - alpha) * p as two rounded products and one rounded sum (no fused
// multiply-add), the order of the reference's tensor expression.  alpha arrives as a float: 1 - alpha is formed from that float in
// double and rounded, so it differs from the reference's (1 - 0.999 in double, then rounded) by at most the rounding of alpha,
// 2^-25 -- an element then differs from a torch run by at most 2^-25 |p| and one unit in the last place of the result.
#include "erc_common.h"

namespace {
__global__ __launch_bounds__(256) void ema_kernel(float* ema, const float* p, int64_t n, float alpha, float one_minus) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float a = alpha * ema[i], b = one_minus * p[i];
        ema[i] = a + b;
    }
}
}  // namespace

extern "C" int erc_ema_step(float* ema, const float* p, int64_t n, float alpha, void* stream) {
    ERC_REQUIRE(ema && p && n > 0 && n <= ((int64_t)1 << 31) * 255, "ema_step: bad arguments (n=%lld)", (long long)n);
    ERC_REQUIRE(alpha >= 0.f && alpha <= 1.f, "ema_step: alpha=%g outside [0, 1]", (double)alpha);
    const float one_minus = (float)(1.0 - (double)alpha);
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ema, p, n, alpha, one_minus);
    ERC_LAUNCH_CHECK("ema_step");
    return ERC_OK;
}
