// dt_common.h -- what the two modes of the domain transform filter share (dt_filter_kernels.hip: DTF_RF;
// dt_window_kernels.hip: DTF_NC): a guide pixel and the L1 difference of two, the output conversion, the parameters as the
// reference clamps them and its sigma schedule.
#pragma once

#include "adf_host.h"

#include <cmath>
#include <type_traits>

namespace adf {

// A guide pixel as one word, and the L1 difference of two of them.
template <int CH> __device__ __forceinline__ unsigned pixel(const uint8_t* g)
{
    unsigned v = g[0];
    if constexpr (CH == 3) v |= (unsigned)g[1] << 8 | (unsigned)g[2] << 16;
    return v;
}
template <int CH> __device__ __forceinline__ int l1(unsigned p, unsigned q)
{
    int s = abs((int)(p & 255) - (int)(q & 255));
    if constexpr (CH == 3) s += abs((int)(p >> 8 & 255) - (int)(q >> 8 & 255)) + abs((int)(p >> 16 & 255) - (int)(q >> 16 & 255));
    return s;
}

// dst = x in the output's depth: x, or rint (half to even) saturated; a NaN gives the depth's minimum.
template <class T> __device__ __forceinline__ T convert(float x)
{
    if constexpr (std::is_same<T, float>::value) {
        return x;
    } else {
        const float lo = std::is_same<T, uint8_t>::value ? 0.0f : -32768.0f, hi = std::is_same<T, uint8_t>::value ? 255.0f : 32767.0f;
        const float v = rintf(x);
        return !(v >= lo) ? (T)lo : v > hi ? (T)hi : (T)v;
    }
}

// The parameters as DT.inl:79-83 clamps them.
struct DtParams { float ss, sr; int N; };
inline DtParams clamped(double sigma_spatial, double sigma_color, int num_iters)
{
    return DtParams{std::max(1.0f, (float)sigma_spatial), std::max(0.01f, (float)sigma_color), std::max(1, num_iters)};
}

// sigmaH_i = ss * 2^(N-i) / sqrt(4^N - 1) in double, left to right (DT.hpp:120-123), i = 1..N.
inline double sigma_h(const DtParams& p, int i)
{
    return (double)p.ss * std::pow(2.0, (double)(p.N - i)) / std::sqrt(std::pow(4.0, (double)p.N) - 1.0);
}

} // namespace adf
