// The total order of the draws of one element (include/epx.h: "Posterior quantiles"): a double is ordered by the key
// k(x) = its IEEE-754 bits as uint64, all bits flipped when the sign bit is set, the sign bit set otherwise, so that
// -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers.  Included by quantiles.inc, by rank_diag.hip, which
// ranks a coordinate's draws by the same keys, and by predict.hip for predict_order.inc; quantiles.py (key_of / value_of)
// states the same in NumPy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace epx {

constexpr uint64_t ORDER_KEY_SIGN = 0x8000000000000000ull;
constexpr uint64_t ORDER_KEY_PAD = 0xffffffffffffffffull;      // behind every value (the key of a NaN with all bits set)

__host__ __device__ inline uint64_t order_key(double x) {
    union { double d; uint64_t u; } v;
    v.d = x;
    return (v.u & ORDER_KEY_SIGN) ? ~v.u : (v.u | ORDER_KEY_SIGN);
}

__host__ __device__ inline double order_value(uint64_t k) {
    union { double d; uint64_t u; } v;
    v.u = (k & ORDER_KEY_SIGN) ? (k & ~ORDER_KEY_SIGN) : ~k;
    return v.d;
}

}  // namespace epx
