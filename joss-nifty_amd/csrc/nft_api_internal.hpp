// Internal cross-file declarations of the nifty_amd C-ABI library.
#pragma once
#include "nft_common.hpp"
#include "fft_core.hpp"

namespace nft {
namespace fast {
template <typename T> struct FastArgs;
}
// one engine-v2 pass (fast_dispatch.hpp: launch) on fp64 data; the kernels are
// instantiated in nft_fft.hip only
int fast_pass_f64(int kind, bool rows, int N, fast::FastArgs<double>& a, hipStream_t s);
const char* last_error();
int get_twiddles(int n, int dtype, const void** out);
FftPlanDev make_plan(int n);
int scale_real(void* x, long long n, int dtype, double scale, hipStream_t s);
}  // namespace nft
