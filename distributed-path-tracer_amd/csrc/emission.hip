// First-hit emission around the filters (ptx_emission_split, ptx_emission_merge). The filters work on radiance / albedo; what a pixel's
// first surface emits is not proportional to its albedo, so it is taken out of the half-buffers before a filter call and put back, unfiltered,
// into the filter's output:  col = (col - e) + e  with  e = emission.rgb / float(guide_spp), the mean of ptx_render_emission's sums.
//   k_em_split   a.c -= a.w * e.c (and b the same): the halves hold SUMS over a.w samples of the pixel
//   k_em_merge   out.c += e.c: the filter's output holds MEANS
// A channel whose e is not > 0 (zero, negative, NaN) is left without arithmetic, so a frame without emission keeps every bit, signed zeros
// and NaNs included. .w is never written differently from how it was read. One lane per pixel, one 16-byte load and store per buffer:
// consecutive lanes touch consecutive float4s. Numerics as in kernels.hip: IEEE binary32, every operation rounded on its own, no contraction.
#include "device_core.hpp"

namespace ptx {

constexpr int kEmBlock = 256;

DEV float4 em_mean(const float4* __restrict__ emission, size_t p, float ng) {
	const float4 E = emission[p];
	return make_float4(E.x / ng, E.y / ng, E.z / ng, 0.f);
}

DEV float4 em_take(float4 A, float4 e) {
	if (e.x > 0) A.x = A.x - (A.w * e.x);
	if (e.y > 0) A.y = A.y - (A.w * e.y);
	if (e.z > 0) A.z = A.z - (A.w * e.z);
	return A;
}

template <bool TWO>
__global__ void __launch_bounds__(kEmBlock) k_em_split(const float4* __restrict__ emission, float ng, size_t n_pixels, float4* __restrict__ a, float4* __restrict__ b) {
	const size_t p = (size_t)blockIdx.x * kEmBlock + threadIdx.x;
	if (p >= n_pixels) return;
	const float4 e = em_mean(emission, p, ng);
	a[p] = em_take(a[p], e);
	if constexpr (TWO) b[p] = em_take(b[p], e);
}

__global__ void __launch_bounds__(kEmBlock) k_em_merge(const float4* __restrict__ emission, float ng, size_t n_pixels, float4* __restrict__ out) {
	const size_t p = (size_t)blockIdx.x * kEmBlock + threadIdx.x;
	if (p >= n_pixels) return;
	const float4 e = em_mean(emission, p, ng);
	float4 O = out[p];
	if (e.x > 0) O.x = O.x + e.x;
	if (e.y > 0) O.y = O.y + e.y;
	if (e.z > 0) O.z = O.z + e.z;
	out[p] = O;
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_emission_split(const float4* emission, uint32_t guide_spp, size_t n_pixels, float4* a, float4* b, hipStream_t stream) {
	const dim3 grid((unsigned)((n_pixels + kEmBlock - 1) / kEmBlock));
	const float ng = (float)guide_spp;
	if (b) hipLaunchKernelGGL(k_em_split<true>, grid, dim3(kEmBlock), 0, stream, emission, ng, n_pixels, a, b);
	else hipLaunchKernelGGL(k_em_split<false>, grid, dim3(kEmBlock), 0, stream, emission, ng, n_pixels, a, b);
	return hipGetLastError();
}

hipError_t launch_emission_merge(const float4* emission, uint32_t guide_spp, size_t n_pixels, float4* out, hipStream_t stream) {
	hipLaunchKernelGGL(k_em_merge, dim3((unsigned)((n_pixels + kEmBlock - 1) / kEmBlock)), dim3(kEmBlock), 0, stream, emission, (float)guide_spp, n_pixels, out);
	return hipGetLastError();
}

}  // namespace ptx
