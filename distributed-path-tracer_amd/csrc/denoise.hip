// Variance-guided a-trous filter on the guide buffers (ptx_denoise; the specification is in include/ptx.h and DESIGN.md §5.5). The reference
// has no denoiser: every value here is defined by that text, IEEE binary32, one rounding per operation in the written parenthesisation.
//   k_dn_prepare     per pixel: demodulated colour (col), the half-frame luminance variance estimate v0, the filter's guide (mean normal,
//                    mean depth) and what the last pass needs to re-modulate (albedo, alpha)
//   k_dn_prepare_counts   the same for half-buffers with per-pixel sample counts (ptx_denoise_counts); everything after it is shared
//   k_dn_prefilter   3 x 3 geometry-weighted mean of v0 -> var
//   k_dn_atrous      one iteration: 25 taps at distance `step`, in row-major order. Two forms of the same arithmetic (atrous_pixel):
//                    TILED = false gathers the taps from global memory; TILED = true stages them in LDS first. The pixels congruent
//                    mod `step` form a dense 5 x 5 stencil on a decimated sub-image, so a workgroup that owns a 16 x 16 tile of one
//                    sub-lattice needs that tile + 2 halo texels whatever the step. The tap order per pixel is the same in both.
// State per pixel: (col.rgb, var), ping-ponged between two buffers, and (nrm.xyz, z), constant over the iterations.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ptx {

constexpr int kDnBlockX = 64, kDnBlockY = 4;   // global form: one wave per 64-pixel row segment, 1 KiB per tap
constexpr int kDnWaves = 4;   // a-trous kernels: waves per SIMD the register budget must leave room for
constexpr int kDnTile = 16, kDnHalo = 2, kDnSpan = kDnTile + 2 * kDnHalo;   // tiled form: 16 x 16 pixels of one sub-lattice + 2 texels around

__device__ __forceinline__ float dn_bw(float x) {
	const float t = fmaxf(0.0f, 1.0f - x);
	return t * t;
}
__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// geometric weight of tap q seen from p; g = (nrm.xyz, z)
__device__ __forceinline__ float dn_geo(const float4& gp, const float4& gq, float sn2, float sz2) {
	const float dx = gp.x - gq.x, dy = gp.y - gq.y, dz = gp.z - gq.z;
	const float xn = ((dx * dx + dy * dy) + dz * dz) / sn2;
	const float zm = fmaxf(gp.w, gq.w);
	const float rel = zm > 0.0f ? (gp.w - gq.w) / zm : 0.0f;
	const float xz = (rel * rel) / sz2;
	return dn_bw(xn) * dn_bw(xz);
}

__global__ void __launch_bounds__(256) k_dn_prepare(const float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ albedo_cov,
                                                    const float4* __restrict__ normal_depth, float n, float na, float nb, size_t n_pixels,
                                                    float4* __restrict__ col_var, float4* __restrict__ guide, float4* __restrict__ remod) {
	const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (p >= n_pixels) return;
	const float4 A = a[p], B = b[p], G = albedo_cov[p], N = normal_depth[p];
	const float cov = G.w, miss = n - cov;   // missed samples count as albedo 1
	const float ax = fmaxf((G.x + miss) / n, 0.001f), ay = fmaxf((G.y + miss) / n, 0.001f), az = fmaxf((G.z + miss) / n, 0.001f);
	const float d = (dn_lum((A.x / na) / ax, (A.y / na) / ay, (A.z / na) / az) - dn_lum((B.x / nb) / ax, (B.y / nb) / ay, (B.z / nb) / az)) * 0.5f;
	col_var[p] = make_float4(((A.x + B.x) / n) / ax, ((A.y + B.y) / n) / ay, ((A.z + B.z) / n) / az, d * d);
	guide[p] = cov > 0.0f ? make_float4(N.x / cov, N.y / cov, N.z / cov, N.w / cov) : make_float4(0.f, 0.f, 0.f, 0.f);
	remod[p] = make_float4(ax, ay, az, (A.w + B.w) / n);
}

// k_dn_prepare for half-buffers that carry their own per-pixel sample counts in .w (ptx_denoise_counts: what ptx_render_adaptive and
// ptx_render_adaptive_nee leave); the guides are sums over ng samples of every pixel. A zero half count gives a non-finite pixel.
__global__ void __launch_bounds__(256) k_dn_prepare_counts(const float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ albedo_cov,
                                                           const float4* __restrict__ normal_depth, float ng, size_t n_pixels, float4* __restrict__ col_var,
                                                           float4* __restrict__ guide, float4* __restrict__ remod) {
	const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (p >= n_pixels) return;
	const float4 A = a[p], B = b[p], G = albedo_cov[p], N = normal_depth[p];
	const float na = A.w, nb = B.w, n = na + nb;
	const float cov = G.w, miss = ng - cov;   // missed samples count as albedo 1
	const float ax = fmaxf((G.x + miss) / ng, 0.001f), ay = fmaxf((G.y + miss) / ng, 0.001f), az = fmaxf((G.z + miss) / ng, 0.001f);
	const float d = (dn_lum((A.x / na) / ax, (A.y / na) / ay, (A.z / na) / az) - dn_lum((B.x / nb) / ax, (B.y / nb) / ay, (B.z / nb) / az)) * 0.5f;
	col_var[p] = make_float4(((A.x + B.x) / n) / ax, ((A.y + B.y) / n) / ay, ((A.z + B.z) / n) / az, d * d);
	guide[p] = cov > 0.0f ? make_float4(N.x / cov, N.y / cov, N.z / cov, N.w / cov) : make_float4(0.f, 0.f, 0.f, 0.f);
	remod[p] = make_float4(ax, ay, az, (A.w + B.w) / n);
}

__global__ void __launch_bounds__(kDnBlockX* kDnBlockY) k_dn_prefilter(const float4* __restrict__ in, const float4* __restrict__ guide, int W, int H, float sigma_n, float sigma_z,
                                                                      float4* __restrict__ out) {
	const int x = blockIdx.x * kDnBlockX + threadIdx.x, y = blockIdx.y * kDnBlockY + threadIdx.y;
	if (x >= W || y >= H) return;
	const float sn2 = sigma_n * sigma_n, sz2 = sigma_z * sigma_z;
	const size_t p = (size_t)y * W + x;
	const float4 cp = in[p], gp = guide[p];
	float s0 = 0.0f, s1 = 0.0f;
	for (int dy = -1; dy <= 1; dy++) {
		for (int dx = -1; dx <= 1; dx++) {
			const int qx = x + dx, qy = y + dy;
			if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
			const size_t q = (size_t)qy * W + qx;
			const float g = (dx == 0 && dy == 0) ? 1.0f : dn_geo(gp, guide[q], sn2, sz2);
			s0 += g;
			s1 += g * in[q].w;
		}
	}
	out[p] = make_float4(cp.x, cp.y, cp.z, s1 / s0);
}

// One pixel of one iteration. tap(dx, dy, qx, qy, c, g) fetches (col, var) and the guide of the tap at (qx, qy) = p + step * (dx, dy) CLAMPED to
// the image, so the fetches of a row of taps need no branch and are in flight together; what a tap outside the image fetched is never used.
template <class Tap>
__device__ __forceinline__ float4 atrous_pixel(int x, int y, int W, int H, int step, float sl2, float sn2, float sz2, const float4& cp, const float4& gp, Tap tap) {
	const float kern[3] = {0.375f, 0.25f, 0.0625f};
	const float Lp = dn_lum(cp.x, cp.y, cp.z);
	const float den = (sl2 * cp.w) + 1e-8f;
	float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f, av = 0.0f;
#pragma nounroll   // one row of taps (ten fetches) in flight at a time: unrolled, the fetches of all five rows are hoisted and the registers spill
	for (int dy = -2; dy <= 2; dy++) {
		const int qy = y + dy * step;   // |dy * step| <= 256 and y < 16384: no overflow
		const int qyc = qy < 0 ? 0 : (qy >= H ? H - 1 : qy);
		const float ky = dy == 0 ? kern[0] : ((dy == 1 || dy == -1) ? kern[1] : kern[2]);
		float4 cq[5], gq[5];
#pragma unroll
		for (int dx = -2; dx <= 2; dx++) {   // the centre tap fetches the pixel itself
			const int qx = x + dx * step;
			tap(dx, dy, qx < 0 ? 0 : (qx >= W ? W - 1 : qx), qyc, cq[dx + 2], gq[dx + 2]);
		}
#pragma unroll
		for (int dx = -2; dx <= 2; dx++) {
			const int qx = x + dx * step;
			const float4 c = cq[dx + 2];
			const float h = kern[dx < 0 ? -dx : dx] * ky;
			const float dl = Lp - dn_lum(c.x, c.y, c.z);
			float w = (h * dn_geo(gp, gq[dx + 2], sn2, sz2)) * dn_bw((dl * dl) / den);
			if (dx == 0) w = dy == 0 ? h : w;   // the centre tap
			// a tap outside the image is skipped, and so is one with !(w > 0), NaN weights too: a non-finite pixel stays itself and
			// contaminates no neighbour. A skipped tap adds nothing, not even 0 * NaN
			const bool take = qx >= 0 && qx < W && qy >= 0 && qy < H && w > 0.0f;
			ar = take ? ar + w * c.x : ar;
			ag = take ? ag + w * c.y : ag;
			ab = take ? ab + w * c.z : ab;
			ws = take ? ws + w : ws;
			av = take ? av + (w * w) * c.w : av;
		}
	}
	return make_float4(ar / ws, ag / ws, ab / ws, av / (ws * ws));
}

// LAST: the iteration writes the caller's buffer, re-modulated, instead of the state
template <bool LAST>
__device__ __forceinline__ void atrous_store(const float4& r, size_t p, const float4* __restrict__ remod, float4* __restrict__ out) {
	if constexpr (LAST) {
		const float4 m = remod[p];
		out[p] = make_float4(r.x * m.x, r.y * m.y, r.z * m.z, m.w);
	} else {
		out[p] = r;
	}
}

template <bool LAST>
__global__ void __launch_bounds__(kDnBlockX* kDnBlockY, kDnWaves) k_dn_atrous(const float4* __restrict__ in, const float4* __restrict__ guide, const float4* __restrict__ remod, int W, int H,
                                                                   int step, float sigma_l, float sigma_n, float sigma_z, float4* __restrict__ out) {
	const int x = blockIdx.x * kDnBlockX + threadIdx.x, y = blockIdx.y * kDnBlockY + threadIdx.y;
	if (x >= W || y >= H) return;
	const size_t p = (size_t)y * W + x;
	const float4 cp = in[p], gp = guide[p];
	const float4 r = atrous_pixel(x, y, W, H, step, sigma_l * sigma_l, sigma_n * sigma_n, sigma_z * sigma_z, cp, gp, [&](int, int, int qx, int qy, float4& cq, float4& gq) {
		const size_t q = (size_t)qy * W + qx;
		cq = in[q];
		gq = guide[q];
	});
	atrous_store<LAST>(r, p, remod, out);
}

// grid.x = tiles per sub-image row * residues in x, grid.y likewise: the residue is the fast index, so neighbouring workgroups read
// neighbouring pixels
template <bool LAST>
__global__ void __launch_bounds__(kDnTile* kDnTile, kDnWaves) k_dn_atrous_tiled(const float4* __restrict__ in, const float4* __restrict__ guide, const float4* __restrict__ remod, int W,
                                                                     int H, int step, int res_x, int res_y, float sigma_l, float sigma_n, float sigma_z, float4* __restrict__ out) {
	__shared__ float4 s_col[kDnSpan][kDnSpan], s_gd[kDnSpan][kDnSpan];
	const int rx = blockIdx.x % res_x, ry = blockIdx.y % res_y;               // the sub-lattice
	const int tx = (blockIdx.x / res_x) * kDnTile, ty = (blockIdx.y / res_y) * kDnTile;   // the tile's origin in the decimated sub-image
	const int tid = threadIdx.y * kDnTile + threadIdx.x;
	for (int i = tid; i < kDnSpan * kDnSpan; i += kDnTile * kDnTile) {
		const int hx = i % kDnSpan, hy = i / kDnSpan;
		const int qx = rx + (tx + hx - kDnHalo) * step, qy = ry + (ty + hy - kDnHalo) * step;   // |.| < 16384 + 18 * 128: no overflow
		if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;   // never used: atrous_pixel skips taps outside the image
		const size_t q = (size_t)qy * W + qx;
		s_col[hy][hx] = in[q];
		s_gd[hy][hx] = guide[q];
	}
	__syncthreads();
	const int lx = threadIdx.x + kDnHalo, ly = threadIdx.y + kDnHalo;
	const int x = rx + (tx + (int)threadIdx.x) * step, y = ry + (ty + (int)threadIdx.y) * step;
	if (x >= W || y >= H) return;
	const float4 r = atrous_pixel(x, y, W, H, step, sigma_l * sigma_l, sigma_n * sigma_n, sigma_z * sigma_z, s_col[ly][lx], s_gd[ly][lx], [&](int dx, int dy, int, int, float4& cq, float4& gq) {
		cq = s_col[ly + dy][lx + dx];
		gq = s_gd[ly + dy][lx + dx];
	});
	atrous_store<LAST>(r, (size_t)y * W + x, remod, out);
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_denoise_prepare(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, uint32_t spp_a, uint32_t spp_b, size_t n_pixels,
                                  float4* col_var, float4* guide, float4* remod, hipStream_t stream) {
	hipLaunchKernelGGL(k_dn_prepare, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, a, b, albedo_cov, normal_depth, (float)(spp_a + spp_b), (float)spp_a,
	                   (float)spp_b, n_pixels, col_var, guide, remod);
	return hipGetLastError();
}

hipError_t launch_denoise_prepare_counts(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, uint32_t guide_spp, size_t n_pixels,
                                         float4* col_var, float4* guide, float4* remod, hipStream_t stream) {
	hipLaunchKernelGGL(k_dn_prepare_counts, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, a, b, albedo_cov, normal_depth, (float)guide_spp, n_pixels, col_var, guide,
	                   remod);
	return hipGetLastError();
}

hipError_t launch_denoise_prefilter(const float4* in, const float4* guide, uint32_t W, uint32_t H, float sigma_n, float sigma_z, float4* out, hipStream_t stream) {
	const dim3 grid((W + kDnBlockX - 1) / kDnBlockX, (H + kDnBlockY - 1) / kDnBlockY), block(kDnBlockX, kDnBlockY);
	hipLaunchKernelGGL(k_dn_prefilter, grid, block, 0, stream, in, guide, (int)W, (int)H, sigma_n, sigma_z, out);
	return hipGetLastError();
}

hipError_t launch_denoise_atrous(const float4* in, const float4* guide, const float4* remod, uint32_t W, uint32_t H, uint32_t step, float sigma_l, float sigma_n, float sigma_z,
                                 bool last, bool tiled, float4* out, hipStream_t stream) {
	if (tiled) {
		// residues that hold a pixel, and the tiles of the largest sub-image (residue 0)
		const uint32_t res_x = step < W ? step : W, res_y = step < H ? step : H;
		const uint32_t sub_w = (W + step - 1) / step, sub_h = (H + step - 1) / step;
		const dim3 grid(res_x * ((sub_w + kDnTile - 1) / kDnTile), res_y * ((sub_h + kDnTile - 1) / kDnTile)), block(kDnTile, kDnTile);
		if (last) hipLaunchKernelGGL(k_dn_atrous_tiled<true>, grid, block, 0, stream, in, guide, remod, (int)W, (int)H, (int)step, (int)res_x, (int)res_y, sigma_l, sigma_n, sigma_z, out);
		else hipLaunchKernelGGL(k_dn_atrous_tiled<false>, grid, block, 0, stream, in, guide, remod, (int)W, (int)H, (int)step, (int)res_x, (int)res_y, sigma_l, sigma_n, sigma_z, out);
	} else {
		const dim3 grid((W + kDnBlockX - 1) / kDnBlockX, (H + kDnBlockY - 1) / kDnBlockY), block(kDnBlockX, kDnBlockY);
		if (last) hipLaunchKernelGGL(k_dn_atrous<true>, grid, block, 0, stream, in, guide, remod, (int)W, (int)H, (int)step, sigma_l, sigma_n, sigma_z, out);
		else hipLaunchKernelGGL(k_dn_atrous<false>, grid, block, 0, stream, in, guide, remod, (int)W, (int)H, (int)step, sigma_l, sigma_n, sigma_z, out);
	}
	return hipGetLastError();
}

}  // namespace ptx
